"""Windowed sampling beside the ordinary loop and beside sequential outpainting, on the MI355X (profiles/windowed.md).

    python tools/windowed_probe.py [--trace]

The 256x256 default architecture (bench.py CFG256) with random weights, DDIM with 50 steps, the captured loop, device events around each
synchronised call, one warm-up call per configuration first (plan, capture, first launches). One JSON line per measurement.

default:  (1) the windowed loop at B = 4, frames = 1152, window_stride = 128 (8 windows per sample: UNet batch 32) against the ordinary
              loop at B = 32 on the same handle, alternating, PROBE_RUNS (default 3) timed calls each. The difference is what gather,
              blend and the wider step cost (the handle re-captures on every switch: that is inside the timed call and is reported
              as it is; the second line repeats the windowed loop back to back, replaying one graph).
          (2) the same 4 x 1152 columns as `longform.outpaint` makes them: per sample one 256-column segment and seven more with the
              first 128 columns pinned by the mask, one sample at a time (B = 1, 32 loops of 50 steps), on a model with the
              single-sample layer rules the `AudioDiffusion` facade selects. The loops alone: no codec on either side.
--trace:  one warm-up and one timed windowed call and nothing else, for a kernel trace taken from outside."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, RUNS = 50, int(os.environ.get("PROBE_RUNS", "3"))
BENCH = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 128, 256, 256, 512, 512),
             down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
             up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
HW, B_WIDE, FRAMES, STRIDE = 256, 4, 1152, 128
N_WIN = (FRAMES - HW) // STRIDE + 1


def timed(dev, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b), 3)


def pipeline(dev, single_sample=False):
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    unet = UNet2DModel(sample_size=(HW, HW), **BENCH).init_random(0)
    if single_sample:
        unet.set_option("wino6", 256)
        unet.set_option("single_sample", 1)
    pipe = AudioDiffusionPipeline(None, unet, Mel(x_res=HW, y_res=HW), DDIMScheduler()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    pipe.scheduler.set_timesteps(STEPS)
    return pipe


def main(dev, trace):
    g = torch.Generator().manual_seed(8)
    pipe = pipeline(dev)
    wide = torch.randn(B_WIDE, 1, HW, FRAMES, generator=g).to(dev)
    windowed = lambda: pipe._denoise(wide, 0, 0.0, None, None, 0, 0, window_stride=STRIDE)   # noqa: E731
    windowed()
    if trace:
        print(json.dumps(dict(what="windowed", ms=timed(dev, windowed))), flush=True)
        return
    batch = torch.randn(B_WIDE * N_WIN, 1, HW, HW, generator=g).to(dev)
    ordinary = lambda: pipe._denoise(batch, 0, 0.0, None, None, 0, 0)   # noqa: E731
    ordinary()
    tw, to = [], []
    for _ in range(RUNS):
        tw.append(timed(dev, windowed))
        to.append(timed(dev, ordinary))
    print(json.dumps(dict(what="alternating", steps=STEPS, unet_batch=B_WIDE * N_WIN, windowed_ms=tw, ordinary_ms=to,
                          windowed_ms_per_step=[round(t / STEPS, 3) for t in tw], ordinary_ms_per_step=[round(t / STEPS, 3) for t in to])),
          flush=True)
    windowed()
    tb = [timed(dev, windowed) for _ in range(RUNS)]
    ordinary()
    ob = [timed(dev, ordinary) for _ in range(RUNS)]
    print(json.dumps(dict(what="back-to-back", steps=STEPS, windowed_ms=tb, ordinary_ms=ob)), flush=True)
    del pipe
    torch.cuda.empty_cache()
    # sequential segments, one sample at a time
    one = pipeline(dev, single_sample=True)
    x1 = torch.randn(1, 1, HW, HW, generator=g).to(dev)
    mask = torch.randn(1, STEPS, HW, HW, generator=g).to(dev)

    def sequential():
        for _ in range(B_WIDE):
            one._denoise(x1, 0, 0.0, None, None, 0, 0)                       # the first segment
            for _ in range(N_WIN - 1):
                one._denoise(x1, 0, 0.0, None, mask, HW - STRIDE, 0)         # a continuation: the first 128 columns pinned
    one._denoise(x1, 0, 0.0, None, None, 0, 0)
    one._denoise(x1, 0, 0.0, None, mask, HW - STRIDE, 0)
    ts = [timed(dev, sequential) for _ in range(RUNS)]
    print(json.dumps(dict(what="sequential-b1", loops=B_WIDE * N_WIN, steps=STEPS, ms=ts,
                          ms_per_sample_step=[round(t / (B_WIDE * N_WIN * STEPS), 3) for t in ts])), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "audio-diffusion_amd"), ROOT]
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    main(torch.device("cuda:0"), args.trace)
