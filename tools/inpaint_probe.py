"""Region in-painting beside the staged mask path and beside sequential outpainting, on the MI355X (profiles/inpaint.md).

    python tools/inpaint_probe.py --what edge --sched ddim|ddpm --path staged|fused [--root TREE]
    python tools/inpaint_probe.py --what continue

The 256x256 default architecture (bench.py CFG256) with random weights, fp32, device events around each synchronised call, one warm-up
call per configuration first (plan, capture, first launches). One JSON line per measurement. One configuration per process, so that the
torch allocator peak is that configuration's own; `--root` points the imports at another checkout of this repository (the parent
commit's, built), so that one shell script can alternate the two builds in the same session.

edge:      edge-column in-painting at B = 16 through the pipeline call (`audio=False`: the codec of the input, the prologue, the loop,
           the u8 images; no image -> audio): the first and the last second of the slice are kept (43 columns each at 22050 Hz,
           hop 512). `staged` is `mask_start_secs` / `mask_end_secs` (a (B, steps, H, W) mask tensor, sliced per chunk); `fused` is
           `keep_mask` with the same columns at `known_level="current"` (the same images, byte for byte). ddim: 50 steps, three timed
           calls. ddpm: 1000 steps with `device_noise_seed`, one timed call. Reported: ms per call and per step, the torch allocator's
           peak over the timed calls, and the number of native loop calls one pipeline call makes.
continue:  the 4 x 1152 columns of profiles/windowed.md item 2, DDIM-50, the loops alone (no codec on either side): ONE windowed call at
           B = 4, frames = 1152, window_stride = 128 with the first 256 columns kept (what `longform.continue_track` runs), against
           `longform.outpaint`'s route: per sample seven continuation segments with the first 128 columns pinned by the staged mask,
           one sample at a time at B = 1 on a model with the single-sample layer rules (the first segment is the input, not generated:
           28 loops of 50 steps)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 128, 256, 256, 512, 512),
             down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
             up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
HW, B_EDGE, SECS = 256, 16, 1.0
B_WIDE, FRAMES, STRIDE = 4, 1152, 128
N_WIN = (FRAMES - HW) // STRIDE + 1


def timed(dev, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b), 3)


def pipeline(dev, sched, single_sample=False):
    import audiodiffusion as ad
    unet = ad.UNet2DModel(sample_size=(HW, HW), **BENCH).init_random(0)
    if single_sample:
        unet.set_option("wino6", 256)
        unet.set_option("single_sample", 1)
    pipe = ad.AudioDiffusionPipeline(None, unet, ad.Mel(x_res=HW, y_res=HW), sched()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def count_loop_calls():
    """-> a list that gains one entry per native loop call made from now on."""
    from audiodiffusion import _native as N
    real, calls = N.lib(), []

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("adm_sample_loop"):
                return fn

            def counted(*a):
                calls.append(name)
                return fn(*a)
            return counted
    N.lib = lambda: Spy()
    return calls


def edge(dev, sched_name, path):
    import audiodiffusion as ad
    ddpm = sched_name == "ddpm"
    pipe = pipeline(dev, ad.DDPMScheduler if ddpm else ad.DDIMScheduler)
    steps, runs = (1000, 1) if ddpm else (50, 3)
    audio = (0.2 * np.random.default_rng(0).standard_normal(HW * pipe.mel.hop_length)).astype(np.float32)
    noise = torch.randn(B_EDGE, 1, HW, HW, generator=torch.Generator().manual_seed(8)).to(dev)
    cols = int(SECS * HW * pipe.mel.get_sample_rate() / pipe.mel.x_res / pipe.mel.hop_length)
    kw = dict(batch_size=B_EDGE, raw_audio=audio, steps=steps, audio=False)
    if ddpm:
        kw["device_noise_seed"] = 1
    if path == "staged":
        kw.update(mask_start_secs=SECS, mask_end_secs=SECS)
    else:
        keep = np.zeros((HW, HW), np.uint8)
        keep[:, :cols] = 1
        keep[:, HW - cols:] = 1
        kw.update(keep_mask=torch.from_numpy(keep).to(dev), known_level="current")
    call = lambda: pipe(noise=noise.clone(), **kw)   # noqa: E731
    calls = count_loop_calls()
    call()
    per_call = len(calls)
    torch.cuda.synchronize(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    ms = [timed(dev, call) for _ in range(runs)]
    print(json.dumps(dict(what="edge", sched=sched_name, path=path, B=B_EDGE, steps=steps, kept_columns=2 * cols, ms=ms,
                          ms_per_step=[round(t / steps, 3) for t in ms], torch_peak_mib=round(torch.cuda.max_memory_allocated(dev) / 2 ** 20, 1),
                          native_loop_calls_per_pipeline_call=per_call)), flush=True)


def continuation(dev):
    import audiodiffusion as ad
    g = torch.Generator().manual_seed(8)
    pipe = pipeline(dev, ad.DDIMScheduler)
    pipe.scheduler.set_timesteps(50)
    wide, known, noise = (torch.randn(B_WIDE, 1, HW, FRAMES, generator=g).to(dev) for _ in range(3))
    keep = torch.zeros(HW, FRAMES, dtype=torch.uint8)
    keep[:, :HW] = 1
    keep = keep.to(dev)
    one_call = lambda: pipe._denoise(wide, 0, 0.0, None, None, 0, 0, window_stride=STRIDE, keep_mask=keep, known=known,   # noqa: E731
                                     known_noise=noise)
    free = lambda: pipe._denoise(wide, 0, 0.0, None, None, 0, 0, window_stride=STRIDE)   # noqa: E731
    one_call()
    tk = [timed(dev, one_call) for _ in range(3)]
    free()
    tf = [timed(dev, free) for _ in range(3)]
    print(json.dumps(dict(what="continue-one-call", B=B_WIDE, frames=FRAMES, window_stride=STRIDE, unet_batch=B_WIDE * N_WIN, steps=50,
                          keep_ms=tk, no_keep_ms=tf)), flush=True)
    del pipe
    torch.cuda.empty_cache()
    one = pipeline(dev, ad.DDIMScheduler, single_sample=True)
    one.scheduler.set_timesteps(50)
    x1 = torch.randn(1, 1, HW, HW, generator=g).to(dev)
    mask = torch.randn(1, 50, HW, HW, generator=g).to(dev)

    def sequential():
        for _ in range(B_WIDE * (N_WIN - 1)):
            one._denoise(x1, 0, 0.0, None, mask, HW - STRIDE, 0)         # a continuation: the first 128 columns pinned
    one._denoise(x1, 0, 0.0, None, mask, HW - STRIDE, 0)
    ts = [timed(dev, sequential) for _ in range(2)]
    print(json.dumps(dict(what="continue-sequential-b1", loops=B_WIDE * (N_WIN - 1), steps=50, ms=ts)), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("edge", "continue"), required=True)
    ap.add_argument("--sched", choices=("ddim", "ddpm"), default="ddim")
    ap.add_argument("--path", choices=("staged", "fused"), default="fused")
    ap.add_argument("--root", default=ROOT)
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path[:0] = [os.path.join(root, "audio-diffusion_amd"), root]
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    if args.what == "edge":
        edge(torch.device("cuda:0"), args.sched, args.path)
    else:
        continuation(torch.device("cuda:0"))
