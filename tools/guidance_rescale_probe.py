"""Time per step of the captured guided sampling loop with and without guidance rescale, on the MI355X (profiles/guidance_rescale.md).

The conditional benchmark model (bench.py CFG_COND: (128, 256, 512, 512), CrossAttn blocks) at 256x256 with B = 16 and at 64x64 with
B = 1. Per configuration: one pipeline, DDIM, `_denoise` calls of PROBE_STEPS steps (default 5) at guidance_scale 3.0; per variant one
warm-up call (plan, capture, first launches) and then PROBE_RUNS (default 5) timed calls, one variant after the other; device events
around each call, divided by the steps. One JSON line per (configuration, variant) with every timed call, so that several processes
(this commit and its parent, alternated by the caller) can be pooled afterwards.

    python tools/guidance_rescale_probe.py [--pkg DIR] [--tag NAME] [--phi 0 0.7] [--kernels | --bits] [--only 64|256]

--pkg: the directory that holds the `audiodiffusion` package to time (default: this tree's); a tree from before the keyword existed takes
       only `--phi off`, which does not pass the keyword at all.
--kernels: instead of the loops, 20 thresholded rescaled guided steps through `ops.sched_step` on random buffers at both shapes, for a
       kernel trace taken from outside (the statistics kernel beside the selection kernel in the same run).
--bits: instead of the loops, one line per step and selection kernel of the build (mode x prediction x guided x noise source, the 26 + 6 of
       csrc/k_sched.hip, without the rescale) with a SHA-256 of its outputs on fixed inputs: the lines of two builds are compared as text.
--only: one of the two configurations, by its height (a kernel trace's statistics are per kernel name: one shape per traced process)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, RUNS = int(os.environ.get("PROBE_STEPS", "5")), int(os.environ.get("PROBE_RUNS", "5"))
BENCH = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
             down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
             cross_attention_dim=100, attention_head_dim=8)
CONFIGS = [(64, 1), (256, 16)]      # (height = width, batch)


def loops(args, dev):
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DConditionModel
    for hw, batch in CONFIGS:
        pipe = AudioDiffusionPipeline(None, UNet2DConditionModel(sample_size=(hw, hw), **BENCH).init_random(0), Mel(x_res=hw, y_res=hw),
                                      DDIMScheduler()).to(dev)
        pipe.set_progress_bar_config(disable=True)
        pipe.scheduler.set_timesteps(STEPS)
        g = torch.Generator().manual_seed(8)
        x = torch.randn(batch, 1, hw, hw, generator=g).to(dev)
        enc = torch.randn(batch, 1, BENCH["cross_attention_dim"], generator=g).to(dev)
        variants = {p: (dict(guidance_scale=3.0) if p == "off" else dict(guidance_scale=3.0, guidance_rescale=float(p))) for p in args.phi}
        times = {k: [] for k in variants}
        # one variant after the other, each behind its own warm-up call: another value is another captured graph on the one handle, and
        # variants alternated call by call would time a capture with every call
        for k, kw in variants.items():
            pipe._denoise(x, 0, 0.0, None, None, 0, 0, encoding=enc, **kw)
            torch.cuda.synchronize(dev)
            for _ in range(RUNS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pipe._denoise(x, 0, 0.0, None, None, 0, 0, encoding=enc, **kw)
                b.record()
                b.synchronize()
                times[k].append(round(a.elapsed_time(b) / STEPS, 4))
        for k, v in times.items():
            print(json.dumps(dict(tag=args.tag, hw=hw, batch=batch, steps=STEPS, guidance_rescale=k, ms_per_step=v)), flush=True)
        del pipe
        torch.cuda.empty_cache()


def kernels(dev):
    from audiodiffusion import ops
    row = dict(sqrt_beta=0.6, sqrt_alpha=0.8, clip=-1.0, k_x0=0.9, k_x=0.0, k_eps=0.4, k_noise=0.0, timestep=500.0)
    table = ops.sched_coef_table([row], dev)
    for hw, batch in CONFIGS:
        g = torch.Generator().manual_seed(8)
        x, c, u = (torch.randn(batch, 1, hw, hw, generator=g).to(dev) for _ in range(3))
        out, scale, resc = torch.empty_like(x), torch.empty(batch, device=dev), torch.empty(batch, device=dev)
        for _ in range(20):
            ops.sched_step(x, c, table, 0, out=out, threshold=(0.995, 4.0), scale_out=scale, uncond=u, guidance_scale=3.0,
                           guidance_rescale=0.7, rescale_out=resc)
        torch.cuda.synchronize(dev)


def bits(dev):
    import hashlib
    from audiodiffusion import ops
    rows = [dict(sqrt_beta=0.62, sqrt_alpha=0.78, clip=1.0, k_x0=0.23, k_x=0.76, k_eps=0.3, k_noise=0.4, timestep=500.0)]
    table = ops.sched_coef_table(rows, dev)
    khist = torch.tensor([-0.31], dtype=torch.float32).to(dev)
    sha = lambda *ts: hashlib.sha256(b"".join(t.detach().cpu().contiguous().numpy().tobytes() for t in ts)).hexdigest()[:16]  # noqa: E731
    for shape in ((3, 2, 8, 12), (2, 1, 64, 64), (1, 1, 256, 256)):
        g = torch.Generator().manual_seed(3)
        x, c, u, nz, h0 = (torch.randn(shape, generator=g).to(dev) for _ in range(5))
        for guided in (0, 1):
            gk = dict(uncond=u, guidance_scale=2.5) if guided else {}
            for pred in (0, 1, 2):
                sel = ops.sched_threshold(x, c, table, 0, 0.9, 4.0, prediction=pred, **gk)
                print(f"bits shape={shape} selection pred={pred} guided={guided} {sha(sel)}", flush=True)
                for mode in ("plain", "thresh"):
                    for stream in (0, 1):
                        scale = torch.zeros(shape[0], device=dev)
                        nk = dict(noise_seed=77, noise_row_offset=5) if stream else dict(noise=nz)
                        out = ops.sched_step(x, c, table, 0, threshold=(0.9, 4.0) if mode == "thresh" else None, scale_out=scale,
                                             prediction=pred, **nk, **gk)
                        print(f"bits shape={shape} step mode={mode} pred={pred} guided={guided} stream={stream} {sha(out, scale)}", flush=True)
            hist = h0.clone()
            out = ops.sched_multistep(x, c, table, khist, hist, 0, noise=nz, **gk)
            print(f"bits shape={shape} step mode=multistep pred=0 guided={guided} stream=0 {sha(out, hist)}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", default=os.path.join(ROOT, "audio-diffusion_amd"))
    ap.add_argument("--tag", default="this")
    ap.add_argument("--phi", nargs="+", default=["0", "0.7"])
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--bits", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    args = ap.parse_args()
    if args.only is not None:
        CONFIGS[:] = [c for c in CONFIGS if c[0] == args.only]
    sys.path[:0] = [args.pkg, ROOT]
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    dev = torch.device("cuda:0")
    bits(dev) if args.bits else kernels(dev) if args.kernels else loops(args, dev)
