"""Time per step of the captured DDIM inversion loop beside the captured DDIM sampling loop of the same model and batch, on the MI355X
(profiles/inversion.md), with the method of tools/device_noise_probe.py.

Two variants, ALTERNATED call by call inside one process, each on a handle of its own over the same weights (a handle holds one captured
step), one warm-up call each (plan, capture):
  s  `_denoise` on the DDIM schedule, eta = 0 (one forward and the fused sampling step per step, no u8 image)
  i  `adm_encode_loop_ex` on the same schedule's "matched" inversion rows (one forward and the inversion step per step)
Two models: bench.py's 256x256 architecture at B = 16 (PROBE_STEPS_256 rows of the 1000-step schedule, default 100) and the same
architecture at 64x64, B = 1 with the single-sample rule (BASELINE config 1's model; PROBE_STEPS_64, default 1000). PROBE_RUNS_256 (3) and
PROBE_RUNS_64 (5) timed calls per variant; the median and the spread are printed. A host clock around the call, ended by a device
synchronise, divided by the number of steps."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "audio-diffusion_amd"), ROOT]
from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel  # noqa: E402
from audiodiffusion import _native as N  # noqa: E402

CFG = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 128, 256, 256, 512, 512),
           down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
           up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
FIELDS = ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise", "timestep")


def measure(name, res, batch, steps, runs, dev, single_sample=False):
    pipe = AudioDiffusionPipeline(None, UNet2DModel(sample_size=res, **CFG).init_random(0), Mel(x_res=res, y_res=res), DDIMScheduler()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    if single_sample:
        pipe.unet.set_option("single_sample", 1)
    pipe.scheduler.set_timesteps(1000)
    steps = min(steps, 1000)
    rows = pipe.scheduler.encode_rows("matched")[:steps]
    coef = (N.SchedCoef * steps)(*[N.SchedCoef(*[float(r[k]) for k in FIELDS]) for r in rows])
    x = torch.randn(batch, 1, res, res, generator=torch.Generator().manual_seed(8)).to(dev)
    img = (0.5 * x).clamp(-1, 1).contiguous()
    inv = UNet2DModel(sample_size=res, **CFG).init_random(0)   # the same weights on a handle of its own: neither loop re-captures
    if single_sample:
        inv.set_option("single_sample", 1)
    h = inv._ensure_handle()

    def call(v):
        if v == "s":
            return pipe._denoise(x, 0, 0.0, None, None, 0, 0, stop_step=None if steps >= 1000 else steps, want_u8=False)[0]
        y = img.clone()
        args = N.SampleLoopArgs(x=N.ptr(y), B=batch, coef_host=coef, n_steps=steps, use_graph=1)
        N.check(N.lib().adm_encode_loop_ex(h, args, N.stream_for(y)))
        return y

    times = {v: [] for v in "si"}
    for v in "si":
        call(v)
    torch.cuda.synchronize(dev)
    for _ in range(runs):
        for v in "si":
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            out = call(v)
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) * 1e3 / steps)
            assert bool(torch.isfinite(out).all())
    rec = dict(model=name, batch=batch, hw=res, steps=steps, runs=runs, captures=N.lib().adm_unet_loop_captures(h),
               ms_per_step={v: round(statistics.median(t), 4) for v, t in times.items()},
               spread_ms_per_step={v: [round(min(t), 4), round(max(t), 4)] for v, t in times.items()})
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    dev = torch.device("cuda:0")
    out = [measure("64x64, B = 1, single-sample rule (BASELINE config 1's model)", 64, 1, int(os.environ.get("PROBE_STEPS_64", "1000")),
                   int(os.environ.get("PROBE_RUNS_64", "5")), dev, True),
           measure("256x256, B = 16", 256, 16, int(os.environ.get("PROBE_STEPS_256", "100")),
                   int(os.environ.get("PROBE_RUNS_256", "3")), dev)]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
