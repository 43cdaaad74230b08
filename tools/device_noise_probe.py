"""Time per step and peak device memory of the DDPM sampling loop with host-staged and with device-drawn noise, on the MI355X
(profiles/device_noise.md).

Variants of one `_denoise` call on the 1000-step DDPM schedule, ALTERNATED inside one process, one warm-up call each (plan, capture):
  a  today's staged path, step noise from a CPU generator (drawn on the host, copied into the (<=100, B, C, H, W) staging tensor)
  b  today's staged path, step noise from a device generator (torch.randn on the GPU, copied into the staging tensor)
  c  device_noise_seed: noise drawn inside the fused step kernel, one native call
Two models: bench.py's 256x256 architecture at B = 16 (BASELINE config 2; PROBE_STEPS_256 consecutive steps from t = 999, default 300: three
staging chunks, so the two inter-chunk synchronisations of the staged path are inside the timed window) and the same architecture at
64x64, B = 1 with the single-sample rule (BASELINE config 1's model; PROBE_STEPS_64 steps, default all 1000). PROBE_RUNS_64 (5) and
PROBE_RUNS_256 (2) timed calls per variant; the median and the spread are printed. A host clock around the call,
ended by a device synchronise: the staged path's host work (draws, copies, chunk synchronisations) is part of what it costs.
PROBE_PKG: directory that holds the `audiodiffusion` package to measure (default: this tree's), so that the same script times variants
a and b on another checkout; PROBE_VARIANTS: e.g. "ab" there. Peak memory: torch's allocator peak (the staging tensor lives there) and
the device's used bytes (hipMemGetInfo) after the call."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("PROBE_PKG") or os.path.join(ROOT, "audio-diffusion_amd")
sys.path[:0] = [PKG, ROOT]
from audiodiffusion import AudioDiffusionPipeline, DDPMScheduler, Mel, UNet2DModel  # noqa: E402

VARIANTS = os.environ.get("PROBE_VARIANTS", "abc")
CFG = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 128, 256, 256, 512, 512),
           down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
           up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)


def measure(name, res, batch, steps, runs, dev, single_sample=False):
    pipe = AudioDiffusionPipeline(None, UNet2DModel(sample_size=res, **CFG).init_random(0), Mel(x_res=res, y_res=res), DDPMScheduler()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    if single_sample:
        pipe.unet.set_option("single_sample", 1)
    pipe.scheduler.set_timesteps(1000)
    x = torch.randn(batch, 1, res, res, generator=torch.Generator().manual_seed(8)).to(dev)
    stop = None if steps >= 1000 else steps

    def call(v):
        if v == "c":
            return pipe._denoise(x, 0, 0.0, None, None, 0, 0, stop_step=stop, device_noise_seed=1234)
        gen = torch.Generator().manual_seed(9) if v == "a" else torch.Generator(device=dev).manual_seed(9)
        return pipe._denoise(x, 0, 0.0, gen, None, 0, 0, stop_step=stop)

    times, peak, used = {v: [] for v in VARIANTS}, {}, {}
    for v in VARIANTS:
        call(v)
    torch.cuda.synchronize(dev)
    for _ in range(runs):
        for v in VARIANTS:
            torch.cuda.synchronize(dev)
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            t0 = time.perf_counter()
            out = call(v)
            torch.cuda.synchronize(dev)
            times[v].append((time.perf_counter() - t0) * 1e3 / min(steps, 1000))
            peak[v] = torch.cuda.max_memory_allocated(dev)
            free, total = torch.cuda.mem_get_info(dev)
            used[v] = total - free
            assert bool(torch.isfinite(out[0]).all())
    rec = dict(model=name, pkg=PKG, batch=batch, hw=res, steps=min(steps, 1000), runs=runs,
               ms_per_step={v: round(statistics.median(t), 4) for v, t in times.items()},
               spread_ms_per_step={v: [round(min(t), 4), round(max(t), 4)] for v, t in times.items()},
               torch_peak_MiB={v: round(p / 2 ** 20, 1) for v, p in peak.items()},
               device_used_MiB={v: round(u / 2 ** 20, 1) for v, u in used.items()})
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    dev = torch.device("cuda:0")
    out = [measure("64x64, B = 1, single-sample rule (BASELINE config 1's model)", 64, 1, int(os.environ.get("PROBE_STEPS_64", "1000")),
                   int(os.environ.get("PROBE_RUNS_64", "5")), dev, True),
           measure("256x256, B = 16 (BASELINE config 2)", 256, 16, int(os.environ.get("PROBE_STEPS_256", "300")),
                   int(os.environ.get("PROBE_RUNS_256", "2")), dev)]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
