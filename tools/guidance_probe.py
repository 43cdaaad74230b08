"""Time per step of the captured sampling loop with and without classifier-free guidance, on the MI355X (profiles/guidance.md).

Two models: the conditional benchmark model (bench.py CFG_COND: (128, 256, 512, 512), CrossAttn blocks, 64x64 latents; PROBE_B samples,
default 16) and the tiny conditional configuration `COND` of tests/test_dpmsolver.py, which tests/test_guidance.py samples with
(16x16, (32, 64), B = 2). For each: device events around one `_denoise` call of PROBE_STEPS DDIM steps (default 20), one warm-up call per variant (capture included), then PROBE_RUNS (default 21) timed calls per variant with the
variants ALTERNATED, and the median. Printed per step: unguided, guided, twice the unguided time, and the difference of the last two.
The guided step is two forwards and one step kernel that reads one more operand (4 B/elem more than the unguided step kernel)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "audio-diffusion_amd"), ROOT]
from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DConditionModel  # noqa: E402

STEPS, RUNS, B = int(os.environ.get("PROBE_STEPS", "20")), int(os.environ.get("PROBE_RUNS", "21")), int(os.environ.get("PROBE_B", "16"))
BENCH = dict(sample_size=(64, 64), in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 256, 512, 512),
             down_block_types=("CrossAttnDownBlock2D",) * 3 + ("DownBlock2D",), up_block_types=("UpBlock2D",) + ("CrossAttnUpBlock2D",) * 3,
             cross_attention_dim=100, attention_head_dim=8)
TINY = dict(sample_size=(16, 16), in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 64),
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=12, attention_head_dim=4)


def measure(name, cfg, batch, dev):
    hw, dim = cfg["sample_size"][0], cfg["cross_attention_dim"]
    pipe = AudioDiffusionPipeline(None, UNet2DConditionModel(**cfg).init_random(0), Mel(x_res=hw, y_res=hw), DDIMScheduler()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    pipe.scheduler.set_timesteps(STEPS)
    g = torch.Generator().manual_seed(8)
    x = torch.randn(batch, 1, hw, hw, generator=g).to(dev)
    enc = torch.randn(batch, 1, dim, generator=g).to(dev)
    variants = {"unguided": {}, "guided": dict(guidance_scale=3.0)}      # the default null encoding: zeros, kept by the pipeline
    times = {k: [] for k in variants}
    for kw in variants.values():                      # warm-up: plan, capture, first launches
        pipe._denoise(x, 0, 0.0, None, None, 0, 0, encoding=enc, **kw)
    torch.cuda.synchronize(dev)
    for _ in range(RUNS):
        for k, kw in variants.items():                # alternated: both see the same neighbours on a shared machine
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            pipe._denoise(x, 0, 0.0, None, None, 0, 0, encoding=enc, **kw)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / STEPS)
    med = {k: statistics.median(v) for k, v in times.items()}
    rec = dict(model=name, batch=batch, hw=hw, steps=STEPS, runs=RUNS,
               unguided_ms_per_step=round(med["unguided"], 4), guided_ms_per_step=round(med["guided"], 4),
               twice_unguided_ms=round(2 * med["unguided"], 4), guided_minus_twice_unguided_ms=round(med["guided"] - 2 * med["unguided"], 4),
               guided_over_unguided=round(med["guided"] / med["unguided"], 4),
               spread_unguided_ms=[round(min(times["unguided"]), 4), round(max(times["unguided"]), 4)],
               spread_guided_ms=[round(min(times["guided"]), 4), round(max(times["guided"]), 4)],
               step_kernel_extra_bytes=4 * batch * hw * hw)
    print(json.dumps(rec), flush=True)
    return rec


if __name__ == "__main__":
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    dev = torch.device("cuda:0")
    out = [measure("tiny conditional (tests/test_dpmsolver.py COND)", TINY, 2, dev), measure("conditional benchmark model (bench.py CFG_COND)", BENCH, B, dev)]
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
