"""The UniPC step kernel beside the multistep step kernel, and ms per step of a 20-step sampling with either scheduler, on the MI355X
(profiles/unipc.md).

    python tools/unipc_probe.py [--kernels] [--only 64|256]

default:   the unconditional benchmark model (bench.py CFG256: (128, 128, 256, 256, 512, 512)) at 64x64 with B = 1 and at 256x256 with B = 16.
           Per configuration one pipeline (one checkpoint, one handle); per scheduler (DPMSolverMultistepScheduler, UniPCMultistepScheduler,
           and UniPC with v_prediction, thresholding and a zero-SNR schedule) one warm-up `_denoise` call of 20 steps (plan, capture, first
           launches) and then PROBE_RUNS (default 3) timed calls, device events around each call, divided by the steps. One JSON line per
           (configuration, scheduler) with every timed call.
--kernels: instead of the loops, 20 full-row UniPC steps (corrector of order 2, predictor of order 2: every buffer read) and 20 multistep
           steps (k_hist != 0) through `ops` on random buffers, for a kernel trace taken from outside.
--only:    one of the two configurations, by its height (a kernel trace's statistics are per kernel name: one shape per traced process)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, RUNS = 20, int(os.environ.get("PROBE_RUNS", "3"))
BENCH = dict(in_channels=1, out_channels=1, layers_per_block=2, block_out_channels=(128, 128, 256, 256, 512, 512),
             down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
             up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
CONFIGS = [(64, 1), (256, 16)]      # (height = width, batch)


def loops(dev):
    from audiodiffusion import AudioDiffusionPipeline, DPMSolverMultistepScheduler, Mel, UNet2DModel, UniPCMultistepScheduler
    scheds = {"dpmsolver++2M": lambda: DPMSolverMultistepScheduler(), "unipc": lambda: UniPCMultistepScheduler(),
              "unipc-v-zero-snr-thresholded": lambda: UniPCMultistepScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                                                              timestep_spacing="trailing", thresholding=True,
                                                                              sample_max_value=4.0)}
    for hw, batch in CONFIGS:
        pipe = AudioDiffusionPipeline(None, UNet2DModel(sample_size=(hw, hw), **BENCH).init_random(0), Mel(x_res=hw, y_res=hw),
                                      DPMSolverMultistepScheduler()).to(dev)
        pipe.set_progress_bar_config(disable=True)
        x = torch.randn(batch, 1, hw, hw, generator=torch.Generator().manual_seed(8)).to(dev)
        for name, make in scheds.items():
            pipe.scheduler = make()
            pipe.scheduler.set_timesteps(STEPS)
            pipe._denoise(x, 0, 0.0, None, None, 0, 0)
            torch.cuda.synchronize(dev)
            times = []
            for _ in range(RUNS):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pipe._denoise(x, 0, 0.0, None, None, 0, 0)
                b.record()
                b.synchronize()
                times.append(round(a.elapsed_time(b) / STEPS, 4))
            print(json.dumps(dict(hw=hw, batch=batch, steps=STEPS, scheduler=name, ms_per_step=times)), flush=True)
        del pipe
        torch.cuda.empty_cache()


def kernels(dev):
    from audiodiffusion import ops
    row = dict(sqrt_beta=0.6, sqrt_alpha=0.8, clip=-1.0, k_x0=0.9, k_x=0.5, k_eps=0.0, k_noise=0.0, timestep=500.0,
               c_x=0.8, c_m1=0.05, c_m2=-0.01, c_t=0.16, p_m1=-0.24)
    table, utable = ops.sched_coef_table([row, row], dev), ops.sched_unipc_table([row, row], dev)
    khist = torch.tensor([-0.3, -0.3], dtype=torch.float32).to(dev)
    for hw, batch in CONFIGS:
        g = torch.Generator().manual_seed(8)
        x, e, h1 = (torch.randn(batch, 1, hw, hw, generator=g).to(dev) for _ in range(3))
        hist, last, out = torch.randn(2, batch, 1, hw, hw, generator=g).to(dev), x.clone(), torch.empty_like(x)
        for k in range(20):
            ops.sched_unipc(x, e, table, utable, hist, last, k & 1, out=out)
            ops.sched_multistep(x, e, table, khist, h1, k & 1, out=out)
        torch.cuda.synchronize(dev)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", type=int, default=None)
    args = ap.parse_args()
    if args.only is not None:
        CONFIGS[:] = [c for c in CONFIGS if c[0] == args.only]
    sys.path[:0] = [os.path.join(ROOT, "audio-diffusion_amd"), ROOT]
    assert torch.cuda.is_available(), "this probe times the MI355X: no GPU, no number"
    dev = torch.device("cuda:0")
    kernels(dev) if args.kernels else loops(dev)
