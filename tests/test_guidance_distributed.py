"""Batch-sharded sampling of a conditional model, with and without classifier-free guidance: two gloo ranks on the emulator return the
bytes of the single-process run. `sample_sharded` row-slices the global encoding and negative encoding like the noise (as
tests/test_dpmsolver_distributed.py does for the multistep scheduler). The global batch of 3 is uneven over 2 ranks."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=12, attention_head_dim=4)
STEPS, BATCH = 3, 3
CASES = {"ddim-guided": ("ddim", 3.0, True), "ddpm-guided-zeros": ("ddpm", 3.0, False), "dpm-guided": ("dpm", 1.5, True),
         "ddim-unguided": ("ddim", None, False)}


def _pipe(kind):
    for p in (ROOT, os.path.join(ROOT, "audio-diffusion_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from native_backend import select
    select("emu")
    from audiodiffusion import (AudioDiffusionPipeline, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, Mel,
                                UNet2DConditionModel)
    unet = UNet2DConditionModel(**COND).init_random(0)
    sched = {"ddim": DDIMScheduler, "ddpm": DDPMScheduler, "dpm": DPMSolverMultistepScheduler}[kind]()
    pipe = AudioDiffusionPipeline(None, unet, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1), sched)
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _sample(case):
    from audiodiffusion.distributed import sample_sharded
    kind, g, negative = CASES[case]
    gen = torch.Generator().manual_seed(7)
    enc = torch.randn(BATCH, 1, 12, generator=gen)
    neg = 0.5 * torch.randn(BATCH, 1, 12, generator=gen) if negative else None
    return sample_sharded(_pipe(kind), global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=g, negative_encoding=neg)


def test_global_encoding_needs_one_row_per_sample():
    """A leading-1 `encoding` would fit a rank that owns one row and not its neighbour: refused; only the negative encoding broadcasts."""
    from audiodiffusion.distributed import sample_sharded
    pipe = _pipe("ddim")
    gen = torch.Generator().manual_seed(7)
    enc, one = torch.randn(BATCH, 1, 12, generator=gen), torch.randn(1, 1, 12, generator=gen)
    with pytest.raises(ValueError, match="encoding has 1 rows"):
        sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=one)
    with pytest.raises(ValueError, match="negative_encoding has 2 rows"):
        sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=3.0, negative_encoding=enc[:2])
    a, _ = sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=3.0, negative_encoding=one)
    b, _ = sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=3.0,
                          negative_encoding=one.expand(BATCH, 1, 12).contiguous())
    assert torch.equal(a, b)


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      ADM_EMU_THREADS="2")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out, (lo, hi) = _sample(case)
    if rank == 0:
        q.put((out.cpu().numpy().copy(), (lo, hi)))  # by value: the producer may exit before the parent reads
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", list(CASES))
def test_sharded_conditional_sampling_matches_single_process(case):
    single, _ = _sample(case)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000 + 2000 * list(CASES).index(case) % 8000      # above the ranges the other multi-process tests draw from
    procs = [ctx.Process(target=_worker, args=(r, 2, port, case, q)) for r in range(2)]
    for p in procs:
        p.start()
    out, (lo, hi) = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    assert (lo, hi) == (0, 2)               # 3 rows over 2 ranks: 2 + 1
    out = torch.from_numpy(out)
    assert out.shape == single.shape == (BATCH, 16, 16)
    assert torch.equal(out, single.cpu())
    if CASES[case][1] is not None:          # guidance is really in
        from audiodiffusion.distributed import sample_sharded
        gen = torch.Generator().manual_seed(7)
        enc = torch.randn(BATCH, 1, 12, generator=gen)
        plain, _ = sample_sharded(_pipe(CASES[case][0]), global_batch=BATCH, steps=STEPS, seed=5, encoding=enc)
        assert not torch.equal(plain.cpu(), single.cpu())
