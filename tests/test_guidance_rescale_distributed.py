"""Batch-sharded sampling with rescaled classifier-free guidance: `sample_sharded(..., guidance_rescale=)` on two gloo ranks (the
emulator) returns the bytes of the single-process run, row by row. The factor r_b is a per-sample statistic computed by one workgroup
per sample, so a sample's bytes cannot depend on the shard it falls in; the global batch of 3 is uneven over 2 ranks (2 + 1), as in
tests/test_guidance_distributed.py, whose tiny model and helpers this file uses."""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import test_guidance_distributed as gd

STEPS, BATCH, G, PHI = 3, 3, 3.0, 0.7
CASES = {"ddim": ("ddim", False), "ddpm-device-noise": ("ddpm", True), "dpm": ("dpm", False)}


def _sample(case, phi=PHI):
    from audiodiffusion.distributed import sample_sharded
    kind, device_noise = CASES[case]
    gen = torch.Generator().manual_seed(7)
    enc = torch.randn(BATCH, 1, 12, generator=gen)
    neg = 0.5 * torch.randn(BATCH, 1, 12, generator=gen)
    return sample_sharded(gd._pipe(kind), global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=G, negative_encoding=neg,
                          device_noise=device_noise, guidance_rescale=phi)


def _worker(rank, world, port, case, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), ADM_EMU_THREADS="2")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out, (lo, hi) = _sample(case)
    if rank == 0:
        q.put((out.cpu().numpy().copy(), (lo, hi)))  # by value: the producer may exit before the parent reads
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", list(CASES))
def test_sharded_rescaled_sampling_matches_single_process(case):
    single, _ = _sample(case)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 45500 + os.getpid() % 2000 + 2000 * list(CASES).index(case)      # above the ranges the other multi-process tests draw from
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
    # the rescale is really in, and 0 is the guided run of before
    guided, _ = _sample(case, phi=0.0)
    assert not torch.equal(guided.cpu(), single.cpu())
    from audiodiffusion.distributed import sample_sharded
    kind, device_noise = CASES[case]
    gen = torch.Generator().manual_seed(7)
    enc = torch.randn(BATCH, 1, 12, generator=gen)
    neg = 0.5 * torch.randn(BATCH, 1, 12, generator=gen)
    before, _ = sample_sharded(gd._pipe(kind), global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=G, negative_encoding=neg,
                               device_noise=device_noise)
    assert torch.equal(before.cpu(), guided.cpu())


def test_the_keyword_rules_hold_before_any_rank_samples(monkeypatch):
    """`sample_sharded` checks the keywords itself, on every rank: a rank without rows never reaches the loop that would refuse them."""
    from audiodiffusion.distributed import sample_sharded
    pipe = gd._pipe("ddim")
    monkeypatch.setattr(pipe, "_denoise", lambda *a, **kw: pytest.fail("the loop was reached"))
    enc = torch.randn(BATCH, 1, 12, generator=torch.Generator().manual_seed(7))
    with pytest.raises(ValueError, match="guidance_scale"):
        sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_rescale=PHI)
    with pytest.raises(ValueError, match="guidance_rescale"):
        sample_sharded(pipe, global_batch=BATCH, steps=STEPS, seed=5, encoding=enc, guidance_scale=G, guidance_rescale=1.5)
