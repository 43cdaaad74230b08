"""Batch-sharded sampling with device noise: two gloo ranks on the emulator return the bytes of the single-process run without ever
building the global noise tensors (`sample_sharded(device_noise=True)`; in the style of tests/test_dpmsolver_distributed.py)."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
STEPS, GLOBAL, SEED = 6, 5, 5      # five rows over two ranks: shards of 3 and 2


def _pipe():
    for p in (ROOT, os.path.join(ROOT, "audio-diffusion_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from native_backend import select
    select("emu")
    from audiodiffusion import AudioDiffusionPipeline, DDPMScheduler, Mel, UNet2DModel
    unet = UNet2DModel(**TINY).init_random(0)
    pipe = AudioDiffusionPipeline(None, unet, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1), DDPMScheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _forbid_global_noise():
    from audiodiffusion import distributed

    def refuse(*a, **k):
        raise AssertionError("global_noise was called on the device-noise path")
    distributed.global_noise = refuse


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      ADM_EMU_THREADS="2")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pipe = _pipe()
    _forbid_global_noise()
    from audiodiffusion.distributed import sample_sharded
    out, (lo, hi) = sample_sharded(pipe, global_batch=GLOBAL, steps=STEPS, seed=SEED, device_noise=True)
    q.put((rank, out.cpu().numpy().copy(), (lo, hi)))  # by value: the producer may exit before the parent reads
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_device_noise_sampling_matches_single_process_without_global_noise(monkeypatch):
    from audiodiffusion import distributed
    from audiodiffusion.distributed import sample_sharded
    pipe = _pipe()
    calls = []
    real = distributed.global_noise
    monkeypatch.setattr(distributed, "global_noise", lambda *a, **k: calls.append(a) or real(*a, **k))
    host, _ = sample_sharded(pipe, global_batch=GLOBAL, steps=STEPS, seed=SEED)
    assert len(calls) == 1, "the default path draws the global noise from the CPU generator, as before"

    def refuse(*a, **k):
        raise AssertionError("global_noise was called on the device-noise path")
    monkeypatch.setattr(distributed, "global_noise", refuse)
    with pytest.raises(AssertionError):
        sample_sharded(pipe, global_batch=GLOBAL, steps=STEPS, seed=SEED)
    single, _ = sample_sharded(pipe, global_batch=GLOBAL, steps=STEPS, seed=SEED, device_noise=True)
    assert single.shape == host.shape == (GLOBAL, 16, 16) and not torch.equal(single, host)      # its own stream, not torch's
    assert sum(r["k_noise"] != 0.0 for r in pipe.scheduler.coef_rows()) == STEPS - 1
    other, _ = sample_sharded(pipe, global_batch=GLOBAL, steps=STEPS, seed=SEED + 1, device_noise=True)
    assert not torch.equal(other, single)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 35500 + os.getpid() % 2000      # 35500-37499: above every range the other multi-process tests draw from (29500-35499)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict((r, (o, s)) for r, o, s in (q.get(timeout=600) for _ in range(2)))
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    assert got[0][1] == (0, 3) and got[1][1] == (3, 5)
    for r in (0, 1):
        out = torch.from_numpy(got[r][0])
        assert out.shape == single.shape and torch.equal(out, single.cpu())
