"""Batch-sharded sampling with the UniPC scheduler: two gloo ranks on the emulator return the bytes of the single-process run
(`sample_sharded` goes through the pipeline's `_denoise`, unchanged; as tests/test_dpmsolver_distributed.py does for the multistep solver)."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
STEPS = 5      # a start without state, one corrector of order 1, three of order 2, a first-order final predictor


def _pipe():
    for p in (ROOT, os.path.join(ROOT, "audio-diffusion_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from native_backend import select
    select("emu")
    from audiodiffusion import AudioDiffusionPipeline, UniPCMultistepScheduler, Mel, UNet2DModel
    unet = UNet2DModel(**TINY).init_random(0)
    pipe = AudioDiffusionPipeline(None, unet, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1),
                                  UniPCMultistepScheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      ADM_EMU_THREADS="2")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from audiodiffusion.distributed import sample_sharded
    out, (lo, hi) = sample_sharded(_pipe(), global_batch=3, steps=STEPS, seed=5)
    if rank == 0:
        q.put((out.cpu().numpy().copy(), (lo, hi)))  # by value: the producer may exit before the parent reads
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_unipc_sampling_matches_single_process():
    from audiodiffusion.distributed import sample_sharded
    pipe = _pipe()
    single, _ = sample_sharded(pipe, global_batch=3, steps=STEPS, seed=5)
    rows = pipe.scheduler.coef_rows()
    assert sum(r["c_t"] != 0.0 for r in rows) == 4 and sum(r["c_m2"] != 0.0 for r in rows) == 3
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 53500 + os.getpid() % 2000      # 53500-55499: above every range the other multi-process tests draw from (29500-53499)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out, (lo, hi) = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    assert (lo, hi) == (0, 2)
    out = torch.from_numpy(out)
    assert out.shape == single.shape == (3, 16, 16)
    assert torch.equal(out, single.cpu())
