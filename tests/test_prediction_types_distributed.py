"""Batch-sharded sampling with a v_prediction DDIM: two gloo ranks on the emulator return the bytes of the single-process run, over
an uneven split (3 rows on 2 ranks). `sample_sharded` goes through the pipeline's `_denoise`, which picks the loop of the scheduler's
prediction type; nothing else is needed (as tests/test_thresholding_distributed.py does for the thresholded loop)."""
import os
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
STEPS = 3
ETA = 0.5      # staged per-step noise as well


def _pipe(prediction_type="v_prediction"):
    for p in (ROOT, os.path.join(ROOT, "audio-diffusion_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from native_backend import select
    select("emu")
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    unet = UNet2DModel(**TINY).init_random(0)
    pipe = AudioDiffusionPipeline(None, unet, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1),
                                  DDIMScheduler(prediction_type=prediction_type))
    pipe.set_progress_bar_config(disable=True)
    return pipe


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      ADM_EMU_THREADS="2")
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from audiodiffusion.distributed import sample_sharded
    out, (lo, hi) = sample_sharded(_pipe(), global_batch=3, steps=STEPS, seed=5, eta=ETA)
    if rank == 0:
        q.put((out.cpu().numpy().copy(), (lo, hi)))  # by value: the producer may exit before the parent reads
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_v_prediction_sampling_matches_single_process():
    from audiodiffusion.distributed import sample_sharded
    single, _ = sample_sharded(_pipe(), global_batch=3, steps=STEPS, seed=5, eta=ETA)
    plain, _ = sample_sharded(_pipe("epsilon"), global_batch=3, steps=STEPS, seed=5, eta=ETA)
    assert not torch.equal(single, plain), "the prediction type changed nothing: the comparison below would show nothing"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 37500 + os.getpid() % 2000      # 37500-39499: above every range the other multi-process tests draw from (29500-37499)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    out, (lo, hi) = q.get(timeout=600)
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    assert (lo, hi) == (0, 2)              # rank 0 owns two rows, rank 1 one: an uneven split
    out = torch.from_numpy(out)
    assert out.shape == single.shape == (3, 16, 16)
    assert torch.equal(out, single.cpu())
