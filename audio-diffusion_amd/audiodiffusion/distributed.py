"""Batch-sharded sampling across the GPUs of one node (BASELINE.json config 3).

Samples never interact (convolutions, GroupNorm statistics, attention and the scheduler are per-sample), so the path
shards by rows with NO collective inside the denoising loop: one process per GPU (`torch.distributed`, backend "nccl" ==
RCCL over xGMI on the MI355X node, "gloo" in CPU tests), identical weights on every rank, the GLOBAL noise batch drawn from
one seed and row-sliced per rank, one `all_gather` of the uint8 images at the end. The result is byte-identical for any
world size. (The reference samples single-process only; this is the new capability the north_star names.)
`device_noise=True` keeps that promise without the global tensors: noise is a function of (seed, GLOBAL row, timestep, element) evaluated
on the device ("adm noise stream 1", include/adm.h), so each rank draws its own rows of the initial latent and its step noise inside the
step kernel, and `global_noise` (O(global batch x noisy steps) host memory on every rank) is never called.
"""
import torch
import torch.distributed as dist


def shard_bounds(global_batch, world, rank):
    per = (global_batch + world - 1) // world
    lo = min(rank * per, global_batch)
    return lo, min(lo + per, global_batch)


def global_noise(shape, seed, steps_with_noise=0):
    """Initial latent (and, for DDPM / eta>0, per-step noise) for the GLOBAL batch from one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    sn = [torch.randn(shape, generator=g) for _ in range(steps_with_noise)]
    return x, sn


def _rows(t, lo, hi, global_batch, name, broadcast=False):
    """Rows [lo:hi] of a GLOBAL per-sample tensor. broadcast: a leading 1 is shared by every row and passed on as it is (the pipeline
    broadcasts a negative encoding, and only that)."""
    if t is None or (broadcast and t.shape[0] == 1):
        return t
    if t.shape[0] != global_batch:
        raise ValueError(f"{name} has {t.shape[0]} rows for a global batch of {global_batch}")
    return t[lo:hi].contiguous()


@torch.no_grad()
def sample_sharded(pipe, global_batch, steps=None, seed=42, eta=0.0, gather=True, group=None, encoding=None, guidance_scale=None,
                   negative_encoding=None, device_noise=False, guidance_rescale=0.0):
    """Returns (images_u8, local_slice): uint8 tensor (global_batch, H, W) on every rank when `gather`, else the
    local shard; `local_slice` = (lo, hi) rows owned by this rank. encoding and negative_encoding are GLOBAL tensors
    (global_batch, seq, dim), row-sliced per rank like the noise (negative_encoding may have a leading 1 instead: broadcast);
    guidance_scale and guidance_rescale as in `AudioDiffusionPipeline.__call__`. The row counts are checked before any rank samples.
    device_noise: `seed` keys the device noise stream (`device_noise_seed=seed`, row offset = this rank's first row) instead of a CPU
    generator: other images than the default path for the same seed, the same bytes for any world size, and no global noise tensor."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    # the keyword rules on every rank, rows or not: all raise, or none (a rank without rows never reaches the loop that checks them)
    from . import ops
    ops.guidance_rescale_on(guidance_rescale, pipe._guided(guidance_scale, negative_encoding, encoding))
    steps = steps or pipe.get_default_steps()
    pipe.scheduler.set_timesteps(steps)
    ss = pipe.unet.sample_size
    H, W = (ss, ss) if isinstance(ss, int) else ss
    lo, hi = shard_bounds(global_batch, world, rank)
    dev = pipe.device
    enc = _rows(encoding, lo, hi, global_batch, "encoding")          # (on every rank, rows or not: all raise, or none)
    neg = _rows(negative_encoding, lo, hi, global_batch, "negative_encoding", broadcast=True)
    if device_noise:
        return _finish(_sample_device_noise(pipe, lo, hi, H, W, seed, eta, enc, guidance_scale, neg, guidance_rescale), lo, hi,
                       global_batch, world, H, W, dev, gather, group)
    rows = pipe.scheduler.coef_rows(eta)
    n_noise = sum(1 for r in rows if r["k_noise"] != 0.0)
    x, sn = global_noise((global_batch, pipe.unet.in_channels, H, W), seed, n_noise)
    step_noise = None
    if n_noise:
        it = iter(sn)
        step_noise = [next(it)[lo:hi].to(dev) if r["k_noise"] != 0.0 else None for r in rows]
    if hi > lo:
        _, u8 = pipe._denoise(x[lo:hi].contiguous().to(dev), 0, eta, None, None, 0, 0, step_noise=step_noise,
                              encoding=enc, guidance_scale=guidance_scale, negative_encoding=neg, guidance_rescale=guidance_rescale)
        u8 = u8.reshape(hi - lo, H, W)
    else:      # more ranks than rows (global_batch < world * per): this rank owns nothing, and still takes part in the gather
        u8 = None
    return _finish(u8, lo, hi, global_batch, world, H, W, dev, gather, group)


def _sample_device_noise(pipe, lo, hi, H, W, seed, eta, enc, guidance_scale, neg, guidance_rescale=0.0):
    """This rank's rows [lo:hi] with every normal drawn on the device: the latent rows from `ops.randn(..., row_offset=lo, noise_stream=1)`,
    the step noise inside the step kernel. -> (hi - lo, H, W) uint8, or None for a rank without rows."""
    if hi <= lo:
        return None
    from . import ops
    x = ops.randn((hi - lo, pipe.unet.in_channels, H, W), seed, row_offset=lo, t=0, noise_stream=1, device=pipe.device)
    _, u8 = pipe._denoise(x, 0, eta, None, None, 0, 0, encoding=enc, guidance_scale=guidance_scale, negative_encoding=neg,
                          device_noise_seed=seed, device_noise_row_offset=lo, guidance_rescale=guidance_rescale)
    return u8.reshape(hi - lo, H, W)


def _finish(u8, lo, hi, global_batch, world, H, W, dev, gather, group):
    """The local shard (None: no rows), or the all_gather of every rank's."""
    if u8 is None:
        u8 = torch.zeros((0, H, W), dtype=torch.uint8, device=dev)
    if not gather or not dist.is_initialized():      # a 1-rank group still goes through the collective (RCCL shake-out)
        return u8, (lo, hi)
    per = (global_batch + world - 1) // world
    pad = torch.zeros((per, H, W), dtype=torch.uint8, device=dev)
    pad[: hi - lo] = u8
    out = torch.empty((world * per, H, W), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(out, pad, group=group)
    return out[:global_batch], (lo, hi)
