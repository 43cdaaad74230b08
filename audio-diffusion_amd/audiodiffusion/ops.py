"""Tensor-level wrappers over the op-level C-ABI entry points (parity tests and the scheduler shims use these).

Every function launches hand-written HIP kernels from libadm_hip.so on torch's current stream; none has a
PyTorch/CPU fallback.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N


def _f32(t):
    assert t.dtype == torch.float32 and t.is_contiguous()
    return t


def sched_coef_table(rows, device):
    """rows: list of dicts/tuples with the 8 adm_sched_coef fields -> (n,8) fp32 device tensor."""
    t = torch.tensor([[float(r[k]) for k in ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise", "timestep")]
                      for r in rows], dtype=torch.float32)
    return t.to(device)


def threshold_ranks(n, ratio):
    """(lo, hi, w) of torch.quantile's linear interpolation over n elements, in the float32 arithmetic torch uses:
    rank = float32(ratio) * float32(n - 1), the two neighbouring order statistics and the weight of the upper one."""
    rank = np.float32(ratio) * np.float32(n - 1)
    lo = np.floor(rank)
    return int(lo), int(np.ceil(rank)), float(np.float32(rank - lo))


PREDICTION_TYPES = {"epsilon": 0, "sample": 1, "v_prediction": 2}   # the C-ABI's `prediction`


def _guidance(eps, uncond, guidance_scale):
    """Classifier-free guidance arguments: both given, or neither. -> True when the guided entry points are to run."""
    if (uncond is None) != (guidance_scale is None):
        raise ValueError("classifier-free guidance needs both `uncond` and `guidance_scale` (or neither)")
    if uncond is None:
        return False
    _f32(uncond)
    assert uncond.shape == eps.shape and uncond.device == eps.device
    return True


def guidance_rescale_on(guidance_rescale, guided):
    """The rule of `guidance_rescale` (include/adm.h "guidance rescale"): None or 0 is off; a value in (0, 1] needs active classifier-free
    guidance (`guided`); anything else is refused. -> True when the rescaled form is to run."""
    if guidance_rescale is None:
        return False
    phi = float(guidance_rescale)
    if not 0.0 <= phi <= 1.0:       # (nan fails both comparisons)
        raise ValueError(f"guidance_rescale={guidance_rescale!r} must be in [0, 1]")
    if phi == 0.0:
        return False
    if not guided:
        raise ValueError(f"guidance_rescale={guidance_rescale!r} rescales the guided model output: it needs active classifier-free "
                         f"guidance (the pipeline: guidance_scale > 1, a UNet2DConditionModel and an `encoding`; a step: `guidance_scale` "
                         f"with the unconditional output)")
    return True


def _seed64(seed, name="seed"):
    """A noise-stream seed as the uint64 the C-ABI takes."""
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError(f"{name}={seed!r} must be in [0, 2^64)")
    return seed


def randn(shape, seed, row_offset=0, t=0, noise_stream=0, device=None):
    """(B, C, H, W) normals of "adm noise stream 1" (include/adm.h; csrc/k_sched.hip `randn_fill_kernel`): Philox4x32-10 keyed by `seed`
    on the counter (float4 index inside the sample, row_offset + b, t, noise_stream), two Box-Muller pairs per counter. Exactly what the
    fused step draws for the same counters (noise_stream 0, t = the row's timestep); noise_stream 1 with t = 0 is the initial latent.
    Its own stream: not torch.randn's on any device. C*H*W % 4 == 0."""
    B, Cc, H, W = (int(v) for v in shape)
    device = torch.device(device) if device is not None else N.default_device()
    out = torch.empty((B, Cc, H, W), dtype=torch.float32, device=device)
    N.check(N.lib().adm_randn(N.ptr(out), B, Cc * H * W, _seed64(seed), int(row_offset), int(t), int(noise_stream), N.stream_for(out)))
    return out


def window_count(total_w, W, stride, wrap=False, names=("total_w", "stride", "wrap")):
    """The placement rules of windowed sampling (include/adm.h "Windowed sampling") -> nW, the number of windows per wide sample.
    A broken rule is a ValueError that names the argument it is about, by the caller's name for it (`names`: total_w, stride, wrap)."""
    n_total, n_stride, n_wrap = names
    if not isinstance(wrap, (bool, np.bool_)) and wrap not in (0, 1):
        raise ValueError(f"{n_wrap}={wrap!r} must be a bool")
    total_w, W, stride = int(total_w), int(W), int(stride)
    if W <= 0 or W % 4:
        raise ValueError(f"the model's width {W} must be a positive multiple of 4 for windowed sampling ({n_total})")
    if stride <= 0 or stride % 4 or stride > W:
        raise ValueError(f"{n_stride}={stride} must be a positive multiple of 4 and at most the model's width {W}")
    if total_w % 4 or total_w < W:
        raise ValueError(f"{n_total}={total_w} must be a multiple of 4 and at least the model's width {W}")
    if wrap:
        if total_w % stride:
            raise ValueError(f"{n_total}={total_w} must be a multiple of {n_stride}={stride} with {n_wrap}=True")
        return total_w // stride
    if (total_w - W) % stride:
        raise ValueError(f"{n_total}={total_w} minus the model's width {W} must be a multiple of {n_stride}={stride} with {n_wrap}=False")
    return (total_w - W) // stride + 1


def window_gather(x, W, stride, wrap=False):
    """x (B, C, H, Wt) -> the windows (B*nW, C, H, W), sample-major: windows[b*nW + w, c, y, j] = x[b, c, y, col(w, j)] with
    col = w*stride + j, modulo Wt when `wrap` (include/adm.h "Windowed sampling"; csrc/k_window.hip). A copy, bit-exact."""
    _f32(x)
    B, Cc, H, Wt = x.shape
    nW = window_count(Wt, W, stride, wrap)
    out = torch.empty((B * nW, Cc, H, int(W)), dtype=torch.float32, device=x.device)
    N.check(N.lib().adm_window_gather(N.ptr(x), N.ptr(out), B, Cc, H, Wt, int(W), int(stride), int(bool(wrap)), N.stream_for(x)))
    return out


def window_blend(windows, total_w, stride, wrap=False):
    """windows (B*nW, C, H, W), as `window_gather` lays them out -> (B, C, H, total_w): per column the mean of the windows that cover it,
    summed in ascending window index from the first window's value, one division by the cover count (include/adm.h "Windowed sampling")."""
    _f32(windows)
    BW, Cc, H, W = windows.shape
    nW = window_count(total_w, W, stride, wrap)
    if BW % nW:
        raise ValueError(f"{BW} windows are not a multiple of the {nW} windows per sample of total_w={total_w}, stride={stride}, wrap={wrap}")
    out = torch.empty((BW // nW, Cc, H, int(total_w)), dtype=torch.float32, device=windows.device)
    N.check(N.lib().adm_window_blend(N.ptr(windows), N.ptr(out), BW // nW, Cc, H, int(total_w), W, int(stride), int(bool(wrap)),
                                     N.stream_for(windows)))
    return out


def window_crossfade(windows, total_w, stride, wrap=False, want_u8=False):
    """windows (B*nW, C, H, W), as `window_gather` lays them out -> (B, C, H, total_w): per column the weighted mean of the windows that
    cover it, each window's integer weight falling to 1 towards every edge that has a neighbour; a column one window covers is that
    window's value, copied (include/adm.h "Tiled codec"; csrc/k_window.hip). The join of a tiled codec's windows, where `window_blend`
    is the fusion of model outputs inside a step. want_u8: -> (out, u8), u8 (B, C, H, total_w) the bytes `dequant_u8(out)` gives,
    written by the same kernel."""
    _f32(windows)
    BW, Cc, H, W = windows.shape
    nW = window_count(total_w, W, stride, wrap)
    if BW % nW:
        raise ValueError(f"{BW} windows are not a multiple of the {nW} windows per sample of total_w={total_w}, stride={stride}, wrap={wrap}")
    out = torch.empty((BW // nW, Cc, H, int(total_w)), dtype=torch.float32, device=windows.device)
    u8 = torch.empty(out.shape, dtype=torch.uint8, device=windows.device) if want_u8 else None
    N.check(N.lib().adm_window_crossfade(N.ptr(windows), N.ptr(out), N.ptr(u8), BW // nW, Cc, H, int(total_w), W, int(stride),
                                         int(bool(wrap)), N.stream_for(windows)))
    return (out, u8) if want_u8 else out


def _sched_args(x, eps, coef_table, step, step_dev, prediction, uncond, guidance_scale, out=None, u8_out=None, noise=None, mask=None,
                mask_start=0, mask_end=0, guidance_rescale=None, rescale_out=None):
    """The `adm_sched_step_args` (include/adm.h) of a plain step on x, eps: (B,C,H,W); the callers add their mode's fields.
    -> (the struct, the tensors it points to that the caller did not pass and that must outlive the native call)"""
    _f32(x), _f32(eps)
    B, Cc, H, W = x.shape
    a = N.SchedStepArgs(x=N.ptr(x), eps=N.ptr(eps), noise=N.ptr(noise), out=N.ptr(out), u8_out=N.ptr(u8_out), coef_table=N.ptr(coef_table),
                        step_dev=N.ptr(step_dev), step=int(step), mask=N.ptr(mask), n_mask_steps=mask.shape[1] if mask is not None else 0,
                        mask_start=int(mask_start), mask_end=int(mask_end), B=B, C=Cc, H=H, W=W, prediction=int(prediction))
    guided = _guidance(eps, uncond, guidance_scale)
    if guided:
        a.eps_uncond, a.guidance_scale = N.ptr(uncond), float(guidance_scale)
    keep = None
    if guidance_rescale_on(guidance_rescale, guided):
        keep = torch.empty((B,), dtype=torch.float32, device=x.device) if rescale_out is None else _f32(rescale_out)
        assert keep.shape == (B,) and keep.device == x.device
        a.guidance_rescale, a.rescale = float(guidance_rescale), N.ptr(keep)
    return a, keep


def _set_known(a, known):
    """The known-region fields of `a` (include/adm.h "Region in-painting"). known: None, or (known, known_noise, keep, known_table):
    known (1 or B, C, H, W) fp32, known_noise (B, C, H, W) fp32, keep (1 or B, H, W) uint8, known_table (n, 2) fp32 of (ka, kb) per row of
    the coefficient table. -> the tensors the struct points to (they must outlive the native call)."""
    if known is None:
        return None
    kn, kz, keep, table = known
    _f32(kn), _f32(kz), _f32(table)
    shape = (a.B, a.C, a.H, a.W)
    if keep.dtype != torch.uint8 or not keep.is_contiguous() or tuple(keep.shape[1:]) != shape[2:] or keep.shape[0] not in (1, a.B):
        raise ValueError(f"keep must be a contiguous uint8 tensor (1 or B, H, W) = (1 or {a.B}, {a.H}, {a.W}), not {keep.dtype} {tuple(keep.shape)}")
    if tuple(kn.shape[1:]) != shape[1:] or kn.shape[0] not in (1, a.B):
        raise ValueError(f"known must be (1 or B, C, H, W) = (1 or {a.B}, {a.C}, {a.H}, {a.W}), not {tuple(kn.shape)}")
    if tuple(kz.shape) != shape:
        raise ValueError(f"known_noise must be (B, C, H, W) = {shape}, not {tuple(kz.shape)}")
    if table.dim() != 2 or table.shape[1] != 2:
        raise ValueError(f"known_table must be (n, 2), not {tuple(table.shape)}")
    a.known, a.known_noise, a.keep, a.known_table = N.ptr(kn), N.ptr(kz), N.ptr(keep), N.ptr(table)
    a.known_batched, a.keep_batched = int(kn.shape[0] == a.B and a.B > 1), int(keep.shape[0] == a.B and a.B > 1)
    return known


def _set_threshold(a, ratio, max_value, scale):
    """The selection's fields of `a`: the ranks of `ratio` over one sample, the maximum and the (B,) tensor that receives the thresholds."""
    a.lo, a.hi, a.w = threshold_ranks(a.C * a.H * a.W, ratio)
    a.max_value, a.scale = float(max_value), N.ptr(scale)


def sched_threshold(x, eps, coef_table, step, ratio, max_value, step_dev=None, out=None, prediction=0, uncond=None,
                    guidance_scale=None, guidance_rescale=None, rescale_out=None):
    """Per-sample dynamic threshold s_b = clamp(quantile(|x0_b|, ratio), 1, max_value) of x0 = (x - sqrt_beta*eps) / sqrt_alpha
    (csrc/k_sched.hip `sched_threshold_kernel`: an exact radix select on the device, equal to torch.quantile to the bit). -> (B,) fp32.
    prediction != 0: `eps` is the model output of a sample (1) or v_prediction (2) model and x0 is formed accordingly. uncond,
    guidance_scale: classifier-free guidance, `eps` is the conditional output and x0 is that of
    o = uncond + guidance_scale * (eps - uncond). guidance_rescale, rescale_out: as in sched_step (the statistics kernel runs first). One
    native call (`adm_sched_threshold_ex`)."""
    a, _keep = _sched_args(x, eps, coef_table, step, step_dev, prediction, uncond, guidance_scale, guidance_rescale=guidance_rescale,
                           rescale_out=rescale_out)
    out = torch.empty((a.B,), dtype=torch.float32, device=x.device) if out is None else out
    _set_threshold(a, ratio, max_value, out)
    N.check(N.lib().adm_sched_threshold_ex(a, N.stream_for(x)))
    return out


def sched_step(x, eps, coef_table, step, noise=None, mask=None, mask_start=0, mask_end=0, out=None, u8_out=None, threshold=None,
               step_dev=None, scale_out=None, prediction=0, uncond=None, guidance_scale=None, noise_seed=None, noise_row_offset=0,
               guidance_rescale=None, rescale_out=None, known=None):
    """Fused scheduler epilogue (pipeline_audio_diffusion.py:165-185,192-194), one native call (`adm_sched_step_ex`). x,eps: (B,C,H,W).
    threshold: None, or (dynamic_thresholding_ratio, sample_max_value): x0 is clamped to its per-sample percentile and divided by it
    instead of the static clamp (scale_out: optional (B,) fp32 that receives the thresholds). step_dev: optional int32 device scalar
    that replaces `step`. prediction != 0: `eps` is the model output of a sample (1) or v_prediction (2) model (include/adm.h has the
    table). uncond, guidance_scale: classifier-free guidance, `eps` is the conditional model output and the step uses
    o = uncond + guidance_scale * (eps - uncond), combined inside the kernel. noise_seed (instead of `noise`): a row with k_noise != 0
    draws its noise inside the kernel from "adm noise stream 1" — `randn(x.shape, noise_seed, noise_row_offset, t=the row's timestep)`
    without the tensor; noise_row_offset is the global row of x[0]. guidance_rescale (None or 0: off, the kernels of the unrescaled step):
    phi in (0, 1] rescales the guided output per sample, o' = phi*(o*r_b) + (1 - phi)*o with r_b = std(eps_b) / std(o_b) computed on the
    device first (include/adm.h "guidance rescale"; `guidance_stats_kernel`); needs uncond and guidance_scale. rescale_out: optional (B,)
    fp32 that receives r_b. known: None, or (known, known_noise, keep, known_table): the known-region overwrite (include/adm.h "Region
    in-painting"): where keep (1 or B, H, W) uint8 is non-zero the result is ka*known + kb*known_noise with (ka, kb) = known_table[step],
    `add_noise`'s bits, formed inside the step kernel; excludes `mask`."""
    if noise_seed is not None and noise is not None:
        raise ValueError("`noise_seed` (noise drawn inside the kernel) and `noise=` (a noise tensor) exclude each other")
    out = torch.empty_like(x) if out is None else out
    a, _keep = _sched_args(x, eps, coef_table, step, step_dev, prediction, uncond, guidance_scale, out, u8_out, noise, mask, mask_start,
                           mask_end, guidance_rescale, rescale_out)
    if threshold is not None:
        a.mode = N.SCHED_THRESH   # (`scale` is a local: the struct holds its address only, and it must outlive the call)
        scale = torch.empty((a.B,), dtype=torch.float32, device=x.device) if scale_out is None else scale_out
        _set_threshold(a, threshold[0], threshold[1], scale)
    if noise_seed is not None:
        a.noise_source, a.seed, a.row_offset = 1, _seed64(noise_seed, "noise_seed"), int(noise_row_offset)
    _known = _set_known(a, known)
    N.check(N.lib().adm_sched_step_ex(a, N.stream_for(x)))
    return out


def encode_step(x, model_out, coef_table, step, prediction=0, step_dev=None):
    """One DDIM inversion step on x IN PLACE (csrc/k_sched.hip `encode_step_kernel`; include/adm.h "DDIM inversion" names the fields of a
    row; `DDIMScheduler.encode_rows` builds them), one native call (`adm_encode_step`). x, model_out: the same shape, numel % 4 == 0;
    model_out is the output of an epsilon (0), sample (1) or v_prediction (2) model. step_dev: optional int32 device scalar that
    replaces `step`. -> x"""
    _f32(x), _f32(model_out), _f32(coef_table)
    assert model_out.shape == x.shape and model_out.device == x.device
    assert coef_table.dim() == 2 and coef_table.shape[1] == 8 and (step_dev is not None or 0 <= int(step) < coef_table.shape[0])
    N.check(N.lib().adm_encode_step(N.ptr(x), N.ptr(model_out), N.ptr(coef_table), N.ptr(step_dev), int(step), int(prediction),
                                    x.numel(), N.stream_for(x)))
    return x


def sched_multistep(x, eps, coef_table, k_hist_table, hist, step, noise=None, mask=None, mask_start=0, mask_end=0, out=None,
                    u8_out=None, step_dev=None, uncond=None, guidance_scale=None, guidance_rescale=None, rescale_out=None, known=None):
    """Fused multistep scheduler epilogue (csrc/k_sched.hip `sched_step_kernel<SCHED_MULTISTEP, ...>`). x, eps, hist: (B,C,H,W); k_hist_table: (n,)
    fp32 beside the (n,8) coef_table. hist is read where k_hist_table[step] != 0 and always rewritten with this step's x0. step_dev:
    optional int32 device scalar that replaces `step`. uncond, guidance_scale: classifier-free guidance as in sched_step; hist then
    holds x0 of the guided output. guidance_rescale, rescale_out: as in sched_step; hist then holds x0 of the rescaled output. known: as
    in sched_step; hist is written before the overwrite and never sees it."""
    _f32(hist), _f32(k_hist_table)
    assert hist.shape == x.shape and k_hist_table.numel() == coef_table.shape[0]
    out = torch.empty_like(x) if out is None else out
    a, _keep = _sched_args(x, eps, coef_table, step, step_dev, 0, uncond, guidance_scale, out, u8_out, noise, mask, mask_start, mask_end,
                           guidance_rescale, rescale_out)
    a.mode, a.k_hist_table, a.hist = N.SCHED_MULTISTEP, N.ptr(k_hist_table), N.ptr(hist)
    _known = _set_known(a, known)
    N.check(N.lib().adm_sched_step_ex(a, N.stream_for(x)))
    return out


UNIPC_FIELDS = ("c_x", "c_m1", "c_m2", "c_t", "p_m1")   # include/adm.h: adm_unipc_coef


def sched_unipc_table(rows, device):
    """rows: list of dicts with the 5 adm_unipc_coef fields (beside the 8 of sched_coef_table) -> (n,5) fp32 device tensor."""
    return torch.tensor([[float(r[k]) for k in UNIPC_FIELDS] for r in rows], dtype=torch.float32).to(device)


def sched_unipc(x, eps, coef_table, unipc_table, hist, last, step, noise=None, mask=None, mask_start=0, mask_end=0, out=None,
                u8_out=None, step_dev=None, uncond=None, guidance_scale=None, guidance_rescale=None, rescale_out=None, threshold=None,
                prediction=0, scale_out=None, known=None):
    """Fused UniPC predictor-corrector step (csrc/k_unipc.hip `unipc_step_kernel`; include/adm.h "UniPC"), one native call
    (`adm_sched_step_ex` with `unipc_table`). x, eps, last: (B,C,H,W); hist: (2,B,C,H,W); unipc_table: (n,5) fp32 beside the (n,8)
    coef_table. Row `step` corrects x with the data predictions of this and the two previous rows (where its c_t != 0; `last` is read only
    then), writes the corrected sample to `last` and this row's data prediction to hist[step & 1], and returns the predicted sample of
    the next level. threshold, prediction, uncond, guidance_scale, guidance_rescale, rescale_out, scale_out, step_dev, mask: as in
    sched_step; the history then holds x0 of the guided / rescaled / thresholded output. `noise` exists for the keyword set of
    sched_multistep and must be None: the step has no noise rows (the native call refuses it by name). known: as in sched_step; `last` and
    hist are written before the overwrite and never see it."""
    _f32(hist), _f32(last), _f32(unipc_table)
    assert tuple(hist.shape) == (2,) + tuple(x.shape) and last.shape == x.shape and unipc_table.shape == (coef_table.shape[0], 5)
    out = torch.empty_like(x) if out is None else out
    a, _keep = _sched_args(x, eps, coef_table, step, step_dev, prediction, uncond, guidance_scale, out, u8_out, noise, mask, mask_start,
                           mask_end, guidance_rescale, rescale_out)
    a.unipc_table, a.hist, a.last = N.ptr(unipc_table), N.ptr(hist), N.ptr(last)
    if threshold is not None:
        a.mode = N.SCHED_THRESH
        scale = torch.empty((a.B,), dtype=torch.float32, device=x.device) if scale_out is None else scale_out
        _set_threshold(a, threshold[0], threshold[1], scale)
    _known = _set_known(a, known)
    N.check(N.lib().adm_sched_step_ex(a, N.stream_for(x)))
    return out


def add_noise(x0, noise, sa, sb, per_sample):
    """scheduler.add_noise. per_sample=True: x0,noise (B,...) with sa,sb (B,) -> (B,...).
    per_sample=False (mask build, pipeline:157): x0 (1,H,W) broadcast, noise (B,1,H,W), sa,sb (n,) -> (B,n,H,W)."""
    _f32(x0), _f32(noise), _f32(sa), _f32(sb)
    B = noise.shape[0]
    P = noise[0].numel()
    if per_sample:
        out = torch.empty_like(noise)
        N.check(N.lib().adm_add_noise(N.ptr(x0), P, N.ptr(noise), N.ptr(sa), N.ptr(sb), 1, 0, N.ptr(out), B, 1, P,
                                      N.stream_for(noise)))
    else:
        n = sa.numel()
        out = torch.empty((B, n) + tuple(noise.shape[2:]), dtype=torch.float32, device=noise.device)
        N.check(N.lib().adm_add_noise(N.ptr(x0), 0, N.ptr(noise), N.ptr(sa), N.ptr(sb), 0, 1, N.ptr(out), B, n, P,
                                      N.stream_for(noise)))
    return out


def noise_and_velocity(x0, noise, sa, sb):
    """Training prologue of a v_prediction model, one kernel: x0, noise (B,...) with sa, sb (B,) ->
    (noisy = sa*x0 + sb*noise, bit-identical to add_noise(per_sample=True); velocity = sa*noise - sb*x0)."""
    _f32(x0), _f32(noise), _f32(sa), _f32(sb)
    assert x0.shape == noise.shape and sa.numel() == noise.shape[0] == sb.numel()
    noisy, velocity = torch.empty_like(noise), torch.empty_like(noise)
    N.check(N.lib().adm_noise_and_velocity(N.ptr(x0), N.ptr(noise), N.ptr(sa), N.ptr(sb), N.ptr(noisy), N.ptr(velocity),
                                           noise.shape[0], noise[0].numel(), N.stream_for(noise)))
    return noisy, velocity


def dequant_u8(x):
    """(x/2+0.5).clamp(0,1)*255 -> round-half-even -> uint8, same shape (pipeline_audio_diffusion.py:192-194)."""
    _f32(x)
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    N.check(N.lib().adm_dequant_u8(N.ptr(x), N.ptr(out), x.numel(), N.stream_for(x)))
    return out


def slerp_grid(x0, x1, alphas):
    """AudioDiffusionPipeline.slerp for every alpha in one launch pair: (len(alphas),) + x0.shape."""
    _f32(x0), _f32(x1)
    assert x0.shape == x1.shape
    al = torch.as_tensor([float(a) for a in alphas], dtype=torch.float64).to(x0.device)
    out = torch.empty((al.numel(),) + tuple(x0.shape), dtype=torch.float32, device=x0.device)
    scratch = torch.zeros(3, dtype=torch.float64, device=x0.device)
    N.check(N.lib().adm_slerp_grid(N.ptr(x0.contiguous()), N.ptr(x1.contiguous()), x0.numel(), N.ptr(al), al.numel(), N.ptr(out),
                                   N.ptr(scratch), N.stream_for(x0)))
    return out


def groupnorm_stats(x1, gamma, beta, groups, eps, x2=None):
    """Returns per-(n,c) (scale, shift) of GroupNorm over the virtual concat (x1|x2)."""
    _f32(x1)
    Nn, C1 = x1.shape[:2]
    C2 = x2.shape[1] if x2 is not None else 0
    HW = x1[0, 0].numel()
    scale = torch.empty((Nn, C1 + C2), dtype=torch.float32, device=x1.device)
    shift = torch.empty_like(scale)
    N.check(N.lib().adm_groupnorm_stats(N.ptr(x1), C1, N.ptr(x2), C2, Nn, HW, groups, float(eps), N.ptr(gamma),
                                        N.ptr(beta), N.ptr(scale), N.ptr(shift), N.stream_for(x1)))
    return scale, shift


def pack_conv_weight(w):
    """(Cout,Cin,ks,ks) -> [Cin][ks*ks][Cout]."""
    _f32(w)
    co, ci, ks, _ = w.shape
    wp = torch.empty((ci, ks * ks, co), dtype=torch.float32, device=w.device)
    N.check(N.lib().adm_pack_conv_weight(N.ptr(w), N.ptr(wp), co, ci, ks, N.stream_for(w)))
    return wp


def pack_conv_weight_T(w):
    """(Cout,Cin,ks,ks) -> backward-data packing [Cout][ks*ks][Cin] (transposed + flipped)."""
    _f32(w)
    co, ci, ks, _ = w.shape
    wp = torch.empty((co, ks * ks, ci), dtype=torch.float32, device=w.device)
    N.check(N.lib().adm_pack_conv_weight_T(N.ptr(w), N.ptr(wp), co, ci, ks, N.stream_for(w)))
    return wp


def pack_winograd_weight(w):
    """(Cout,Cin,3,3) -> Winograd-domain U = G g G^T as [Cin][16][Cout]."""
    _f32(w)
    co, ci = w.shape[:2]
    # the buffer holds the F(2x2,3x3) image and, where conv_wino6_kernel may run, the F(4x4,3x3) image behind it (adm.h)
    wu = torch.empty((int(N.lib().adm_winograd_packed_floats(co, ci, 0)),), dtype=torch.float32, device=w.device)
    N.check(N.lib().adm_pack_winograd_weight(N.ptr(w), N.ptr(wu), co, ci, N.stream_for(w)))
    return wu


def pack_winograd_weight_T(w):
    """(Cout,Cin,3,3) -> Winograd-domain filters of the data-gradient convolution as [Cout][16][Cin]."""
    _f32(w)
    co, ci = w.shape[:2]
    wu = torch.empty((int(N.lib().adm_winograd_packed_floats(co, ci, 1)),), dtype=torch.float32, device=w.device)
    N.check(N.lib().adm_pack_winograd_weight_T(N.ptr(w), N.ptr(wu), co, ci, N.stream_for(w)))
    return wu


def pack_bf16_weight(w, transposed=False):
    """(Cout,Cin,3,3) fp32 -> bf16 MFMA operand layout [tap][Cin/8][Cout][8] (transposed: the data-gradient filters)."""
    _f32(w)
    co, ci = w.shape[:2]
    ks = w.shape[2] if w.dim() == 4 else 1
    shape = (ks * ks, co // 8, ci, 8) if transposed else (ks * ks, ci // 8, co, 8)
    wb = torch.empty(shape, dtype=torch.bfloat16, device=w.device)
    N.check(N.lib().adm_pack_bf16_weight_ks(N.ptr(w), C.c_void_p(wb.data_ptr()), co, ci, ks, int(transposed), N.stream_for(w)))
    return wb


def conv2d(x1, wpacked, bias, ks, x2=None, up=False, stride=1, pad_lo=1, gn=None, act=False, chan_add=None,
           residual=None, wino=None, bf16=None, stats=False):
    """Fused convolution (see include/adm.h adm_conv_args). stats=True: also returns the GroupNorm partial sums of the output
    the kernel's epilogue wrote, (N, Cout, tiles, 2) fp64 — None when the dispatched kernel has no such epilogue."""
    _f32(x1)
    Nn, C1, H, W = x1.shape
    Cout = wpacked.shape[2]
    Ho, Wo = C.c_int(), C.c_int()
    N.lib().adm_conv_out_dims(H, W, int(up), stride, ks, pad_lo, C.byref(Ho), C.byref(Wo))
    out = torch.empty((Nn, Cout, Ho.value, Wo.value), dtype=torch.float32, device=x1.device)
    a = N.ConvArgs()
    a.x1, a.C1 = N.ptr(x1), C1
    a.x2, a.C2 = (N.ptr(x2), x2.shape[1]) if x2 is not None else (None, 0)
    a.N, a.H, a.W = Nn, H, W
    a.up, a.stride, a.ks, a.pad_lo = int(up), stride, ks, pad_lo  # up: 0 none, 1/True nearest x2, 2 zero-insertion x2
    if gn is not None:
        a.gn_scale, a.gn_shift = N.ptr(gn[0]), N.ptr(gn[1])
    a.act = int(act)
    a.wpacked, a.bias, a.Cout = N.ptr(wpacked), N.ptr(bias), Cout
    if chan_add is not None:
        assert chan_add.dtype == torch.float32 and chan_add.stride(1) == 1
        a.chan_add, a.chan_add_stride = C.c_void_p(chan_add.data_ptr()), chan_add.stride(0)
    a.residual = N.ptr(residual)
    a.wino_packed = N.ptr(wino)
    a.bf16_packed = C.c_void_p(bf16.data_ptr()) if bf16 is not None else None
    a.out = N.ptr(out)
    st = None
    if stats:
        tiles = N.lib().adm_conv_stats_tiles(C.byref(a))
        if tiles > 0:
            st = torch.full((Nn, Cout, tiles, 2), float("nan"), dtype=torch.float64, device=x1.device)
            a.stats_out, a.stats_tiles = N.ptr(st), tiles
    N.check(N.lib().adm_conv2d(C.byref(a), N.stream_for(x1)))
    return (out, st) if stats else out


def groupnorm_finalize(st1, gamma, beta, groups, eps, hw, st2=None):
    """GroupNorm (scale, shift) from the per-tile partial sums convolutions wrote (conv2d(..., stats=True)); st2: the second
    part of a virtual channel concat."""
    Nn, C1, t1 = st1.shape[:3]
    C2, t2 = (st2.shape[1], st2.shape[2]) if st2 is not None else (0, 0)
    scale = torch.empty((Nn, C1 + C2), dtype=torch.float32, device=st1.device)
    shift = torch.empty_like(scale)
    N.check(N.lib().adm_groupnorm_finalize(N.ptr(st1), C1, t1, N.ptr(st2), C2, t2, Nn, hw, groups, float(eps), N.ptr(gamma),
                                           N.ptr(beta), N.ptr(scale), N.ptr(shift), N.stream_for(st1)))
    return scale, shift


def attention(qkv, head_dim):
    """qkv (N,3C,H,W) -> (N,C,H,W)."""
    _f32(qkv)
    Nn, C3, H, W = qkv.shape
    out = torch.empty((Nn, C3 // 3, H, W), dtype=torch.float32, device=qkv.device)
    N.check(N.lib().adm_attention(N.ptr(qkv), N.ptr(out), Nn, C3 // 3, H * W, head_dim, N.stream_for(qkv)))
    return out


# ---------------------------------------------------------------------------------------------- Transformer2DModel pieces
def layernorm_nct(x, gamma, beta, eps=1e-5):
    """LayerNorm over the channel axis of (N,C,H,W) for every token (BasicTransformerBlock.norm1/2/3)."""
    _f32(x)
    Nn, Cc = x.shape[:2]
    y = torch.empty_like(x)
    N.check(N.lib().adm_layernorm_nct(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(y), Nn, Cc, x[0, 0].numel(), eps,
                                      N.stream_for(x)))
    return y


def geglu(x):
    """(N,2*C4,H,W) = [h | gate] -> (N,C4,H,W) = h * gelu(gate)."""
    _f32(x)
    Nn, C2 = x.shape[:2]
    out = torch.empty((Nn, C2 // 2) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    N.check(N.lib().adm_geglu(N.ptr(x), N.ptr(out), Nn, C2 // 2, x[0, 0].numel(), N.stream_for(x)))
    return out


def cross_attention(q, ctx, wk, wv, head_dim):
    """q (N,C,H,W), ctx (N,S,Dc), to_k/to_v weights (C,Dc) -> (N,C,H,W)."""
    _f32(q), _f32(ctx)
    Nn, Cc = q.shape[:2]
    out = torch.empty_like(q)
    N.check(N.lib().adm_cross_attention(N.ptr(q), N.ptr(ctx), N.ptr(wk), N.ptr(wv), N.ptr(out), Nn, Cc, q[0, 0].numel(),
                                        ctx.shape[1], ctx.shape[2], head_dim, N.stream_for(q)))
    return out


def layernorm_nct_backward(x, dy, gamma, eps=1e-5):
    """-> (dx, dgamma, dbeta) of layernorm_nct."""
    _f32(x), _f32(dy)
    Nn, Cc = x.shape[:2]
    T = x[0, 0].numel()
    dx = torch.empty_like(x)
    stats = torch.empty(2 * Nn * T, dtype=torch.float32, device=x.device)
    dg, db = torch.zeros_like(gamma), torch.zeros_like(gamma)
    N.check(N.lib().adm_layernorm_nct_backward(N.ptr(x), N.ptr(dy), N.ptr(gamma), N.ptr(dx), 0, N.ptr(stats), N.ptr(dg),
                                               N.ptr(db), Nn, Cc, T, eps, N.stream_for(x)))
    return dx, dg, db


def geglu_backward(x, dy):
    _f32(x), _f32(dy)
    Nn, C2 = x.shape[:2]
    dx = torch.empty_like(x)
    N.check(N.lib().adm_geglu_backward(N.ptr(x), N.ptr(dy), N.ptr(dx), Nn, C2 // 2, x[0, 0].numel(), N.stream_for(x)))
    return dx


def cross_attention_backward(q, ctx, wk, wv, dy, head_dim):
    """-> (dq, dWk, dWv) of cross_attention."""
    _f32(q), _f32(dy)
    Nn, Cc = q.shape[:2]
    dq = torch.empty_like(q)
    dwk, dwv = torch.zeros_like(wk), torch.zeros_like(wv)
    N.check(N.lib().adm_cross_attention_backward(N.ptr(q), N.ptr(ctx), N.ptr(wk), N.ptr(wv), N.ptr(dy), N.ptr(dq), N.ptr(dwk),
                                                 N.ptr(dwv), Nn, Cc, q[0, 0].numel(), ctx.shape[1], ctx.shape[2], head_dim,
                                                 N.stream_for(q)))
    return dq, dwk, dwv


def attention_backward_blocked(qkv, dout, head_dim, block=0):
    _f32(qkv), _f32(dout)
    Nn, C3, H, W = qkv.shape
    dqkv = torch.empty_like(qkv)
    stats = torch.empty(3 * Nn * (C3 // 3 // head_dim) * H * W, dtype=torch.float32, device=qkv.device)
    N.check(N.lib().adm_attention_backward_blocked(N.ptr(qkv), N.ptr(dout), N.ptr(dqkv), N.ptr(stats), Nn, C3 // 3, H * W,
                                                   head_dim, block, N.stream_for(qkv)))
    return dqkv


def attention_blocked(qkv, head_dim, key_block=0):
    """adm_attention with keys processed in blocks (online softmax): qkv (N,3C,H,W) -> (N,C,H,W)."""
    _f32(qkv)
    Nn, C3, H, W = qkv.shape
    out = torch.empty((Nn, C3 // 3, H, W), dtype=torch.float32, device=qkv.device)
    N.check(N.lib().adm_attention_blocked(N.ptr(qkv), N.ptr(out), Nn, C3 // 3, H * W, head_dim, key_block, N.stream_for(qkv)))
    return out


# ---------------------------------------------------------------------------------------------- backward ops (training)
def _conv_args(x1, wpacked, bias, ks, x2, up, stride, pad_lo, gn, act, Cout):
    Nn, C1, H, W = x1.shape
    a = N.ConvArgs()
    a.x1, a.C1 = N.ptr(x1), C1
    a.x2, a.C2 = (N.ptr(x2), x2.shape[1]) if x2 is not None else (None, 0)
    a.N, a.H, a.W = Nn, H, W
    a.up, a.stride, a.ks, a.pad_lo = int(up), stride, ks, pad_lo
    if gn is not None:
        a.gn_scale, a.gn_shift = N.ptr(gn[0]), N.ptr(gn[1])
    a.act = int(act)
    a.wpacked, a.bias, a.Cout = N.ptr(wpacked), N.ptr(bias), Cout
    return a


def sumpool2x2(x, out=None, accumulate=False):
    """(N,C,2H,2W) -> (N,C,H,W) sum over 2x2 blocks: backward of the folded nearest-x2 upsample."""
    _f32(x)
    Nn, Cc, H, W = x.shape
    out = torch.empty((Nn, Cc, H // 2, W // 2), dtype=torch.float32, device=x.device) if out is None else out
    N.check(N.lib().adm_sumpool2x2(N.ptr(x), N.ptr(out), H, W, Nn * Cc, int(accumulate), N.stream_for(x)))
    return out


def groupnorm_stats_ex(x1, gamma, beta, groups, eps, x2=None):
    """Like groupnorm_stats but also returns (N, groups, 2) [mean, rstd] for the backward pass."""
    Nn, C1 = x1.shape[:2]
    C2 = x2.shape[1] if x2 is not None else 0
    HW = x1[0, 0].numel()
    scale = torch.empty((Nn, C1 + C2), dtype=torch.float32, device=x1.device)
    shift = torch.empty_like(scale)
    mr = torch.empty((Nn, groups, 2), dtype=torch.float32, device=x1.device)
    N.check(N.lib().adm_groupnorm_stats_ex(N.ptr(x1), C1, N.ptr(x2), C2, Nn, HW, groups, float(eps), N.ptr(gamma),
                                           N.ptr(beta), N.ptr(scale), N.ptr(shift), N.ptr(mr), N.stream_for(x1)))
    return scale, shift, mr


def groupnorm_backward(x1, da, mean_rstd, gamma, beta, groups, act, x2=None):
    """Backward of a = act(GroupNorm(cat(x1,x2))): returns (dx1, dx2 or None, dgamma, dbeta)."""
    Nn, C1 = x1.shape[:2]
    C2 = x2.shape[1] if x2 is not None else 0
    HW = x1[0, 0].numel()
    dev = x1.device
    dg, db = torch.zeros(C1 + C2, device=dev), torch.zeros(C1 + C2, device=dev)
    s12 = torch.empty((Nn, groups, 2), dtype=torch.float32, device=dev)
    dx1 = torch.empty_like(x1)
    dx2 = torch.empty_like(x2) if x2 is not None else None
    N.check(N.lib().adm_groupnorm_backward(N.ptr(x1), C1, N.ptr(x2), C2, N.ptr(da.contiguous()), Nn, HW, groups,
                                           N.ptr(mean_rstd), N.ptr(gamma), N.ptr(beta), int(act), N.ptr(s12), N.ptr(dg),
                                           N.ptr(db), N.ptr(dx1), 0, N.ptr(dx2), 0, N.stream_for(x1)))
    return dx1, dx2, dg, db


def _batch_view(t, bstride):
    """Address and batch stride of a source given as a slice of a wider (N, C + extra, H, W) buffer: every sample contiguous, samples `bstride`
    floats apart (adm_conv_args.x1_bstride / x2_bstride)."""
    assert t.stride(0) == bstride and t[0].is_contiguous() and bstride >= t[0].numel(), "a batch-strided source: contiguous samples, stride(0) = bstride"
    assert t.is_cuda == N.is_device_build()
    return C.c_void_p(t.data_ptr())


def conv2d_wgrad(x1, dy, Cout, ks, x2=None, up=False, stride=1, pad_lo=1, gn=None, act=False, accumulate=False, out=None,
                 x1_bstride=None, x2_bstride=None):
    """dW (Cout,Cin,ks,ks) of the fused conv, with the load-path activation recomputed.
    out: the caller's dW (a contiguous view of Cout*Cin*ks*ks floats at any float offset of a gradient buffer) instead of a fresh tensor;
    accumulate: dW += instead of dW =; x1_bstride / x2_bstride: x1 / x2 are channel slices of wider buffers (samples that many floats apart)."""
    _f32(x1 if x1_bstride is None else x1[:1]), _f32(dy)
    Ct = x1.shape[1] + (x2.shape[1] if x2 is not None else 0)
    a = _conv_args(x1 if x1_bstride is None else x1[:1], dy, None, ks, None if x2_bstride is not None else x2, up, stride, pad_lo, gn, act,
                   Cout)  # wpacked unused by wgrad
    a.N = x1.shape[0]
    if x1_bstride is not None:
        a.x1, a.x1_bstride = _batch_view(x1, x1_bstride), x1_bstride
    if x2_bstride is not None:
        a.x2, a.C2, a.x2_bstride = _batch_view(x2, x2_bstride), x2.shape[1], x2_bstride
    ws_n = N.lib().adm_conv_wgrad_workspace(C.byref(a))
    ws = torch.empty(ws_n, dtype=torch.float32, device=x1.device)
    if out is None:
        dW = torch.zeros((Cout, Ct, ks, ks), dtype=torch.float32, device=x1.device)
    else:
        _f32(out)
        assert out.numel() == Cout * Ct * ks * ks and out.device == x1.device
        dW = out
    N.check(N.lib().adm_conv2d_wgrad(C.byref(a), N.ptr(dy), N.ptr(dW), int(accumulate), N.ptr(ws), N.stream_for(x1)))
    return dW


def last_wgrad_variant():
    """(kernel, reduce, split, tiles_per_block) of the last conv2d_wgrad on this thread (include/adm.h: adm_last_wgrad_variant)."""
    v = N.WgradVariant()
    N.lib().adm_last_wgrad_variant(C.byref(v))
    return v.kernel, v.reduce, v.split, v.tiles_per_block


def wgrad_reduce(workspace, split, numel, dW, accumulate=False, taps=1):
    """dW (=|+=) the sum of the `split` slabs of `numel` floats in `workspace` ([tap][cout*cin] order -> (cout, cin, tap)): adm_wgrad_reduce."""
    _f32(workspace), _f32(dW)
    assert workspace.numel() >= split * numel and dW.numel() == numel
    N.check(N.lib().adm_wgrad_reduce(N.ptr(workspace), split, numel, N.ptr(dW), int(accumulate), taps, N.stream_for(dW)))
    return dW


def blocked_image(x1, x2=None, gn=None, act=False, sums=False, zero_insert=False):
    """Blocked 16-bit operand image [n][C/8][H+2][W+2][8] (zero halo) of act(gn(concat(x1, x2))) — include/adm.h
    adm_blocked_apply.  Returns a (N, C/8, H+2, W+2, 8) bf16 tensor (binary16 bits under option conv_op16_f16);
    sums=True: also the per-(n, c) and per-c sums of the fp32 input."""
    _f32(x1)
    Nn, C1, H, W = x1.shape
    C2 = x2.shape[1] if x2 is not None else 0
    zi = 2 if zero_insert else 1        # zero_insert 1 / 2: the (2H, 2W) image with x(y, x) on pixel (2y + 1, 2x + 1) / (2y, 2x) (stride-2 backward)
    img = torch.zeros((Nn, (C1 + C2) // 8, zi * H + 2, zi * W + 2, 8), dtype=torch.bfloat16, device=x1.device)
    assert img.numel() * 2 == N.lib().adm_blocked_image_bytes(Nn, C1 + C2, zi * H, zi * W)
    nc = torch.zeros((Nn, C1 + C2), dtype=torch.float32, device=x1.device) if sums else None
    c = torch.zeros(C1 + C2, dtype=torch.float32, device=x1.device) if sums else None
    scr = torch.empty(N.lib().adm_blocked_sums_scratch(Nn, C1 + C2, H, W), dtype=torch.float32, device=x1.device) if sums else None
    N.check(N.lib().adm_blocked_apply(N.ptr(x1), C1, N.ptr(x2), C2, Nn, H, W, N.ptr(gn[0]) if gn is not None else None,
                                      N.ptr(gn[1]) if gn is not None else None, int(act), int(zero_insert), C.c_void_p(img.data_ptr()), N.ptr(scr),
                                      N.ptr(nc), C1 + C2, N.ptr(c), N.stream_for(x1)))
    return (img, nc, c) if sums else img


def conv2d_bf16_blocked(img, wb, Cout, bias=None, chan_add=None, residual=None, up=False, stats=False):
    """3x3 stride-1 convolution of a blocked image on 16-bit MFMA operands (adm_conv2d_bf16_blocked); wb from pack_bf16_weight
    (transposed=True with the image of dy: the data gradient); up: nearest x2 of the image folded in (Upsample2D.conv)."""
    Nn, Cg, Hp, Wp, _ = img.shape
    up = int(up)                        # 0 stride 1, 1 nearest x2 of the image folded in, 2 / 3 stride-2 output (pad (0,1,0,1) / padding 1)
    H, W = (Hp - 2) * (2 if up == 1 else 1), (Wp - 2) * (2 if up == 1 else 1)
    out = torch.empty((Nn, Cout, H // 2, W // 2) if up >= 2 else (Nn, Cout, H, W), dtype=torch.float32, device=img.device)
    ca, cas = (None, 0)
    if chan_add is not None:
        assert chan_add.dtype == torch.float32 and chan_add.stride(1) == 1
        ca, cas = C.c_void_p(chan_add.data_ptr()), chan_add.stride(0)
    st = torch.zeros((Nn, Cout, (H // 8) * (W // 32), 2), dtype=torch.float64, device=img.device) if stats else None
    assert not (stats and up >= 2)
    N.check(N.lib().adm_conv2d_bf16_blocked(C.c_void_p(img.data_ptr()), Cg * 8, Nn, H, W, C.c_void_p(wb.data_ptr()), Cout,
                                            N.ptr(bias), ca, cas, N.ptr(residual), N.ptr(out), int(up), N.ptr(st), N.stream_for(out)))
    return (out, st) if stats else out


def conv2d_wgrad_bf16_blocked(x_img, dy_img, up=False):
    """dW (Cout, Cin, 3, 3) from the blocked images of the activated input and of dy (adm_conv2d_wgrad_bf16_blocked);
    up: x_img is the half-resolution input of an Upsample2D convolution."""
    Nn, CgI = x_img.shape[:2]
    CgO, Hp, Wp = dy_img.shape[1:4]
    H, W, Cin, Cout = Hp - 2, Wp - 2, CgI * 8, CgO * 8
    ws_n = N.lib().adm_conv_wgrad_blocked_workspace(Cin, Cout, Nn, H, W)
    assert ws_n > 0, "shape not eligible"
    ws = torch.empty(ws_n, dtype=torch.float32, device=x_img.device)
    dW = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float32, device=x_img.device)
    N.check(N.lib().adm_conv2d_wgrad_bf16_blocked(C.c_void_p(x_img.data_ptr()), Cin, C.c_void_p(dy_img.data_ptr()), Cout, Nn, H, W,
                                                  N.ptr(dW), 0, N.ptr(ws), int(up), N.stream_for(dW)))
    return dW


def chan_sums(dy):
    """(N,C,H,W) -> (per-(n,c) sums (N,C), per-c sums (C,))."""
    _f32(dy)
    Nn, Cc = dy.shape[:2]
    nc = torch.empty((Nn, Cc), dtype=torch.float32, device=dy.device)
    c = torch.zeros(Cc, dtype=torch.float32, device=dy.device)
    N.check(N.lib().adm_chan_sums(N.ptr(dy), Nn, Cc, dy[0, 0].numel(), N.ptr(nc), Cc, 0, N.ptr(c), N.stream_for(dy)))
    return nc, c


def attention_backward(qkv, dout, head_dim):
    _f32(qkv), _f32(dout)
    Nn, C3, H, W = qkv.shape
    dqkv = torch.empty_like(qkv)
    N.check(N.lib().adm_attention_backward(N.ptr(qkv), N.ptr(dout), N.ptr(dqkv), Nn, C3 // 3, H * W, head_dim,
                                           N.stream_for(qkv)))
    return dqkv


def linear_backward(dY, X, W, x_silu=False):
    """Y = b + W @ f(X) with f = silu if x_silu: returns (dW, db, dX)."""
    B, J = dY.shape
    K = X.shape[1]
    dW, db = torch.zeros((J, K), device=dY.device), torch.zeros(J, device=dY.device)
    dX = torch.empty((B, K), device=dY.device)
    N.check(N.lib().adm_linear_backward(N.ptr(dY.contiguous()), J, N.ptr(X), N.ptr(W), B, J, K, int(x_silu), N.ptr(dW),
                                        N.ptr(db), N.ptr(dX), N.stream_for(dY)))
    return dW, db, dX


def conv_small_cin_wgrad(x, dy, out=None):
    """out: the caller's dW (Cout*Cin*9 floats); the kernel ADDS to what it holds."""
    Nn, Ci, H, W = x.shape
    Co = dy.shape[1]
    dW = torch.zeros((Co, Ci, 3, 3), device=x.device) if out is None else out
    assert dW.numel() == Co * Ci * 9
    N.check(N.lib().adm_conv_small_cin_wgrad(N.ptr(x), Ci, Nn, H, W, N.ptr(dy), Co, N.ptr(dW), N.stream_for(x)))
    return dW


def conv_small_cout_backward(x, w, dy, gn=None, act=False, out=None, want=(True, True)):
    """conv_out class (Cout <= 4): returns (da, dW) with da the gradient w.r.t. the activated input.
    out = (da, dW): the caller's destinations (either None: a fresh one); da is written, dW is ADDED to. want = (da?, dW?): False passes NULL."""
    Nn, Ci, H, W = x.shape
    Co = dy.shape[1]
    da, dW = out if out is not None else (None, None)
    if want[0] and da is None:
        da = torch.empty_like(x)
    if want[1] and dW is None:
        dW = torch.zeros((Co, Ci, 3, 3), device=x.device)
    da, dW = (da if want[0] else None), (dW if want[1] else None)
    assert da is None or da.numel() == x.numel()
    assert dW is None or dW.numel() == Co * Ci * 9
    N.check(N.lib().adm_conv_small_cout_backward(N.ptr(x), Ci, Nn, H, W, N.ptr(gn[0]) if gn else None,
                                                 N.ptr(gn[1]) if gn else None, int(act), N.ptr(w), N.ptr(dy), Co,
                                                 N.ptr(da), N.ptr(dW), N.stream_for(x)))
    return da, dW


# ---------------------------------------------------------------------------------------------- timestep embedding (test aids)
def time_embedding(t, freqs, w1, b1, w2, b2, flip=True, save=False):
    """t (B,), freqs (dim_in / 2,), linear_1 (dim_emb, dim_in), linear_2 (dim_emb, dim_emb) -> (emb, emb_act) (B, dim_emb) each, emb_act = silu(emb);
    save=True: also (sinusoid (B, dim_in), z (B, dim_emb)), the input and the pre-activation output of linear_1."""
    for a in (t, freqs, w1, b1, w2, b2):
        _f32(a)
    B, half = t.numel(), freqs.numel()
    dim_emb, dim_in = w1.shape
    assert dim_in == 2 * half and tuple(w2.shape) == (dim_emb, dim_emb)
    emb = torch.empty((B, dim_emb), dtype=torch.float32, device=t.device)
    emb_act = torch.empty_like(emb)
    sinus = torch.empty((B, dim_in), dtype=torch.float32, device=t.device) if save else None
    z = torch.empty_like(emb) if save else None
    N.check(N.lib().adm_time_embedding(N.ptr(t), N.ptr(freqs), half, int(flip), N.ptr(w1), N.ptr(b1), N.ptr(w2), N.ptr(b2), dim_in, dim_emb,
                                       N.ptr(emb), B, N.ptr(sinus), N.ptr(z), N.ptr(emb_act), N.stream_for(t)))
    return (emb, emb_act, sinus, z) if save else (emb, emb_act)


def temb_proj(emb, w, bias, activated=False):
    """(B, K) x stacked time_emb_proj weights (R, K) -> bias + silu(emb) W^T (B, R); activated=True: emb already holds silu(emb)."""
    _f32(emb), _f32(w), _f32(bias)
    B, K = emb.shape
    R = w.shape[0]
    out = torch.empty((B, R), dtype=torch.float32, device=emb.device)
    N.check(N.lib().adm_temb_proj(N.ptr(emb), N.ptr(w), N.ptr(bias), N.ptr(out), B, K, R, int(activated), N.stream_for(emb)))
    return out
