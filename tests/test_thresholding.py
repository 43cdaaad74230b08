"""Dynamic thresholding (Imagen §2.3; diffusers' `thresholding`) in DDIMScheduler / DDPMScheduler: the selection kernel
(`adm_sched_threshold`), the thresholded step (`adm_sched_step_thresholded`), the captured loop (`adm_sample_loop_thresholded`) inside
the pipeline, and the plumbing — on the emulator and, under `-m gpu`, on the MI355X.

A. The selection to the bit: with sqrt_alpha = 1 and eps = 0 (x0 == x) the scales equal clamp(torch.quantile(|x|), 1, max) on the CPU.
B. The thresholded step against the same formula in float64, bar of tests/test_dpmsolver.py (`_judge`):
   max|d| / max|ref| <= 8 * max(e_torch_fp32, 4 * 2^-24); the quantile is 1-Lipschitz in the max norm, so the rule carries over.
C. Anchors that do not rest on the recalled formula: sample_max_value = 1 is bit-identical to the static clamp to 1; thresholding off
   is bit-identical to `adm_sched_step` / `adm_sample_loop` called directly.
D. A sample's bits (step and scale) do not depend on its batch.
E. The pipeline against the oracle pipeline driven by a subclass of the oracle schedulers that thresholds with torch.quantile:
   max|d| <= 1e-3 on the final floats, images within 1 LSB; the loop against the eager steps and graph on against graph off, bit for bit.
F. Plumbing: save / load, a hand-written config, bad values, the multistep scheduler still refuses, the ABI version, no spills.
(Two gloo ranks: tests/test_thresholding_distributed.py.)
"""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest
import torch

import sched_kernels
from native_backend import BACKENDS, select
from oracle import mel as omel
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle.unet import UNet2DModel as OracleUNet

U = 2.0 ** -24
TINY = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 64),
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
MEL = dict(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=2, sample_rate=4000)
HUGE = 1e38       # a sample_max_value that never binds: the clamp must not hide the selection


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _f32(v):
    return float(np.float32(v))


def _g(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _judge(tag, what, got, ref64, ref32):
    got = got.detach().cpu()
    assert got.shape == ref64.shape == ref32.shape
    assert bool(torch.isfinite(got).all()), (tag, what, "kernel output is not finite")
    e_kernel, e_torch = _g(got, ref64), _g(ref32, ref64)
    bound = 8 * max(e_torch, 4 * U)
    print(f"THRESH {tag} out={what} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} bound={bound:.3e}")
    assert e_kernel <= bound, (tag, what, e_kernel, e_torch, bound)


# ================================================================ A. the selection, to the bit
IDENT = [dict(sqrt_beta=_f32(0.37), sqrt_alpha=1.0, clip=-1.0, k_x0=1.0, k_x=0.0, k_eps=0.0, k_noise=0.0, timestep=0.0)]
SEL_SHAPES = [(1, 1, 4, 4), (2, 1, 16, 16), (3, 2, 8, 12), (1, 3, 40, 52), (2, 1, 256, 256)]
RATIOS = [0.0, 0.5, 0.995, 0.999, 1.0]
KINDS = ["gauss", "ties", "equal", "zeros", "logu", "scales"]


def _sel_input(kind, shape):
    B = shape[0]
    g = torch.Generator().manual_seed(100 + len(kind) + shape[2])
    x = 3.0 * torch.randn(shape, generator=g)
    if kind == "ties":                  # multiples of 0.25: both ranks fall inside one large run of equal values
        x = torch.round(x * 4) / 4
    elif kind == "equal":               # the last sample all equal (signs mixed)
        x[B - 1] = 1.75
        x[B - 1].view(-1)[::3] = -1.75
    elif kind == "zeros":               # the last sample all zero, -0.0 among them: q = 0, s = 1
        x[B - 1] = 0.0
        x[B - 1].view(-1)[::2] = -0.0
    elif kind == "logu":                # magnitudes log-uniform over 1e-30 .. 1e30: the quantile crosses exponent boundaries
        mag = torch.pow(10.0, 60.0 * torch.rand(shape, generator=g, dtype=torch.float64) - 30.0).float()
        x = torch.where(x < 0, -mag, mag)
    elif kind == "scales":              # samples 1e3 apart: leakage between samples would show at once
        for b in range(B):
            x[b] *= 1e3 ** b
    return x.contiguous()


def _cpu_scale(x, ratio, max_value):
    return torch.quantile(x.abs().flatten(1), float(ratio), dim=1).clamp(min=1.0, max=max_value)


def _kernel_scale(dev, x, ratio, max_value, eps=None, rows=IDENT, step=0):
    from audiodiffusion import ops
    table = ops.sched_coef_table(rows, dev)
    e = torch.zeros_like(x) if eps is None else eps
    return ops.sched_threshold(x.to(dev), e.to(dev), table, step, ratio, max_value).cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("backend", BACKENDS)
def test_selection_equals_torch_quantile_to_the_bit(backend, shape, kind):
    dev = select(backend)
    x = _sel_input(kind, shape)
    for ratio in RATIOS:
        want = _cpu_scale(x, ratio, HUGE)
        got = _kernel_scale(dev, x, ratio, HUGE)
        print(f"THRESH backend={backend} shape={shape} kind={kind} ratio={ratio} scale={got.tolist()} torch={want.tolist()}")
        assert got.dtype == torch.float32 and got.shape == (shape[0],)
        assert torch.equal(got, want), (kind, shape, ratio, got.tolist(), want.tolist())
    if kind == "zeros":
        assert float(want[-1]) == 1.0
    if kind == "scales" and shape[0] > 1:
        assert float(want[1]) > 100 * float(want[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_selection_lands_on_both_ends_of_the_clamp(backend):
    dev = select(backend)
    shape = (2, 1, 16, 16)
    small, big = 0.1 * _randn(shape, 1), 3.0 * _randn(shape, 2)
    s_small, s_big = _kernel_scale(dev, small, 0.995, 1.5), _kernel_scale(dev, big, 0.995, 1.5)
    assert torch.equal(s_small, _cpu_scale(small, 0.995, 1.5)) and s_small.tolist() == [1.0, 1.0]      # q < 1: s == 1
    assert torch.equal(s_big, _cpu_scale(big, 0.995, 1.5)) and s_big.tolist() == [1.5, 1.5]            # q > max: s == max
    free = _kernel_scale(dev, big, 0.995, HUGE)
    assert bool((free > 1.5).all())


@pytest.mark.parametrize("backend", BACKENDS)
def test_selection_reads_x0_and_not_x(backend):
    """eps != 0 and sqrt_alpha != 1: the statistic is over the x0 the step kernel computes (within the fp32 rounding of x0)."""
    dev = select(backend)
    shape = (2, 1, 16, 16)
    x, e = _randn(shape, 3), _randn(shape, 4)
    row = dict(sqrt_beta=_f32(0.91), sqrt_alpha=_f32(0.41), clip=-1.0, k_x0=1.0, k_x=0.0, k_eps=0.0, k_noise=0.0, timestep=0.0)
    got = _kernel_scale(dev, x, 0.9, HUGE, eps=e, rows=[row])
    x0 = (x.double() - row["sqrt_beta"] * e.double()) / row["sqrt_alpha"]
    want = torch.quantile(x0.abs().flatten(1), 0.9, dim=1).clamp(min=1.0)
    assert float(((got.double() - want).abs() / want).max()) <= 8 * U


# ================================================================ B. the thresholded step against float64
ROWS = [dict(sqrt_beta=_f32(0.91), sqrt_alpha=_f32(0.41), clip=-1.0, k_x0=_f32(0.62), k_x=0.0, k_eps=_f32(0.71),     # DDIM, eta > 0
             k_noise=_f32(0.33), timestep=900.0),
        dict(sqrt_beta=_f32(0.62), sqrt_alpha=_f32(0.78), clip=-1.0, k_x0=_f32(0.23), k_x=_f32(0.76), k_eps=0.0,     # DDPM
             k_noise=_f32(0.12), timestep=500.0),
        dict(sqrt_beta=_f32(0.35), sqrt_alpha=_f32(0.94), clip=0.5, k_x0=_f32(0.44), k_x=_f32(0.52), k_eps=0.0,      # clip set: ignored
             k_noise=0.0, timestep=100.0)]
STEP_SHAPES = SEL_SHAPES[:4]
# regime: (input scale, sample_max_value). x0 of rows 0..2 has a standard deviation of about 3.3 / 1.6 / 1.1 times the input scale.
BETWEEN, AT_MAX, AT_ONE = (1.0, 1e3), (1.0, 1.25), (0.05, 2.0)
PLAIN = dict(alias=False, u8=False, dev=False, mask=False, row=0, regime=BETWEEN, ratio=0.995)
FULL = dict(alias=True, u8=True, dev=True, mask=False, row=1, regime=BETWEEN, ratio=0.9)
DDPM_MAX = dict(alias=False, u8=True, dev=False, mask=False, row=1, regime=AT_MAX, ratio=0.995)
DDIM_ONE = dict(alias=True, u8=False, dev=True, mask=False, row=0, regime=AT_ONE, ratio=0.995)
CLIP_IGNORED = dict(alias=False, u8=True, dev=False, mask=False, row=2, regime=BETWEEN, ratio=0.995)
MASK = dict(alias=True, u8=True, dev=True, mask=True, row=0, regime=BETWEEN, ratio=0.5)
MASK_MAX = dict(alias=False, u8=False, dev=False, mask=True, row=2, regime=AT_MAX, ratio=0.995)
KCASES, _CASELIST = [], []
for _s in STEP_SHAPES:
    for _name, _v in (("plain", PLAIN), ("full", FULL), ("ddpm-max", DDPM_MAX), ("ddim-one", DDIM_ONE), ("clip-ignored", CLIP_IGNORED)) + \
            ((("mask", MASK), ("mask-max", MASK_MAX)) if _s[1] == 1 else ()):
        KCASES.append(pytest.param(_s, _v, id="x".join(map(str, _s)) + "-" + _name))
        _CASELIST.append((_s, _v))


def _step_inputs(shape, v):
    scale = v["regime"][0]
    x, e, nz = scale * _randn(shape, 1), scale * _randn(shape, 2), _randn(shape, 4)
    mask = _randn((shape[0], len(ROWS), shape[2], shape[3]), 5) if v["mask"] else None
    return x, e, nz, mask


def _formula(x, e, nz, c, ratio, max_value, dtype):
    """The thresholded step in `dtype`; c: the eight fp32 coefficients of the row (exact in either dtype). -> (prev, s)."""
    x, e, nz = x.to(dtype), e.to(dtype), nz.to(dtype)
    x0 = (x - c["sqrt_beta"] * e) / c["sqrt_alpha"]
    s = torch.quantile(x0.abs().flatten(1), float(ratio), dim=1).clamp(min=1.0, max=max_value)
    sv = s.view(-1, 1, 1, 1)
    x0 = torch.clamp(x0, -sv, sv) / sv
    prev = c["k_x0"] * x0 + c["k_x"] * x + c["k_eps"] * e
    if c["k_noise"] != 0:
        prev = prev + c["k_noise"] * nz
    return prev, s


def _run_step(dev, shape, v, x, e, nz, mask, rows=ROWS, threshold="case"):
    from audiodiffusion import ops
    table = ops.sched_coef_table(rows, dev)
    xd = x.clone().to(dev)
    B, Cc, H, W = shape
    u8 = torch.zeros((B, H * W * Cc), dtype=torch.uint8, device=dev) if v["u8"] else None
    step_dev = torch.tensor([v["row"]], dtype=torch.int32).to(dev) if v["dev"] else None
    scale = torch.zeros((B,), dtype=torch.float32, device=dev)
    th = (v["ratio"], v["regime"][1]) if threshold == "case" else threshold
    out = ops.sched_step(xd, e.to(dev), table, -1 if v["dev"] else v["row"], noise=nz.to(dev),
                         mask=None if mask is None else mask.to(dev), mask_start=3 if v["mask"] else 0,
                         mask_end=5 if v["mask"] else 0, out=xd if v["alias"] else None, u8_out=u8, threshold=th,
                         step_dev=step_dev, scale_out=scale)
    if not v["alias"]:
        assert torch.equal(xd.cpu(), x), "x was written although out does not alias it"
    return out.cpu(), scale.cpu(), None if u8 is None else u8.cpu()


def _regime(s, max_value):
    return ["one" if v == 1.0 else ("max" if v == max_value else "between") for v in s.tolist()]


def test_step_cases_cover_all_three_regimes():
    """From the float64 reference's own s_b: s == 1, 1 < s < max and s == max each occur over the case list of B."""
    seen = set()
    for shape, v in _CASELIST:
        x, e, nz, _ = _step_inputs(shape, v)
        _, s = _formula(x, e, nz, ROWS[v["row"]], v["ratio"], v["regime"][1], torch.float64)
        seen.update(_regime(s, v["regime"][1]))
    assert seen == {"one", "between", "max"}, seen


@pytest.mark.parametrize("shape,v", KCASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_thresholded_step_against_float64(backend, shape, v):
    dev = select(backend)
    B, Cc, H, W = shape
    x, e, nz, mask = _step_inputs(shape, v)
    c, max_value = ROWS[v["row"]], v["regime"][1]
    (ref64, s64), (ref32, s32) = (_formula(x, e, nz, c, v["ratio"], max_value, dt) for dt in (torch.float64, torch.float32))
    if mask is not None:
        for r_ in (ref64, ref32):
            r_[..., :3] = mask[:, v["row"], None, :, :3].to(r_.dtype)
            r_[..., W - 5:] = mask[:, v["row"], None, :, W - 5:].to(r_.dtype)
    out, scale, u8 = _run_step(dev, shape, v, x, e, nz, mask)
    tag = f"backend={backend} shape={shape} variant={v} s64={s64.tolist()}"
    _judge(tag, "out", out, ref64, ref32)
    _judge(tag, "scale", scale, s64, s32)
    assert _regime(scale, max_value) == _regime(s64, max_value), (scale.tolist(), s64.tolist())
    if mask is not None:
        assert torch.equal(out[..., :3], mask[:, v["row"], None, :, :3]) and torch.equal(out[..., W - 5:], mask[:, v["row"], None, :, W - 5:])
    if u8 is not None:
        want = ((out / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).reshape(B, -1)
        assert torch.equal(u8, want), "u8 is not the half-to-even quantisation of the kernel's own float output"
    out2, scale2, u82 = _run_step(dev, shape, v, x, e, nz, mask)
    assert torch.equal(out, out2) and torch.equal(scale, scale2) and (u8 is None or torch.equal(u8, u82))


# ================================================================ C. anchors that do not rest on the recalled formula
@pytest.mark.parametrize("shape,v", [KCASES[8], KCASES[12], KCASES[13], KCASES[16], KCASES[19]])
@pytest.mark.parametrize("backend", BACKENDS)
def test_step_with_max_value_one_is_the_static_clamp_to_one(backend, shape, v):
    dev = select(backend)
    x, e, nz, mask = _step_inputs(shape, dict(v, regime=BETWEEN))
    clip_rows = [dict(r, clip=1.0) for r in ROWS]
    th_out, scale, th_u8 = _run_step(dev, shape, v, x, e, nz, mask, threshold=(v["ratio"], 1.0))
    cl_out, _, cl_u8 = _run_step(dev, shape, v, x, e, nz, mask, rows=clip_rows, threshold=None)
    assert scale.tolist() == [1.0] * shape[0]
    assert torch.equal(th_out, cl_out) and (th_u8 is None or torch.equal(th_u8, cl_u8))
    un_out, _, _ = _run_step(dev, shape, v, x, e, nz, mask, rows=[dict(r, clip=-1.0) for r in ROWS], threshold=None)
    assert not torch.equal(un_out, cl_out), "the clamp never bound: the comparison shows nothing"


def _raw_step(dev, sched, eps, t, x, eta, noise):
    """`adm_sched_step` called directly with the scheduler's own table."""
    from audiodiffusion import _native as N
    i = sched._index_of(t)
    table = sched.coef_table(dev, eta)
    out = torch.empty_like(x)
    B, Cc, H, W = x.shape
    N.check(N.lib().adm_sched_step(N.ptr(x), N.ptr(eps), N.ptr(noise), N.ptr(out), None, N.ptr(table), None, i, None, 0, 0, 0,
                                   B, Cc, H, W, N.stream_for(x)))
    return out


@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_step_with_thresholding_off_is_adm_sched_step(backend, kind):
    dev = select(backend)
    from audiodiffusion import DDIMScheduler, DDPMScheduler
    s = DDIMScheduler(thresholding=False, sample_max_value=3.0) if kind == "ddim" else DDPMScheduler(thresholding=False)
    s.set_timesteps(5)
    assert s.threshold() is None
    x, eps, nz = (2.0 * _randn((2, 1, 16, 16), 1)).to(dev), _randn((2, 1, 16, 16), 2).to(dev), _randn((2, 1, 16, 16), 3).to(dev)
    for t in s.timesteps[:3]:
        if kind == "ddim":
            got = s.step(eps, t, x, eta=0.5, variance_noise=nz).prev_sample
            want = _raw_step(dev, s, eps, t, x, 0.5, nz)
        else:
            got = s.step(eps, t, x, variance_noise=nz).prev_sample
            want = _raw_step(dev, s, eps, t, x, 0.0, nz)
        assert torch.equal(got, want)


# ================================================================ D. batch independence
@pytest.mark.parametrize("backend", BACKENDS)
def test_bits_of_a_sample_do_not_depend_on_its_batch(backend):
    dev = select(backend)
    shape = (3, 2, 8, 12)
    x, e, nz, _ = _step_inputs(shape, FULL)
    for b in range(3):
        x[b] *= 10.0 ** b            # neighbours of very different scale
    out3, s3, u83 = _run_step(dev, shape, FULL, x, e, nz, None)
    out1, s1, u81 = _run_step(dev, (1,) + shape[1:], FULL, x[1:2].contiguous(), e[1:2].contiguous(), nz[1:2].contiguous(), None)
    assert torch.equal(out3[1:2], out1) and torch.equal(s3[1:2], s1) and torch.equal(u83[1:2], u81)
    assert len(set(s3.tolist())) == 3


# ================================================================ E. the pipeline against the oracle pipeline
class _RefThreshold:
    """diffusers' `_threshold_sample` with the real torch.quantile; `seen` collects s of every (step, sample)."""

    def _threshold(self, x0):
        c = self.config
        s = torch.quantile(x0.abs().flatten(1), float(c.dynamic_thresholding_ratio), dim=1)
        s = s.clamp(min=1.0, max=float(c.sample_max_value))
        self.seen.append(s.clone())
        s = s.view(-1, 1, 1, 1)
        return torch.clamp(x0, -s, s) / s


class RefDDIM(_RefThreshold, osched.DDIMScheduler):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.seen = []

    def step(self, model_output, timestep, sample, eta=0.0, generator=None, variance_noise=None):
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        b_t = 1 - a_t
        x0 = self._threshold((sample - b_t ** (0.5) * model_output) / a_t ** (0.5))
        variance = ((1 - a_prev) / b_t) * (1 - a_t / a_prev)
        std = eta * variance ** (0.5)
        prev = a_prev ** (0.5) * x0 + (1 - a_prev - std ** 2) ** (0.5) * model_output       # the raw eps in the direction term
        if eta > 0:
            prev = prev + std * variance_noise
        return {"prev_sample": prev, "pred_original_sample": x0}


class RefDDPM(_RefThreshold, osched.DDPMScheduler):
    def __init__(self, **kw):
        super().__init__(**kw)
        self.seen = []

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None):
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t, cur_a = 1 - a_t, a_t / a_prev
        cur_b = 1 - cur_a
        x0 = self._threshold((sample - b_t ** (0.5) * model_output) / a_t ** (0.5))
        prev = (a_prev ** (0.5) * cur_b) / b_t * x0 + cur_a ** (0.5) * (1 - a_prev) / b_t * sample
        if t > 0:
            var = torch.clamp((1 - a_prev) / (1 - a_t) * cur_b, min=1e-20)
            prev = prev + (var ** 0.5) * variance_noise
        return {"prev_sample": prev, "pred_original_sample": x0}


TH = dict(thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=4.0)


def _build(kind="ddim", cfg=TH, unet_cfg=TINY, cond=False):
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, DDPMScheduler, Mel, UNet2DConditionModel, UNet2DModel
    torch.manual_seed(0)
    if cond:
        from oracle.unet_condition import UNet2DConditionModel as OracleCond
        ref_unet = OracleCond(**unet_cfg).eval()
        unet = UNet2DConditionModel(**unet_cfg).load_state_dict(ref_unet.state_dict())
    else:
        ref_unet = OracleUNet(**unet_cfg).eval()
        unet = UNet2DModel(**unet_cfg).load_state_dict(ref_unet.state_dict())
    ref = opipe.AudioDiffusionPipeline(None, ref_unet, omel.Mel(**MEL), (RefDDIM if kind == "ddim" else RefDDPM)(**cfg))
    mine = AudioDiffusionPipeline(None, unet, Mel(**MEL), (DDIMScheduler if kind == "ddim" else DDPMScheduler)(**cfg))
    mine.set_progress_bar_config(disable=True)
    return ref, mine


def _cmp(mi, mf, ri, rf, scale=1.0):
    err = float((mf.cpu() - rf).abs().max())
    a = np.stack([np.asarray(i).astype(int) for i in mi])
    b = np.stack([np.asarray(i).astype(int) for i in ri])
    print(f"THRESH pipeline max|d|={err:.3e} lsb={np.abs(a - b).max()}")
    assert err <= 1e-3 * scale
    assert a.shape == b.shape and np.abs(a - b).max() <= 1


def _assert_strictly_between(ref, max_value=TH["sample_max_value"]):
    s = torch.stack(ref.scheduler.seen)
    print(f"THRESH reference s per (step, sample): {s.tolist()}")
    assert bool(((s > 1.0) & (s < max_value)).any()), s.tolist()


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind,steps,eta", [("ddim", 5, 0.0), ("ddim", 5, 0.5), ("ddpm", 4, 0.0)], ids=["ddim-eta0", "ddim-eta0.5", "ddpm"])
def test_sampling_matches_the_oracle_pipeline(backend, kind, steps, eta):
    dev = select(backend)
    ref, mine = _build(kind)
    noise = _randn((2, 1, 16, 16), 42)
    step_noise = None if (kind == "ddim" and eta == 0.0) else _randn((steps, 2, 1, 16, 16), 43)
    kw = dict(batch_size=2, steps=steps, audio=False, return_float=True)
    if kind == "ddim":
        kw["eta"] = eta
    ri, rf = ref(noise=noise.clone(), step_noise=step_noise, **kw)
    mi, mf = mine(noise=noise.clone().to(dev), step_noise=None if step_noise is None else step_noise.to(dev), **kw)
    _assert_strictly_between(ref)
    _cmp(mi, mf, ri, rf)


@pytest.mark.parametrize("backend", BACKENDS)
def test_from_audio_late_start_and_mask(backend):
    dev = select(backend)
    ref, mine = _build("ddim")
    raw = (0.3 * np.random.default_rng(0).standard_normal(16 * 64 + 10)).astype(np.float32)
    noise = _randn((1, 1, 16, 16), 3)
    kw = dict(raw_audio=raw, slice=0, start_step=2, steps=6, mask_start_secs=0.05, mask_end_secs=0.03, audio=False, return_float=True)
    ri, rf = ref(noise=noise.clone(), **kw)
    ref.mel.load_audio(raw_audio=raw)
    cond_ref = ref.mel.audio_slice_to_image(0)
    mine.mel.audio_slice_to_image = lambda slice, _img=cond_ref: _img     # the same conditioning image (as tests/test_pipeline.py)
    mi, mf = mine(noise=noise.clone().to(dev), **kw)
    pps = 16 * 4000 / 16 / 64
    assert int(0.05 * pps) > 0 and int(0.03 * pps) > 0
    _assert_strictly_between(ref)
    _cmp(mi, mf, ri, rf)


COND = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 64),
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=12, attention_head_dim=4)


@pytest.mark.parametrize("backend", BACKENDS)
def test_conditional_unet_in_the_thresholded_loop(backend):
    dev = select(backend)
    ref, mine = _build("ddim", unet_cfg=COND, cond=True)
    noise, enc = _randn((2, 1, 16, 16), 42), _randn((2, 1, 12), 43)
    ri, rf = ref(batch_size=2, steps=4, noise=noise.clone(), encoding=enc, audio=False, return_float=True)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), encoding=enc.to(dev), audio=False, return_float=True)
    _assert_strictly_between(ref)
    _cmp(mi, mf, ri, rf)


VAE_TINY = dict(sample_size=(32, 32), in_channels=1, out_channels=1, latent_channels=1, layers_per_block=1,
                block_out_channels=(32, 64), down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2)
MEL32 = dict(x_res=32, y_res=32, hop_length=64, n_fft=256, n_iter=2, sample_rate=4000)


@pytest.mark.parametrize("backend", BACKENDS)
def test_latent_pipeline_with_thresholding(backend):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, AutoencoderKL, DDIMScheduler, Mel, UNet2DModel
    from oracle.vae import AutoencoderKL as OracleVAE
    torch.manual_seed(0)
    ref_unet, ref_vae = OracleUNet(**TINY).eval(), OracleVAE(**VAE_TINY).eval()
    unet = UNet2DModel(**TINY).load_state_dict(ref_unet.state_dict())
    vae = AutoencoderKL(**VAE_TINY).load_state_dict(ref_vae.state_dict())
    ref = opipe.AudioDiffusionPipeline(ref_vae, ref_unet, omel.Mel(**MEL32), RefDDIM(**TH))
    mine = AudioDiffusionPipeline(vae, unet, Mel(**MEL32), DDIMScheduler(**TH))
    mine.set_progress_bar_config(disable=True)
    noise = _randn((2, 1, 16, 16), 11)
    ri, rf = ref(batch_size=2, steps=4, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)
    assert rf.shape == mf.shape == (2, 1, 32, 32)
    _assert_strictly_between(ref)                    # the statistic is over the latent's C*H*W
    _cmp(mi, mf, ri, rf, scale=max(1.0, float(rf.abs().max())))


def _raw_loop(mine, x0, n, eta=0.0):
    """`adm_sample_loop` called directly with the scheduler's rows: what `_denoise` did before thresholding existed."""
    from audiodiffusion import _native as N
    rows = mine.scheduler.coef_rows(eta)[:n]
    coef = (N.SchedCoef * n)(*[N.SchedCoef(*[float(r[k]) for k in
                               ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise", "timestep")]) for r in rows])
    x = x0.contiguous().clone()
    B, Cc, H, W = x.shape
    u8 = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device)
    N.check(N.lib().adm_sample_loop(mine.unet._ensure_handle(), N.ptr(x), B, coef, n, None, None, 0, 0, N.ptr(u8), 1, N.stream_for(x)))
    return x, u8


@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_bit_identities(backend):
    dev = select(backend)
    from audiodiffusion import DDIMScheduler
    _, mine = _build("ddim")
    thr, n = mine.scheduler, 4
    x0 = (1.5 * _randn((3, 1, 16, 16), 9)).to(dev)
    # thresholding off: `_denoise` is `adm_sample_loop` called directly, before and after thresholded runs on the same handle
    mine.scheduler = DDIMScheduler(thresholding=False)
    mine.scheduler.set_timesteps(n)
    raw_before, raw_u8 = _raw_loop(mine, x0, n)
    off_before, off_u8 = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    assert torch.equal(off_before, raw_before) and torch.equal(off_u8, raw_u8)
    mine.scheduler = thr
    thr.set_timesteps(n)
    whole, u8 = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    # (1) one native loop == the same steps one by one through scheduler.step
    y = x0
    for t in thr.timesteps:
        y = thr.step(mine.unet(y, t)["sample"], t, y).prev_sample
    assert torch.equal(whole, y)
    # (2) captured graph on / off, (3) a second call of the same captured loop (nothing may be left over from the first)
    if backend != "emu":             # (the emulator has no graph: both settings are the same code there)
        eager, u8e = mine._denoise(x0, 0, 0.0, None, None, 0, 0, use_graph=False)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    again, u8a = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    assert torch.equal(whole, again) and torch.equal(u8, u8a)
    # (4) a sample's bits do not depend on its batch
    one, u81 = mine._denoise(x0[1:2].contiguous(), 0, 0.0, None, None, 0, 0)
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)
    # (5) sample_max_value = 1 is the static clamp to 1
    mine.scheduler = DDIMScheduler(thresholding=True, sample_max_value=1.0, clip_sample=False)
    mine.scheduler.set_timesteps(n)
    th1, th1_u8 = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    mine.scheduler = DDIMScheduler(clip_sample=True, clip_sample_range=1.0)
    mine.scheduler.set_timesteps(n)
    cl1, cl1_u8 = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    assert torch.equal(th1, cl1) and torch.equal(th1_u8, cl1_u8)
    # (6) the plain loop on the same handle is what it was
    raw_after, _ = _raw_loop(mine, x0, n)
    assert torch.equal(raw_before, raw_after) and torch.equal(cl1, raw_after)
    assert not torch.equal(raw_before, whole)


# ================================================================ F. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_save_load_round_trip_keeps_the_keys_and_samples_the_same(backend, tmp_path):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler
    _, mine = _build("ddim")
    mine.scheduler.save_pretrained(str(tmp_path / "s"))
    d = json.load(open(tmp_path / "s" / "scheduler_config.json"))
    assert d["thresholding"] is True and d["dynamic_thresholding_ratio"] == 0.9 and d["sample_max_value"] == 4.0
    s2 = DDIMScheduler.from_pretrained(str(tmp_path / "s"))
    assert dict(s2.config) == dict(mine.scheduler.config) and s2.threshold() == (0.9, 4.0)
    mine.save_pretrained(str(tmp_path / "m"))
    again = AudioDiffusionPipeline.from_pretrained(str(tmp_path / "m")).to(dev)
    again.set_progress_bar_config(disable=True)
    assert type(again.scheduler) is DDIMScheduler and dict(again.scheduler.config) == dict(mine.scheduler.config)
    noise = _randn((1, 1, 16, 16), 1)
    a = mine(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    b = again(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    assert torch.equal(a, b)
    mine.scheduler = DDIMScheduler()
    c = mine(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    assert not torch.equal(a, c)


@pytest.mark.parametrize("cls", ["DDIMScheduler", "DDPMScheduler"])
def test_a_hand_written_config_with_thresholding_loads(cls, tmp_path):
    select("emu")
    import audiodiffusion
    with open(tmp_path / "scheduler_config.json", "w") as f:
        json.dump({"_class_name": cls, "_diffusers_version": "0.24.0", "num_train_timesteps": 1000, "thresholding": True}, f)
    s = getattr(audiodiffusion, cls).from_pretrained(str(tmp_path))
    assert s.config.thresholding is True and s.threshold() == (0.995, 1.0)          # the defaults of the two other keys
    assert getattr(audiodiffusion, cls)().threshold() is None


@pytest.mark.parametrize("bad,key", [(dict(dynamic_thresholding_ratio=1.5), "dynamic_thresholding_ratio"),
                                     (dict(dynamic_thresholding_ratio=-0.1), "dynamic_thresholding_ratio"),
                                     (dict(sample_max_value=0.5), "sample_max_value"),
                                     (dict(thresholding=True, sample_max_value=float("nan")), "sample_max_value")])
@pytest.mark.parametrize("cls", ["DDIMScheduler", "DDPMScheduler"])
def test_bad_values_raise_and_name_the_key(cls, bad, key):
    select("emu")
    import audiodiffusion
    with pytest.raises(ValueError, match=key):
        getattr(audiodiffusion, cls)(**bad)


def test_the_multistep_scheduler_still_refuses_thresholding():
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError, match="thresholding"):
        DPMSolverMultistepScheduler(thresholding=True)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_version_and_argument_checks(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    assert N.lib().adm_version() >= 110
    x = _randn((1, 1, 4, 4), 0).to(dev)
    table = ops.sched_coef_table(IDENT, dev)
    out = torch.zeros((1,), dtype=torch.float32, device=dev)
    # ranks outside the sample, a weight outside [0, 1), a maximum below 1: refused before anything is launched
    for lo, hi, w, mx in [(0, 16, 0.5, 2.0), (-1, 0, 0.5, 2.0), (3, 5, 0.5, 2.0), (3, 4, 1.0, 2.0), (3, 4, 0.5, 0.5)]:
        rc = N.lib().adm_sched_threshold(N.ptr(x), N.ptr(x), N.ptr(table), None, 0, lo, hi, w, mx, N.ptr(out), 1, 1, 4, 4,
                                         N.stream_for(x))
        assert rc != 0, (lo, hi, w, mx)
    assert ops.threshold_ranks(16, 0.995) == (14, 15, float(np.float32(0.995) * np.float32(15) - np.float32(14)))
    assert ops.threshold_ranks(16, 1.0) == (15, 15, 0.0) and ops.threshold_ranks(16, 0.0) == (0, 0, 0.0)


HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_scheduler_kernels_compile_without_spills():
    """The static check of tests/test_no_spill.py on k_sched.hip: the selection and the step exist as exactly the instantiations the
    dispatch tables hold (the thresholded ones among them), and no kernel of the file uses scratch."""
    sched_kernels.assert_kernel_set_and_no_scratch()
