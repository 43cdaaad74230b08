"""Classifier-free guidance: the guided instantiations of the fused step kernel and of the selection (`adm_sched_step_guided`,
`adm_sched_threshold_guided`), the eager `step(..., model_output_uncond=, guidance_scale=)` of the three schedulers, the native loop
(`adm_sample_loop_guided`: two forwards and one guided step per captured step) inside the pipeline, and the plumbing around them — on the
emulator and, under `-m gpu`, on the MI355X.

A. The step kernel against the same formula in float64, o = u + g*(c - u) included. Bar and rule of tests/test_dpmsolver.py:
   max|d| / max|ref| <= 8 * max(e_torch_fp32, 4 * 2^-24), e_torch_fp32 the same formula in fp32 torch; for `out` and for `hist`.
B. Exact anchors that need no recalled formula: (i) uncond IS cond: c - u = 0, u + g*0 = u, so the bits of the unguided step; (ii) the guided
   kernel == the unguided kernel fed o = u + g*(c - u) from CPU torch (three separately rounded fp32 operations).
C. The selection equals torch.quantile of |x0| of that torch-combined output to the bit (rows on which x0 is +-o exactly).
D. The pipeline against a reference loop: two oracle UNet2DConditionModel forwards, the torch combination, the oracle scheduler's step (the
   oracle pipeline with its `_predict` replaced). max|d| <= 1e-3 on the final floats, images within 1 LSB, 4 steps at scale 3.0 (the
   reference's own fp32-vs-fp64 difference there is 9.8e-5 for DDIM and 2.4e-5 for DDPM; at 10 steps 7e-3: the loop is chaotic at random weights).
E. Loop identities, bit for bit. F. Plumbing. (Two gloo ranks: tests/test_guidance_distributed.py; training: tests/test_guidance_train.py.)
"""
import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_prediction_types as tp
import test_thresholding as tt
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import mel as omel
from oracle import pipeline as opipe
from oracle import schedulers as osched

_judge, _randn, _f32, COND, MEL = td._judge, td._randn, td._f32, td.COND, td.MEL
HUGE = 1e38
SCALES = [1.5, 3.0, 7.5]          # exact in fp32
PRED = {"epsilon": 0, "sample": 1, "v_prediction": 2}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _combine(u, c, g):
    """diffusers' `uncond + scale * (cond - uncond)` in the dtype of its operands: three separately rounded torch operations."""
    return u + g * (c - u)


# ================================================================ A. the step kernel against float64
ROWS = [dict(sqrt_beta=_f32(0.91), sqrt_alpha=_f32(0.41), clip=-1.0, k_x0=_f32(0.62), k_x=_f32(0.13), k_eps=_f32(0.71), k_noise=_f32(0.35),
             timestep=900.0, k_hist=_f32(-0.11)),
        dict(sqrt_beta=_f32(0.62), sqrt_alpha=_f32(0.78), clip=1.0, k_x0=_f32(0.23), k_x=_f32(0.76), k_eps=0.0, k_noise=_f32(0.4),
             timestep=500.0, k_hist=_f32(-0.31)),
        dict(sqrt_beta=_f32(0.35), sqrt_alpha=_f32(0.94), clip=-1.0, k_x0=_f32(0.44), k_x=_f32(0.52), k_eps=_f32(0.3), k_noise=0.0,
             timestep=100.0, k_hist=_f32(-0.17))]
SHAPES = [(1, 1, 4, 4), (2, 1, 16, 16), (3, 2, 8, 12)]
BIG = (1, 1, 1032, 2048)          # 528384 float4 > 2048 blocks * 256 lanes: the grid-stride loop turns over


def _v(mode="plain", pred=0, zero=False, alias=False, u8=False, dev=False, mask=False, noise=False, row=0):
    return dict(mode=mode, pred=pred, zero=zero, alias=alias, u8=u8, dev=dev, mask=mask, noise=noise, row=row)


VARIANTS = {
    "plain-epsilon": _v(), "plain-sample": _v(pred=1, row=1), "plain-v": _v(pred=2, row=2),
    "noise": _v(noise=True, row=1), "noise-v": _v(pred=2, noise=True, row=0),
    "full": _v(alias=True, u8=True, dev=True, noise=True, row=1),
    "ms-hist": _v("multistep"), "ms-zero": _v("multistep", zero=True, row=1),
    "ms-full": _v("multistep", alias=True, u8=True, dev=True, noise=True, row=1),
}
MASKED = {"mask": _v(alias=True, u8=True, dev=True, mask=True, noise=True, row=0),
          "ms-mask-zero": _v("multistep", zero=True, mask=True, u8=True, row=2)}
KCASES = []
for _s in SHAPES:
    for _n, _var in list(VARIANTS.items()) + (list(MASKED.items()) if _s[1] == 1 else []):
        KCASES.append(pytest.param(_s, _var, id="x".join(map(str, _s)) + "-" + _n))


def _formula(v, x, c_, u_, g, m1, nz, dtype):
    """The kernel's arithmetic in `dtype`; the row's fp32 coefficients and g are exact in either dtype. -> (prev, m0)"""
    r = ROWS[v["row"]]
    x, c_, u_, m1 = (t.to(dtype) for t in (x, c_, u_, m1))
    o = _combine(u_, c_, g)
    sa, sb = r["sqrt_alpha"], r["sqrt_beta"]
    if v["pred"] == 0:
        x0, e = (x - sb * o) / sa, o
    elif v["pred"] == 1:
        x0 = o
        e = (x - sa * x0) / sb
    else:
        x0, e = sa * x - sb * o, sa * o + sb * x
    m0 = x0.clamp(-r["clip"], r["clip"]) if r["clip"] >= 0 else x0
    prev = r["k_x0"] * m0 + r["k_x"] * x
    if v["mode"] == "multistep":
        if not v["zero"]:
            prev = prev + r["k_hist"] * m1
    else:
        prev = prev + r["k_eps"] * e
    if nz is not None and r["k_noise"] != 0:
        prev = prev + r["k_noise"] * nz.to(dtype)
    return prev, m0


def _run_kernel(dev, v, x, c_, u_, g, hist0, nz, mask):
    from audiodiffusion import ops
    table = ops.sched_coef_table(ROWS, dev)
    B, C, H, W = x.shape
    xd = x.clone().to(dev)
    u8 = torch.zeros((B, H * W * C), dtype=torch.uint8, device=dev) if v["u8"] else None
    step_dev = torch.tensor([v["row"]], dtype=torch.int32).to(dev) if v["dev"] else None
    kw = dict(noise=None if nz is None else nz.to(dev), mask=None if mask is None else mask.to(dev), mask_start=3 if v["mask"] else 0,
              mask_end=5 if v["mask"] else 0, out=xd if v["alias"] else None, u8_out=u8, step_dev=step_dev, uncond=u_.to(dev),
              guidance_scale=g)
    step = -1 if v["dev"] else v["row"]
    hist = None
    if v["mode"] == "multistep":
        kh = torch.tensor([0.0 if v["zero"] else r["k_hist"] for r in ROWS], dtype=torch.float32).to(dev)
        hist = hist0.clone().to(dev)
        out = ops.sched_multistep(xd, c_.to(dev), table, kh, hist, step, **kw)
    else:
        out = ops.sched_step(xd, c_.to(dev), table, step, prediction=v["pred"], **kw)
    if not v["alias"]:
        assert torch.equal(xd.cpu(), x), "x was written although out does not alias it"
    return out.cpu(), None if hist is None else hist.cpu(), None if u8 is None else u8.cpu()


def _check_kernel(backend, shape, v, g):
    dev = select(backend)
    B, C, H, W = shape
    x, c_, u_, m1 = _randn(shape, 1), _randn(shape, 2), _randn(shape, 6), _randn(shape, 3)
    nz = _randn(shape, 4) if v["noise"] else None
    mask = _randn((B, len(ROWS), H, W), 5) if v["mask"] else None
    hist0 = torch.full(shape, float("nan")) if v["zero"] else m1      # k_hist == 0: the history must not be read
    (ref64, m64), (ref32, m32) = (_formula(v, x, c_, u_, g, m1, nz, dt) for dt in (torch.float64, torch.float32))
    if mask is not None:
        for r_ in (ref64, ref32):
            r_[..., :3] = mask[:, v["row"], None, :, :3].to(r_.dtype)
            r_[..., W - 5:] = mask[:, v["row"], None, :, W - 5:].to(r_.dtype)
    out, hist, u8 = _run_kernel(dev, v, x, c_, u_, g, hist0, nz, mask)
    tag = f"GUIDANCE backend={backend} shape={shape} g={g} variant={v}"
    _judge(tag, "out", out, ref64, ref32)
    if v["mode"] == "multistep":
        _judge(tag, "hist", hist, m64, m32)          # m0 of the GUIDED output (with a mask: not the masked value)
    if mask is not None:
        assert torch.equal(out[..., :3], mask[:, v["row"], None, :, :3]) and torch.equal(out[..., W - 5:], mask[:, v["row"], None, :, W - 5:])
    if u8 is not None:
        want = ((out / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).reshape(B, -1)
        assert torch.equal(u8, want), "u8 is not the half-to-even quantisation of the kernel's own float output"
    out2, hist2, u82 = _run_kernel(dev, v, x, c_, u_, g, hist0, nz, mask)
    assert _same_bits(out, out2) and (hist is None or _same_bits(hist, hist2)) and (u8 is None or torch.equal(u8, u82))
    # guidance is really in: the unguided formula on the conditional output alone is far away
    plain, _ = _formula(v, x, c_, c_, g, m1, nz, torch.float64)
    if mask is None:
        assert float((plain - ref64).abs().max()) > 1e-2


@pytest.mark.parametrize("g", SCALES)
@pytest.mark.parametrize("shape,v", KCASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_step_against_float64(backend, shape, v, g):
    _check_kernel(backend, shape, v, g)


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_step_grid_stride_loop_turns_over(backend):
    _check_kernel(backend, BIG, VARIANTS["plain-epsilon"], 3.0)


@pytest.mark.parametrize("name", ["full", "ms-full", "noise-v"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_step_bits_of_a_sample_do_not_depend_on_its_batch(backend, name):
    dev = select(backend)
    v, shape = VARIANTS[name], (3, 2, 8, 12)
    x, c_, u_, m1, nz = (_randn(shape, s) for s in (1, 2, 6, 3, 4))
    for b in range(3):
        x[b] *= 10.0 ** b
        c_[b] *= 10.0 ** b
    one = lambda t: t[1:2].contiguous()  # noqa: E731
    out3, hist3, u83 = _run_kernel(dev, v, x, c_, u_, 3.0, m1, nz, None)
    out1, hist1, u81 = _run_kernel(dev, v, one(x), one(c_), one(u_), 3.0, one(m1), one(nz), None)
    assert _same_bits(out3[1:2], out1) and (hist3 is None or _same_bits(hist3[1:2], hist1))
    assert u83 is None or torch.equal(u83[1:2], u81)


# ================================================================ B. exact anchors
MODES = [("plain", p) for p in (0, 1, 2)] + [("thresh", p) for p in (0, 1, 2)] + [("multistep", 0)]


def _op(dev, mode, pred, x, eps, nz, m1, row, uncond=None, g=None):
    """One step through ops.* -> (out, hist or None, scale or None), on the CPU."""
    from audiodiffusion import ops
    table = ops.sched_coef_table(ROWS, dev)
    kw = {} if uncond is None else dict(uncond=uncond.to(dev), guidance_scale=g)
    if mode == "multistep":
        kh = torch.tensor([r["k_hist"] for r in ROWS], dtype=torch.float32).to(dev)
        hist = m1.clone().to(dev)
        out = ops.sched_multistep(x.to(dev), eps.to(dev), table, kh, hist, row, noise=nz.to(dev), **kw)
        return out.cpu(), hist.cpu(), None
    scale = torch.zeros((x.shape[0],), dtype=torch.float32, device=dev)
    out = ops.sched_step(x.to(dev), eps.to(dev), table, row, noise=nz.to(dev), threshold=(0.9, HUGE) if mode == "thresh" else None,
                         scale_out=scale, prediction=pred, **kw)
    return out.cpu(), None, scale.cpu() if mode == "thresh" else None


@pytest.mark.parametrize("g", SCALES)
@pytest.mark.parametrize("mode,pred", MODES, ids=[f"{m}-{p}" for m, p in MODES])
@pytest.mark.parametrize("backend", BACKENDS)
def test_anchors_same_tensor_and_torch_combined_output(backend, mode, pred, g):
    dev = select(backend)
    for shape in ((2, 1, 16, 16), (3, 2, 8, 12)):
        x, c_, u_, m1, nz = (1.5 * _randn(shape, s) for s in (11, 12, 16, 13, 14))
        for row in (0, 1):
            # (i) uncond is the conditional tensor itself: the unguided step's bits, at any scale
            cd = c_.to(dev)
            got = _op(dev, mode, pred, x, cd, nz, m1, row, uncond=cd, g=g)
            want = _op(dev, mode, pred, x, c_, nz, m1, row)
            for a, b in zip(got, want):
                assert (a is None and b is None) or _same_bits(a, b), ("same tensor", mode, pred, shape, row)
            # (ii) the guided kernel == the unguided kernel on o = u + g*(c - u) from CPU torch
            got = _op(dev, mode, pred, x, c_, nz, m1, row, uncond=u_, g=g)
            o = _combine(u_, c_, g)
            assert o.dtype == torch.float32
            want = _op(dev, mode, pred, x, o, nz, m1, row)
            for a, b in zip(got, want):
                assert (a is None and b is None) or _same_bits(a, b), ("torch-combined", mode, pred, shape, row)
            assert not torch.equal(got[0], _op(dev, mode, pred, x, c_, nz, m1, row)[0])
            if mode == "thresh":
                assert bool((got[2] > 1.0).all()), got[2].tolist()      # the threshold is really dynamic (max_value never binds)


# ================================================================ C. the selection
# rows on which x0 is +-o EXACTLY, so that torch.quantile(|o|) is the answer to the bit: epsilon with sa = sb = 1 and x = 0
# ((0 - 1*o) / 1, fused or not), sample at any row (x0 = o), v_prediction at the zero-SNR row (fma(0, x, -(1*o)))
SEL_ROWS = {0: dict(tt.IDENT[0], sqrt_beta=1.0, sqrt_alpha=1.0), 1: tt.IDENT[0], 2: dict(tt.IDENT[0], sqrt_beta=1.0, sqrt_alpha=0.0)}


def _sel_inputs(kind, shape):
    c_, u_ = 3.0 * _randn(shape, 21 + shape[2]), 2.0 * _randn(shape, 22 + shape[2])
    if kind == "ties":          # multiples of 0.25 and g a multiple of 0.5: o is a multiple of 1/8, both ranks inside long runs
        c_, u_ = torch.round(c_ * 4) / 4, torch.round(u_ * 4) / 4
    return c_.contiguous(), u_.contiguous()


@pytest.mark.parametrize("kind", ["gauss", "ties"])
@pytest.mark.parametrize("shape", tt.SEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_selection_equals_torch_quantile_to_the_bit(backend, shape, kind):
    from audiodiffusion import ops
    dev = select(backend)
    c_, u_ = _sel_inputs(kind, shape)
    n = shape[1] * shape[2] * shape[3]
    straddled = tied = False
    for g in SCALES:
        o = _combine(u_, c_, g)
        srt = o.abs().flatten(1).sort(dim=1).values
        for pred, row in SEL_ROWS.items():
            table = ops.sched_coef_table([row], dev)
            x = torch.zeros(shape) if pred == 0 else _randn(shape, 23)
            for ratio in tt.RATIOS:
                want = torch.quantile(o.abs().flatten(1), float(ratio), dim=1).clamp(min=1.0, max=HUGE)
                got = ops.sched_threshold(x.to(dev), c_.to(dev), table, 0, ratio, HUGE, prediction=pred, uncond=u_.to(dev),
                                          guidance_scale=g).cpu()
                assert got.dtype == torch.float32 and torch.equal(got, want), (kind, shape, g, pred, ratio, got.tolist(), want.tolist())
                lo, hi, _ = ops.threshold_ranks(n, ratio)
                straddled |= hi > lo and bool((srt[:, hi] != srt[:, lo]).any())
                tied |= hi > lo and bool((srt[:, hi] == srt[:, lo]).any())
        # not the selection of the conditional output alone
        alone = ops.sched_threshold(torch.zeros(shape).to(dev), c_.to(dev), ops.sched_coef_table([SEL_ROWS[0]], dev), 0, 0.9, HUGE).cpu()
        guided = ops.sched_threshold(torch.zeros(shape).to(dev), c_.to(dev), ops.sched_coef_table([SEL_ROWS[0]], dev), 0, 0.9, HUGE,
                                     uncond=u_.to(dev), guidance_scale=g).cpu()
        assert not torch.equal(alone, guided)
    if kind == "gauss":
        assert straddled, "no case in which the two ranks straddle two distinct values"
    if kind == "ties" and n >= 256:
        assert tied, "no case in which both ranks fall inside one run of equal values"


# ================================================================ D. the pipeline against a reference loop
_ORACLE = {}


def _oracle_unet():
    if "cond" not in _ORACLE:
        from oracle.unet_condition import UNet2DConditionModel as OracleCond
        torch.manual_seed(0)
        _ORACLE["cond"] = OracleCond(**COND).eval()
    return _ORACLE["cond"]


def _build(kind="ddim", ref_sched=None, vae=False, **cfg):
    """(reference pipeline, this package's pipeline) over the same conditional tiny weights."""
    from audiodiffusion import (AudioDiffusionPipeline, AutoencoderKL, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, Mel,
                                UNet2DConditionModel)
    ref_unet = _oracle_unet()
    unet = UNet2DConditionModel(**COND).load_state_dict(ref_unet.state_dict())
    classes = {"ddim": (osched.DDIMScheduler, DDIMScheduler), "ddpm": (osched.DDPMScheduler, DDPMScheduler),
               "dpm": (td.RefDPM, DPMSolverMultistepScheduler)}
    ref_vae = mine_vae = None
    mel = MEL
    if vae:
        from oracle.vae import AutoencoderKL as OracleVAE
        torch.manual_seed(1)
        ref_vae = OracleVAE(**td.VAE_TINY).eval()
        mine_vae = AutoencoderKL(**td.VAE_TINY).load_state_dict(ref_vae.state_dict())
        mel = td.MEL32
    ref = opipe.AudioDiffusionPipeline(ref_vae, ref_unet, omel.Mel(**mel), ref_sched if ref_sched is not None else classes[kind][0]())
    mine = AudioDiffusionPipeline(mine_vae, unet, Mel(**mel), classes[kind][1](**cfg))
    mine.set_progress_bar_config(disable=True)
    return ref, mine


def _guide_reference(ref, g, negative):
    """The reference loop's model call: two oracle forwards and the torch combination (then the oracle scheduler's `step`, as ever)."""
    def predict(images, t, encoding):
        neg = torch.zeros_like(encoding) if negative is None else negative.expand_as(encoding)
        c_ = ref.unet(images, t, encoding)["sample"]
        u_ = ref.unet(images, t, neg)["sample"]
        return _combine(u_, c_, g)
    ref._predict = predict


def _cmp(tag, mi, mf, ri, rf, scale=1.0):
    err = float((mf.cpu() - rf).abs().max())
    a = np.stack([np.asarray(i).astype(int) for i in mi])
    b = np.stack([np.asarray(i).astype(int) for i in ri])
    print(f"GUIDANCE pipeline {tag} max|d|={err:.3e} lsb={np.abs(a - b).max()} max|ref|={float(rf.abs().max()):.3f}")
    assert err <= 1e-3 * scale
    assert a.shape == b.shape and np.abs(a - b).max() <= 1


def _run_pair(backend, ref, mine, g=3.0, negative=None, steps=4, B=2, noisy=False, scale=None, hw=16):
    dev = select(backend)
    noise, enc = _randn((B, 1, hw, hw), 42), _randn((B, 1, 12), 43)
    step_noise = _randn((steps, B, 1, hw, hw), 44) if noisy else None
    kw = dict(batch_size=B, steps=steps, audio=False, return_float=True)
    _, unguided = ref(noise=noise.clone(), encoding=enc, step_noise=step_noise, **kw)
    _guide_reference(ref, g, negative)
    ri, rf = ref(noise=noise.clone(), encoding=enc, step_noise=step_noise, **kw)
    mi, mf = mine(noise=noise.clone().to(dev), encoding=enc.to(dev), step_noise=None if step_noise is None else step_noise.to(dev),
                  guidance_scale=g, negative_encoding=None if negative is None else negative.to(dev), **kw)
    _cmp(f"backend={backend} sched={type(mine.scheduler).__name__} negative={'zeros' if negative is None else 'given'}", mi, mf, ri, rf,
         scale=1.0 if scale is None else max(1.0, float(rf.abs().max())))
    assert float((rf - unguided).abs().max()) > 1e-2, "guidance changes nothing here: the comparison shows nothing"
    return rf


@pytest.mark.parametrize("negative", ["zeros", "given"])
@pytest.mark.parametrize("kind", ["ddim", "ddpm"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_sampling_matches_the_reference_loop(backend, kind, negative):
    select(backend)
    ref, mine = _build(kind)
    neg = None if negative == "zeros" else 0.5 * _randn((2, 1, 12), 45)
    _run_pair(backend, ref, mine, negative=neg, noisy=kind == "ddpm")


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_multistep_sampling_matches_the_restated_solver(backend):
    """`timestep_spacing="leading"` (timesteps 800, 600, 400, 200), chosen on the CPU with the reference alone: the solver does not clamp
    x0, and the default "linspace" schedule starts at t = 999, where 1 / sqrt_alpha = 160 carries the random-weight model's output to
    max|ref| = 433; the reference loop's own fp32-vs-fp64 difference is then 9.3e-4, the whole bar. From t = 800 max|ref| is 72 and that
    difference 8.3e-5, a tenth of the bar, as for the DDIM and DDPM runs above."""
    select(backend)
    ref, mine = _build("dpm", ref_sched=td.RefDPM(timestep_spacing="leading"), timestep_spacing="leading")
    _run_pair(backend, ref, mine)
    assert mine.scheduler.timesteps.tolist() == [800, 600, 400, 200]
    assert sum(r["k_hist"] != 0.0 for r in mine.scheduler.loop_rows()) == 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_thresholded_sampling_matches_the_reference_loop(backend):
    select(backend)
    ref, mine = _build("ddim", ref_sched=tt.RefDDIM(**tt.TH), **tt.TH)
    _run_pair(backend, ref, mine)
    tt._assert_strictly_between(ref)


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_v_prediction_sampling_matches_the_reference_loop(backend):
    select(backend)
    ref_sched = tp.RefDDIM()
    ref_sched.kind = "v_prediction"
    ref, mine = _build("ddim", ref_sched=ref_sched, prediction_type="v_prediction")
    _run_pair(backend, ref, mine)


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_latent_sampling_matches_the_reference_loop(backend):
    select(backend)
    ref, mine = _build("ddim", vae=True)
    rf = _run_pair(backend, ref, mine, scale="max|ref|")
    assert rf.shape == (2, 1, 32, 32)


# ================================================================ E. loop identities, bit for bit
def _eager_guided(mine, x, enc, neg, g, eta=0.0, step_noise=None):
    sched = mine.scheduler
    y = x
    for k, t in enumerate(sched.timesteps):
        c_ = mine.unet(y, t, enc)["sample"]
        u_ = mine.unet(y, t, neg)["sample"]
        kw = dict(model_output_uncond=u_, guidance_scale=g)
        if step_noise is not None:
            kw["variance_noise"] = step_noise[k]
        if eta:
            kw["eta"] = eta
        y = sched.step(c_, t, y, **kw).prev_sample
    return y


LOOPS = [("ddim", {}), ("ddpm", {}), ("dpm", {}), ("ddim", dict(tt.TH)), ("ddim", dict(prediction_type="v_prediction"))]


@pytest.mark.parametrize("kind,cfg", LOOPS, ids=["ddim", "ddpm", "dpm", "ddim-thresholded", "ddim-v"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_loop_bit_identities(backend, kind, cfg):
    dev = select(backend)
    _, mine = _build(kind, **cfg)
    sched, n, g = mine.scheduler, 3, 3.0          # (3 steps: the multistep run has its one second-order row)
    x0, enc, neg = _randn((2, 1, 16, 16), 9).to(dev), _randn((2, 1, 12), 10).to(dev), (0.5 * _randn((2, 1, 12), 11)).to(dev)
    sn = _randn((n, 2, 1, 16, 16), 12).to(dev) if kind == "ddpm" else None
    sched.set_timesteps(n)
    den = lambda x, e, **kw: mine._denoise(x, 0, 0.0, None, None, 0, 0, encoding=e, **kw)  # noqa: E731
    plain_before, _ = den(x0, enc, step_noise=sn)
    whole, u8 = den(x0, enc, step_noise=sn, guidance_scale=g, negative_encoding=neg)
    assert not torch.equal(whole, plain_before)
    # (1) the native guided loop == the same steps eagerly: two unet calls and the guided scheduler step
    assert torch.equal(whole, _eager_guided(mine, x0, enc, neg, g, step_noise=sn))
    # (2) captured graph on == off
    if backend != "emu":
        eager, u8e = den(x0, enc, step_noise=sn, guidance_scale=g, negative_encoding=neg, use_graph=False)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    # (3) a second call on the same model
    again, u8a = den(x0, enc, step_noise=sn, guidance_scale=g, negative_encoding=neg)
    assert torch.equal(whole, again) and torch.equal(u8, u8a)
    # (4) a sample's bits do not depend on its batch
    one, u81 = den(x0[1:2].contiguous(), enc[1:2].contiguous(), step_noise=None if sn is None else sn[:, 1:2].contiguous(),
                   guidance_scale=g, negative_encoding=neg[1:2].contiguous())
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)
    # (5) negative_encoding == encoding: c - u = 0, the unguided loop's bits (anchor B(i) through the executor)
    same, u8s = den(x0, enc, step_noise=sn, guidance_scale=g, negative_encoding=enc.clone())
    # (6) the unguided loop on the same handle is what it was before the guided runs
    plain_after, u8p = den(x0, enc, step_noise=sn)
    assert torch.equal(plain_before, plain_after)
    assert torch.equal(same, plain_after) and torch.equal(u8s, u8p)
    if kind != "ddim" or cfg:
        return
    # (7) scale 1.0 and None: today's call
    for off in (1.0, 0.5, None):
        y, u8y = den(x0, enc, step_noise=sn, guidance_scale=off)
        assert torch.equal(y, plain_after) and torch.equal(u8y, u8p)
    # (8) another scale is another captured graph, not a replay of the last one
    other, _ = den(x0, enc, step_noise=sn, guidance_scale=1.5, negative_encoding=neg)
    assert not torch.equal(other, whole)
    assert torch.equal(den(x0, enc, step_noise=sn, guidance_scale=g, negative_encoding=neg)[0], whole)


@pytest.mark.parametrize("backend", BACKENDS)
def test_scale_at_most_one_never_reaches_the_guided_entry_point(backend, monkeypatch):
    dev = select(backend)
    _, mine = _build("ddim")
    calls = spy_sample_loop(monkeypatch)
    noise, enc = _randn((1, 1, 16, 16), 1).to(dev), _randn((1, 1, 12), 2).to(dev)
    for g in (None, 0.0, 1.0):
        mine(batch_size=1, steps=2, noise=noise.clone(), encoding=enc, audio=False, guidance_scale=g)
    assert len(calls) == 3 and all(c["symbol"] == "adm_sample_loop_ex" and c["encoding_uncond"] is None for c in calls)
    mine(batch_size=1, steps=2, noise=noise.clone(), encoding=enc, audio=False, guidance_scale=1.0001)
    assert len(calls) == 4 and calls[3]["symbol"] == "adm_sample_loop_ex" and calls[3]["encoding_uncond"] is not None
    assert calls[3]["guidance_scale"] == np.float32(1.0001)


# ================================================================ F. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_value_errors_name_what_is_missing(backend):
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    dev = select(backend)
    _, mine = _build("ddim")
    noise, enc = _randn((2, 1, 16, 16), 1).to(dev), _randn((2, 1, 12), 2).to(dev)
    kw = dict(batch_size=2, steps=2, audio=False)
    for g in (None, 1.0, 0.3):
        with pytest.raises(ValueError, match="negative_encoding"):
            mine(noise=noise.clone(), encoding=enc, negative_encoding=enc, guidance_scale=g, **kw)
    with pytest.raises(ValueError, match="encoding"):
        mine(noise=noise.clone(), guidance_scale=3.0, **kw)
    plain = AudioDiffusionPipeline(None, UNet2DModel(**td.TINY).init_random(0), Mel(**MEL), DDIMScheduler())
    plain.set_progress_bar_config(disable=True)
    with pytest.raises(ValueError, match="UNet2DConditionModel"):
        plain(noise=noise.clone(), encoding=enc, guidance_scale=3.0, **kw)
    for bad in (float("inf"), float("-inf"), float("nan")):         # nan > 1 is False: checked before the `<= 1 is off` rule
        with pytest.raises(ValueError, match="finite"):
            mine(noise=noise.clone(), encoding=enc, guidance_scale=bad, **kw)
    for bad in (_randn((3, 1, 12), 3), _randn((2, 2, 12), 3), _randn((2, 1, 8), 3)):
        with pytest.raises(ValueError, match="negative_encoding shape"):
            mine(noise=noise.clone(), encoding=enc, negative_encoding=bad.to(dev), guidance_scale=3.0, **kw)


@pytest.mark.parametrize("backend", BACKENDS)
def test_ops_and_schedulers_want_both_guidance_arguments_or_neither(backend):
    from audiodiffusion import DDIMScheduler, DPMSolverMultistepScheduler, ops
    dev = select(backend)
    shape = (1, 1, 4, 4)
    x, c_, u_ = (_randn(shape, s).to(dev) for s in (1, 2, 3))
    table = ops.sched_coef_table(ROWS, dev)
    for kw in (dict(uncond=u_), dict(guidance_scale=3.0)):
        with pytest.raises(ValueError, match="guidance"):
            ops.sched_step(x, c_, table, 0, **kw)
        with pytest.raises(ValueError, match="guidance"):
            ops.sched_threshold(x, c_, table, 0, 0.9, 2.0, **kw)
        with pytest.raises(ValueError, match="guidance"):
            ops.sched_multistep(x, c_, table, torch.zeros(3).to(dev), torch.zeros(shape).to(dev), 0, **kw)
    for sched in (DDIMScheduler(), DPMSolverMultistepScheduler()):
        sched.set_timesteps(4)
        with pytest.raises(ValueError, match="guidance"):
            sched.step(c_, sched.timesteps[0], x, model_output_uncond=u_)
        with pytest.raises(TypeError):
            sched.step(c_, sched.timesteps[0], x, None, None, None, None, None, u_, 3.0)      # keyword-only


@pytest.mark.parametrize("backend", BACKENDS)
def test_negative_encoding_broadcasts_from_a_leading_one(backend):
    dev = select(backend)
    _, mine = _build("ddim")
    noise, enc, neg = _randn((2, 1, 16, 16), 1).to(dev), _randn((2, 1, 12), 2).to(dev), _randn((1, 1, 12), 3).to(dev)
    kw = dict(batch_size=2, steps=2, audio=False, return_float=True, encoding=enc, guidance_scale=3.0)
    _, one = mine(noise=noise.clone(), negative_encoding=neg, **kw)
    _, full = mine(noise=noise.clone(), negative_encoding=neg.expand(2, 1, 12).contiguous(), **kw)
    _, two_d = mine(noise=noise.clone(), negative_encoding=neg[:, 0], **kw)
    _, zeros = mine(noise=noise.clone(), **kw)
    _, zeros_given = mine(noise=noise.clone(), negative_encoding=torch.zeros(2, 1, 12).to(dev), **kw)
    assert torch.equal(one, full) and torch.equal(one, two_d) and torch.equal(zeros, zeros_given) and not torch.equal(one, zeros)


@pytest.mark.parametrize("backend", BACKENDS)
def test_null_encoding_buffer_is_kept_between_calls_and_never_a_callers_tensor(backend):
    """The unconditional encoding's address is in the captured graph's key: the zeros / broadcast buffer the pipeline makes is refilled in
    place by the next call (no second capture), and a caller's own tensor is used as it is and never written."""
    dev = select(backend)
    _, mine = _build("ddim")
    noise, enc = _randn((2, 1, 16, 16), 1).to(dev), _randn((2, 1, 12), 2).to(dev)
    own, lead = (0.5 * _randn((2, 1, 12), 3)).to(dev), _randn((1, 1, 12), 4).to(dev)
    own0, lead0 = own.clone(), lead.clone()
    kw = dict(batch_size=2, steps=2, audio=False, return_float=True, encoding=enc, guidance_scale=3.0)
    _, z1 = mine(noise=noise.clone(), **kw)
    p1 = mine.unet._enc_uncond.data_ptr()
    _, z2 = mine(noise=noise.clone(), **kw)
    assert mine.unet._enc_uncond.data_ptr() == p1 and torch.equal(z1, z2)
    _, b1 = mine(noise=noise.clone(), negative_encoding=lead, **kw)                 # broadcast: into the kept buffer
    assert mine.unet._enc_uncond.data_ptr() == p1 and torch.equal(mine.unet._enc_uncond, lead.expand(2, 1, 12))
    _, o1 = mine(noise=noise.clone(), negative_encoding=own, **kw)                  # the caller's tensor itself
    assert mine.unet._enc_uncond is own
    _, z3 = mine(noise=noise.clone(), **kw)                                         # zeros again: the kept buffer, not the caller's
    assert mine.unet._enc_uncond.data_ptr() == p1 and torch.equal(z3, z1)
    assert torch.equal(own, own0) and torch.equal(lead, lead0)
    _, o2 = mine(noise=noise.clone(), negative_encoding=own, **kw)
    assert torch.equal(o1, o2) and not torch.equal(o1, z1) and not torch.equal(b1, z1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_audio_diffusion_front_end_passes_both_keywords_through(backend, tmp_path):
    from audiodiffusion import AudioDiffusion
    dev = select(backend)
    _, mine = _build("ddim")
    mine.save_pretrained(str(tmp_path / "pipe"))
    front = AudioDiffusion(str(tmp_path / "pipe"), cuda=backend != "emu", progress_bar=None)
    front.pipe.set_progress_bar_config(disable=True)
    noise, enc, neg = _randn((1, 1, 16, 16), 1).to(dev), _randn((1, 1, 12), 2).to(dev), _randn((1, 1, 12), 3).to(dev)
    seen = {}
    real = front.pipe._denoise

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)
    front.pipe._denoise = spy
    img, _ = front.generate_spectrogram_and_audio(steps=2, noise=noise.clone(), encoding=enc, guidance_scale=3.0, negative_encoding=neg)
    assert seen["guidance_scale"] == 3.0 and seen["negative_encoding"] is neg
    plain, _ = front.generate_spectrogram_and_audio(steps=2, noise=noise.clone(), encoding=enc)
    assert seen["guidance_scale"] is None and seen["negative_encoding"] is None
    assert np.asarray(img).shape == (16, 16) and not np.array_equal(np.asarray(img), np.asarray(plain))


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_version_and_argument_checks(backend):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    lib = N.lib()
    assert lib.adm_version() >= 112
    for sym in ("adm_sched_threshold_guided", "adm_sched_step_guided", "adm_sample_loop_guided"):
        assert hasattr(lib, sym), sym
    shape = (1, 1, 4, 4)
    x, c_, u_, out = (_randn(shape, s).to(dev) for s in (1, 2, 3, 4))
    table = ops.sched_coef_table(ROWS, dev)
    kh, hist, scale = torch.zeros(3).to(dev), torch.zeros(shape).to(dev), torch.zeros(1).to(dev)

    def step(g=3.0, u=u_, kh_=None, hist_=None, scale_=None, pred=0):
        return lib.adm_sched_step_guided(N.ptr(x), N.ptr(c_), N.ptr(u), g, None, N.ptr(out), None, N.ptr(table), N.ptr(kh_), N.ptr(hist_),
                                         None, 0, None, 0, 0, 0, 1, 1, 4, 4, N.stream_for(x), 3, 4, 0.5, 2.0, N.ptr(scale_), pred)
    assert step() == 0 and step(kh_=kh, hist_=hist) == 0 and step(scale_=scale, pred=2) == 0
    assert step(u=None) != 0
    for bad in (float("inf"), float("nan")):
        assert step(g=bad) != 0 and "finite" in lib.adm_last_error().decode()
    assert step(kh_=kh, hist_=hist, pred=2) != 0 and "epsilon only" in lib.adm_last_error().decode()
    assert step(kh_=kh, hist_=hist, scale_=scale) != 0
    assert step(hist_=hist) != 0 and "k_hist_table" in lib.adm_last_error().decode()
    assert step(pred=3) != 0

    def sel(g=3.0, u=u_):
        return lib.adm_sched_threshold_guided(N.ptr(x), N.ptr(c_), N.ptr(u), g, N.ptr(table), None, 0, 3, 4, 0.5, 2.0, N.ptr(scale), 1, 1, 4, 4,
                                              N.stream_for(x), 0)
    assert sel() == 0 and sel(u=None) != 0 and sel(g=float("nan")) != 0
    # the loop: a conditional handle with an encoding set, and an unconditional encoding
    _, mine = _build("ddim")
    mine.scheduler.set_timesteps(2)
    rows = mine.scheduler.coef_rows()
    coef = (N.SchedCoef * 2)(*[N.SchedCoef(*[float(r[k]) for k in tp.FIELDS]) for r in rows])
    h = mine.unet._ensure_handle()
    xs, enc = _randn((1, 1, 16, 16), 5).to(dev), _randn((1, 1, 12), 6).to(dev)

    def loop(handle, neg, g=3.0, khist=None, thresholded=0, pred=0):
        return lib.adm_sample_loop_guided(handle, N.ptr(xs), 1, coef, khist, 2, None, None, 0, 0, None, 1, N.stream_for(xs), 0, 0, 0.0, 1.0,
                                          thresholded, pred, N.ptr(neg), g)
    assert loop(h, enc) != 0 and "no encoding set" in lib.adm_last_error().decode()
    mine.unet._set_encoding(h, enc, 1, dev)
    assert loop(h, None) != 0
    assert loop(h, enc, g=float("inf")) != 0 and "finite" in lib.adm_last_error().decode()
    import ctypes as C
    assert loop(h, enc, khist=(C.c_float * 2)(0.5, 0.0)) != 0 and "first order" in lib.adm_last_error().decode()
    assert loop(h, enc, khist=(C.c_float * 2)(0.0, 0.5), pred=2) != 0
    assert loop(h, enc, khist=(C.c_float * 2)(0.0, 0.5), thresholded=1) != 0
    assert loop(h, enc, pred=5) != 0
    assert loop(h, enc) == 0
    from audiodiffusion import UNet2DModel
    plain = UNet2DModel(**td.TINY).init_random(0)
    assert loop(plain._ensure_handle(), enc) != 0 and "no cross-attention" in lib.adm_last_error().decode()
