"""Guidance rescale (Lin et al. 2023 §3.4; include/adm.h "guidance rescale"): the statistics kernel (`guidance_stats_kernel`), the rescaled
operand of the guided step and selection kernels, `step(..., guidance_rescale=)` of the three schedulers, the native loop inside the
pipeline and the plumbing around them, on the emulator and, under `-m gpu`, on the MI355X.

The restatement (`_rescaled`), in the dtype of its operands, o = u + g*(c - u) as tests/test_guidance.py `_combine`:
    r_b = std(c_b) / std(o_b) (torch.std: unbiased; 1 where std_o == 0 or a std is not finite),  o' = phi*(o*r_b) + (1 - phi)*o
with phi the fp32 value of the keyword and 1 - phi formed in fp32 [3P-recall: diffusers' rescale_noise_cfg, restated from memory].

A. Every guided step kernel (mode x prediction x noise source: none, a buffer, the noise stream) with the rescale on against the same
   formula in float64, `out` and `hist`: tests/test_dpmsolver.py `_judge`, max|d|/max|ref| <= 8*max(e_torch_fp32, 4*2^-24).
B. Anchors that need no recalled formula: (i) rescale_out against the float64 std(c)/std(o) of the fp32 c and o: relative error <= 4*2^-24
   (two square roots and one division rounded to fp32, plus second order); (ii) phi = 1 on a row that returns the model output itself: the
   float64 std of `out` is that of c within 6*2^-24 (zero-mean family; the offset family's bound is derived in the test); (iii) phi 0 / None: the bits of the guided step; (iv) a sample's bits do not depend on
   its batch; (v) two calls, the same bits; (vi) constant c and u: r_b == 1, finite out.
C. The thresholded path's scale_out == torch.quantile of |x0| of o' formed in fp32 torch from the kernel's own rescale_out, to the bit.
D. The pipeline against the oracle pipeline with its prediction replaced by two oracle forwards and `_rescaled`: max|d| <= 1e-3 on the
   final floats, images within 1 LSB; 4 steps at g = 3.0, phi = 0.7 (figures of the reference alone in the test's docstring).
E. Loop identities, bit for bit. F. Plumbing. (Two gloo ranks: tests/test_guidance_rescale_distributed.py.)
"""
import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_guidance as tg
import test_prediction_types as tp
import test_thresholding as tt
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import schedulers as osched

_judge, _randn, _same_bits, _combine = td._judge, td._randn, tg._same_bits, tg._combine
U = 2.0 ** -24
HUGE = 1e38
PHIS = [0.3, 0.7, 1.0]
SCALES = tg.SCALES
SHAPES = [(3, 1, 4, 4),        # 4 float4 per sample, most lanes idle
          (3, 1, 36, 52),      # 468 float4: not a multiple of a wave or of the workgroup
          (3, 2, 8, 12),       # C > 1
          (1, 1, 128, 128)]    # 4096 float4: the statistics kernel's loop (2 loads x 1024 lanes) turns over; one sample alone
FAMILIES = ["normal", "offset"]            # zero mean; 5 + 0.01*randn, where fp32 accumulation would lose the variance
SEED, ROW_OFFSET = 0x1234_5678_9ABC_DEF0, 5
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


def _phi32(phi):
    """(phi, 1 - phi) as the kernel has them: the keyword rounded to fp32 and the difference formed in fp32."""
    p = np.float32(phi)
    return float(p), float(np.float32(1.0) - p)


def _cu(shape, family, seed=0):
    """The conditional and the unconditional output: the samples of a batch scaled differently, so that their r_b differ."""
    c, u = _randn(shape, 31 + seed), _randn(shape, 32 + seed)
    for b in range(shape[0]):
        c[b] *= 1.0 + b
        u[b] /= 1.0 + b
    if family == "offset":
        c, u = 5.0 + 0.01 * c, 5.0 + 0.01 * u
    return c.contiguous(), u.contiguous()


def _ratio(c, o):
    sc, so = c.flatten(1).std(dim=1), o.flatten(1).std(dim=1)
    bad = (so == 0) | ~torch.isfinite(sc) | ~torch.isfinite(so)
    return torch.where(bad, torch.ones_like(sc), sc / so)


def _rescaled(u, c, g, phi, dtype=None, r=None):
    """The restatement in `dtype` (default: the operands'). r: the (B,) factors to use instead of computing them. -> (o', r)"""
    if dtype is not None:
        u, c = u.to(dtype), c.to(dtype)
    o = _combine(u, c, g)
    r = _ratio(c, o) if r is None else r.to(o.dtype)
    p, om = _phi32(phi)
    return p * (o * r.view(-1, 1, 1, 1)) + om * o, r


# ================================================================ A. the step kernels against float64
CASES = [(m, p, nz) for m in ("plain", "thresh") for p in (0, 1, 2) for nz in ("none", "buffer", "stream")] + \
        [("multistep", 0, "none"), ("multistep", 0, "buffer")]


def _row(mode, pred, noise):
    return pred if noise == "none" and mode != "multistep" else pred % 2      # rows 0 and 1 have k_noise != 0 (and k_hist != 0)


def _formula(mode, pred, row, x, o, m1, nz, dtype):
    """The step's arithmetic in `dtype` on the (already combined and rescaled) model output o. -> (prev, m0)"""
    from audiodiffusion import ops
    r = tg.ROWS[row]
    x, o, m1 = x.to(dtype), o.to(dtype), m1.to(dtype)
    sa, sb = r["sqrt_alpha"], r["sqrt_beta"]
    if pred == 0:
        x0, e = (x - sb * o) / sa, o
    elif pred == 1:
        x0 = o
        e = (x - sa * x0) / sb
    else:
        x0, e = sa * x - sb * o, sa * o + sb * x
    if mode == "thresh":
        srt = x0.abs().flatten(1).sort(dim=1).values
        lo, hi, w = ops.threshold_ranks(srt.shape[1], 0.9)
        s = (srt[:, lo] + w * (srt[:, hi] - srt[:, lo])).clamp(min=1.0, max=HUGE).view(-1, 1, 1, 1)
        m0 = torch.minimum(torch.maximum(x0, -s), s) / s
    else:
        m0 = x0.clamp(-r["clip"], r["clip"]) if r["clip"] >= 0 else x0
    prev = r["k_x0"] * m0 + r["k_x"] * x
    prev = prev + (r["k_hist"] * m1 if mode == "multistep" else r["k_eps"] * e)
    if nz is not None and r["k_noise"] != 0:
        prev = prev + r["k_noise"] * nz.to(dtype)
    return prev, m0


def _noise(dev, shape, row, noise):
    from audiodiffusion import ops
    if noise == "none":
        return None
    if noise == "buffer":
        return _randn(shape, 4)
    return ops.randn(shape, SEED, ROW_OFFSET, t=int(tg.ROWS[row]["timestep"]), device=dev).cpu()      # what the kernel draws, materialised


def _run(dev, mode, pred, row, x, c, u, g, phi, m1, nz, noise, rescale_fill=0.0):
    """One step through ops.* -> (out, hist or None, scale or None, rescale), on the CPU."""
    from audiodiffusion import ops
    table = ops.sched_coef_table(tg.ROWS, dev)
    B = x.shape[0]
    resc = torch.full((B,), rescale_fill, dtype=torch.float32, device=dev)
    kw = dict(uncond=u.to(dev), guidance_scale=g, guidance_rescale=phi, rescale_out=resc)
    if noise == "buffer":
        kw["noise"] = nz.to(dev)
    if mode == "multistep":
        kh = torch.tensor([r["k_hist"] for r in tg.ROWS], dtype=torch.float32).to(dev)
        hist = m1.clone().to(dev)
        out = ops.sched_multistep(x.to(dev), c.to(dev), table, kh, hist, row, **kw)
        return out.cpu(), hist.cpu(), None, resc.cpu()
    if noise == "stream":
        kw.update(noise_seed=SEED, noise_row_offset=ROW_OFFSET)
    scale = torch.zeros((B,), dtype=torch.float32, device=dev)
    out = ops.sched_step(x.to(dev), c.to(dev), table, row, threshold=(0.9, HUGE) if mode == "thresh" else None, scale_out=scale,
                         prediction=pred, **kw)
    return out.cpu(), None, scale.cpu() if mode == "thresh" else None, resc.cpu()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("mode,pred,noise", CASES, ids=[f"{m}-{p}-{n}" for m, p, n in CASES])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rescaled_step_against_float64(backend, mode, pred, noise, shape):
    dev = select(backend)
    row = _row(mode, pred, noise)
    x, m1 = _randn(shape, 1), _randn(shape, 3)
    nz = _noise(dev, shape, row, noise)
    for family in FAMILIES:
        c, u = _cu(shape, family)
        for g in SCALES:
            plain64, _ = _formula(mode, pred, row, x, _combine(u.double(), c.double(), g), m1, nz, torch.float64)
            for phi in PHIS:
                (o64, _), (o32, _) = _rescaled(u, c, g, phi, torch.float64), _rescaled(u, c, g, phi, torch.float32)
                (ref64, m64), (ref32, m32) = (_formula(mode, pred, row, x, o, m1, nz, dt) for o, dt in ((o64, torch.float64), (o32, torch.float32)))
                out, hist, _, _ = _run(dev, mode, pred, row, x, c, u, g, phi, m1, nz, noise)
                tag = f"RESCALE backend={backend} {mode}-{pred}-{noise} shape={shape} family={family} g={g} phi={phi}"
                _judge(tag, "out", out, ref64, ref32)
                if mode == "multistep":
                    _judge(tag, "hist", hist, m64, m32)
                # the rescale is really in: the guided formula without it is far away
                # (not thresholded sample prediction: x0 / s does not see a per-sample factor, and row 1 has no eps term; not the
                #  offset family: row 1 clamps its x0 = o' of about 5 to 1 either way)
                if family == "normal" and not (mode == "thresh" and pred == 1):
                    assert float((plain64 - ref64).abs().max()) > 1e-3 * float(ref64.abs().max()), tag


# ================================================================ B. anchors
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("backend", BACKENDS)
def test_rescale_out_is_the_float64_ratio_of_standard_deviations(backend, shape, family):
    dev = select(backend)
    x = _randn(shape, 1)
    worst, seen = 0.0, []
    for seed in range(3):
        c, u = _cu(shape, family, seed)
        for g in SCALES:
            want = _ratio(c.double(), _combine(u, c, g).double())        # of the fp32 c and the fp32 o, in float64
            for mode in ("plain", "thresh"):
                got = _run(dev, mode, 0, 0, x, c, u, g, 0.7, x, None, "none")[3]
                err = float(((got.double() - want).abs() / want).max()) / U
                worst = max(worst, err)
                assert err <= 4.0, (shape, family, seed, g, mode, err, got.tolist(), want.tolist())
            seen.append(got.tolist())
    print(f"RESCALE rescale_out backend={backend} shape={shape} family={family} worst relative error = {worst:.2f} * 2^-24")
    assert all(len(set(r)) == shape[0] for r in seen), "the samples of a batch share a factor: a wrong row would not show"


IDENT_ROW = dict(tt.IDENT[0], sqrt_alpha=1.0)          # k_x0 = 1, every other coefficient 0, no clamp: out is the model output


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("backend", BACKENDS)
def test_full_rescale_gives_the_output_the_conditional_standard_deviation(backend, shape, family):
    from audiodiffusion import ops
    dev = select(backend)
    assert IDENT_ROW["k_x0"] == 1.0 and IDENT_ROW["clip"] < 0 and not any(IDENT_ROW[k] for k in ("k_x", "k_eps", "k_noise"))
    table = ops.sched_coef_table([IDENT_ROW], dev)
    c, u = _cu(shape, family)
    x = _randn(shape, 1)
    worst = 0.0
    for g in SCALES:
        out = ops.sched_step(x.to(dev), c.to(dev), table, 0, prediction=1, uncond=u.to(dev), guidance_scale=g, guidance_rescale=1.0).cpu()
        sc, so = c.double().flatten(1).std(dim=1), out.double().flatten(1).std(dim=1)
        err = float(((so - sc).abs() / sc).max()) / U
        worst = max(worst, err)
        if family == "normal":
            assert err <= 6.0, (shape, family, g, err)
        else:
            # 6 * 2^-24 counts the product's rounding as 2^-24 of the standard deviation, which holds where the elements are of its order.
            # Here they are 500 times larger, and no fp32 output can meet it: every element near 5 is rounded to a multiple of
            # ulp = 2^(floor(log2|out|) - 23), an error e of standard deviation ulp / sqrt(12) that is independent of the element's
            # deviation d. It moves the standard deviation by sum(d*e) / ((n - 1) * std), a sum of n independent terms whose own standard
            # deviation is (ulp / sqrt(12)) / sqrt(n - 1), relative to std: (ulp / sqrt(12)) / (std_c * sqrt(n - 1)). Four of those,
            # beside r_b's 4 * 2^-24:
            n = shape[1] * shape[2] * shape[3]
            ulp = 2.0 ** (torch.floor(torch.log2(out.double().flatten(1).abs().max(dim=1).values)) - 23)
            bound = 4.0 + 4.0 * (ulp / 12 ** 0.5) / (sc * (n - 1) ** 0.5) / U
            assert bool((((so - sc).abs() / sc) / U <= bound).all()), (shape, family, g, err, bound.tolist())
    print(f"RESCALE std(out) backend={backend} shape={shape} family={family} worst relative error = {worst:.2f} * 2^-24")


MODES = tg.MODES       # (mode, pred): plain and thresh for the three predictions, multistep for epsilon


@pytest.mark.parametrize("mode,pred", MODES, ids=[f"{m}-{p}" for m, p in MODES])
@pytest.mark.parametrize("backend", BACKENDS)
def test_zero_and_none_are_the_guided_step_and_two_calls_agree(backend, mode, pred):
    dev = select(backend)
    shape = (3, 2, 8, 12)
    x, m1, nz = _randn(shape, 1), _randn(shape, 3), _randn(shape, 4)
    c, u = _cu(shape, "normal")
    want = tg._op(dev, mode, pred, x, c, nz, m1, 1, uncond=u, g=3.0)
    for off in (None, 0, 0.0):
        got = _run(dev, mode, pred, 1, x, c, u, 3.0, off, m1, nz, "buffer", rescale_fill=-7.0)
        for a, b in zip(got[:3], want):
            assert (a is None and b is None) or _same_bits(a, b), (mode, pred, off)
        assert bool((got[3] == -7.0).all()), "rescale_out was written although the rescale is off"
    on = _run(dev, mode, pred, 1, x, c, u, 3.0, 0.7, m1, nz, "buffer")
    again = _run(dev, mode, pred, 1, x, c, u, 3.0, 0.7, m1, nz, "buffer")
    assert not torch.equal(on[0], want[0])
    for a, b in zip(on, again):
        assert (a is None and b is None) or _same_bits(a, b), (mode, pred)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES[:3], ids=_ids)
@pytest.mark.parametrize("backend", BACKENDS)
def test_bits_of_a_sample_do_not_depend_on_its_batch(backend, shape, family):
    dev = select(backend)
    x, m1, nz = _randn(shape, 1), _randn(shape, 3), _randn(shape, 4)
    c, u = _cu(shape, family)
    for mode, pred in (("plain", 0), ("thresh", 2), ("multistep", 0)):
        whole = _run(dev, mode, pred, 1, x, c, u, 3.0, 0.7, m1, nz, "buffer")
        for b in range(shape[0]):
            one = lambda t: t[b:b + 1].contiguous()  # noqa: E731
            alone = _run(dev, mode, pred, 1, one(x), one(c), one(u), 3.0, 0.7, one(m1), one(nz), "buffer")
            for w, a in zip(whole, alone):
                assert (w is None and a is None) or _same_bits(w[b:b + 1], a), (mode, pred, b)
        assert len(set(whole[3].tolist())) == shape[0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_constant_outputs_are_left_as_guidance_made_them(backend):
    dev = select(backend)
    for shape in SHAPES:
        c, u = torch.full(shape, 3.3), torch.full(shape, -1.7)
        x = _randn(shape, 1)
        for mode in ("plain", "thresh"):
            out, _, _, r = _run(dev, mode, 0, 0, x, c, u, 3.0, 0.7, x, None, "none")
            want = _run(dev, mode, 0, 0, x, c, u, 3.0, None, x, None, "none")[0]
            assert bool((r == 1.0).all()) and bool(torch.isfinite(out).all()), (shape, mode, r.tolist())
            # o' = phi*(o*1) + (1 - phi)*o: o again up to the roundings of the two products and the sum
            assert float((out - want).abs().max()) <= 8 * U * float(want.abs().max())


# ================================================================ C. the selection
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("backend", BACKENDS)
def test_rescaled_selection_equals_torch_quantile_to_the_bit(backend, shape, family):
    from audiodiffusion import ops
    dev = select(backend)
    c, u = _cu(shape, family)
    for g in SCALES:
        for phi in PHIS:
            for pred, row in tg.SEL_ROWS.items():          # rows on which x0 is +-o' exactly
                table = ops.sched_coef_table([row], dev)
                x = torch.zeros(shape) if pred == 0 else _randn(shape, 23)
                for ratio in (0.5, 0.995):
                    r = torch.zeros((shape[0],), dtype=torch.float32, device=dev)
                    got = ops.sched_threshold(x.to(dev), c.to(dev), table, 0, ratio, HUGE, prediction=pred, uncond=u.to(dev), guidance_scale=g,
                                              guidance_rescale=phi, rescale_out=r).cpu()
                    o, _ = _rescaled(u, c, g, phi, r=r.cpu())          # fp32 torch, the kernel's own factors, the definition's order
                    assert o.dtype == torch.float32
                    want = torch.quantile(o.abs().flatten(1), float(ratio), dim=1).clamp(min=1.0, max=HUGE)
                    assert torch.equal(got, want), (shape, family, g, phi, pred, ratio, got.tolist(), want.tolist())
                    # the thresholded step's own scale_out is the same selection
                    scale = torch.zeros((shape[0],), dtype=torch.float32, device=dev)
                    ops.sched_step(x.to(dev), c.to(dev), table, 0, threshold=(ratio, HUGE), scale_out=scale, prediction=pred, uncond=u.to(dev),
                                   guidance_scale=g, guidance_rescale=phi)
                    assert torch.equal(scale.cpu(), want)
        plain = ops.sched_threshold(torch.zeros(shape).to(dev), c.to(dev), ops.sched_coef_table([tg.SEL_ROWS[0]], dev), 0, 0.5, HUGE,
                                    uncond=u.to(dev), guidance_scale=g).cpu()
        resc = ops.sched_threshold(torch.zeros(shape).to(dev), c.to(dev), ops.sched_coef_table([tg.SEL_ROWS[0]], dev), 0, 0.5, HUGE,
                                   uncond=u.to(dev), guidance_scale=g, guidance_rescale=0.7).cpu()
        assert not torch.equal(plain, resc) or bool((plain == 1.0).all())          # not the selection of the unrescaled output


# ================================================================ D. the pipeline against a reference loop
class RefVThresh(tt._RefThreshold, osched.DDIMScheduler):
    """v_prediction with dynamic thresholding: diffusers' conversion (tests/test_prediction_types.py `_RefPred`), then `_threshold_sample`
    in place of the static clamp [3P-recall]."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.seen = []

    def step(self, model_output, timestep, sample, eta=0.0, generator=None, variance_noise=None):
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        sa, sb = a_t ** (0.5), (1 - a_t) ** (0.5)
        x0, e = sa * sample - sb * model_output, sa * model_output + sb * sample
        x0 = self._threshold(x0)
        prev = a_prev ** (0.5) * x0 + (1 - a_prev) ** (0.5) * e
        return {"prev_sample": prev, "pred_original_sample": x0}


def _rescale_reference(ref, g, phi):
    """The reference loop's model call: two oracle forwards, the torch combination and the torch rescale."""
    def predict(images, t, encoding):
        c_ = ref.unet(images, t, encoding)["sample"]
        u_ = ref.unet(images, t, torch.zeros_like(encoding))["sample"]
        return _rescaled(u_, c_, g, phi)[0]
    ref._predict = predict


G, PHI, STEPS = 3.0, 0.7, 4
PIPES = {"ddim": lambda: tg._build("ddim"), "ddpm": lambda: tg._build("ddpm"),
         "dpm": lambda: tg._build("dpm", ref_sched=td.RefDPM(timestep_spacing="leading"), timestep_spacing="leading"),
         "ddim-v-thresholded": lambda: tg._build("ddim", ref_sched=RefVThresh(**tt.TH), prediction_type="v_prediction", **tt.TH)}


@pytest.mark.parametrize("kind", list(PIPES))
@pytest.mark.parametrize("backend", BACKENDS)
def test_rescaled_guided_sampling_matches_the_reference_loop(backend, kind):
    """4 steps at g = 3.0, phi = 0.7, B = 2, the conditional tiny model. The reference loop alone, fp32 against the same loop in float64
    (the oracle model and every tensor of the loop in double), on the CPU: max|d| = 7.0e-5 for DDIM, 4.4e-5 for DDPM, 7.9e-5 for the
    multistep solver ("leading" spacing, as tests/test_guidance.py chose for the guided case; max|ref| = 72) and 5.0e-6 for v_prediction
    with thresholding: each under a tenth of the bar of 1e-3, so 4 steps and phi = 0.7 stay."""
    dev = select(backend)
    ref, mine = PIPES[kind]()
    B, hw = 2, 16
    noise, enc = _randn((B, 1, hw, hw), 42), _randn((B, 1, 12), 43)
    step_noise = _randn((STEPS, B, 1, hw, hw), 44) if kind == "ddpm" else None
    kw = dict(batch_size=B, steps=STEPS, audio=False, return_float=True)
    tg._guide_reference(ref, G, None)
    _, guided = ref(noise=noise.clone(), encoding=enc, step_noise=step_noise, **kw)
    _rescale_reference(ref, G, PHI)
    ri, rf = ref(noise=noise.clone(), encoding=enc, step_noise=step_noise, **kw)
    mi, mf = mine(noise=noise.clone().to(dev), encoding=enc.to(dev), step_noise=None if step_noise is None else step_noise.to(dev),
                  guidance_scale=G, guidance_rescale=PHI, **kw)
    tg._cmp(f"RESCALE backend={backend} kind={kind}", mi, mf, ri, rf)
    assert float((rf - guided).abs().max()) > 1e-2, "the rescale changes nothing here: the comparison shows nothing"
    if kind == "ddim-v-thresholded":
        tt._assert_strictly_between(ref)


# ================================================================ E. loop identities, bit for bit
def _eager(mine, x, enc, neg, g, phi, step_noise=None, seed=None, row_offset=0):
    sched = mine.scheduler
    y = x
    for k, t in enumerate(sched.timesteps):
        c_ = mine.unet(y, t, enc)["sample"]
        u_ = mine.unet(y, t, neg)["sample"]
        kw = dict(model_output_uncond=u_, guidance_scale=g, guidance_rescale=phi)
        if step_noise is not None:
            kw["variance_noise"] = step_noise[k]
        if seed is not None:
            kw.update(device_noise_seed=seed, device_noise_row_offset=row_offset)
        y = sched.step(c_, t, y, **kw).prev_sample
    return y


LOOPS = [("ddim", {}), ("ddpm", {}), ("dpm", {}), ("ddim", dict(tt.TH, prediction_type="v_prediction"))]


@pytest.mark.parametrize("kind,cfg", LOOPS, ids=["ddim", "ddpm", "dpm", "ddim-v-thresholded"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_rescaled_loop_bit_identities(backend, kind, cfg):
    dev = select(backend)
    _, mine = tg._build(kind, **cfg)
    sched, n, g = mine.scheduler, 3, 3.0
    x0, enc, neg = _randn((2, 1, 16, 16), 9).to(dev), _randn((2, 1, 12), 10).to(dev), (0.5 * _randn((2, 1, 12), 11)).to(dev)
    sn = _randn((n, 2, 1, 16, 16), 12).to(dev) if kind == "ddpm" else None
    sched.set_timesteps(n)
    den = lambda pipe, x, e, ng, phi, **kw: pipe._denoise(x, 0, 0.0, None, None, 0, 0, encoding=e, guidance_scale=g,  # noqa: E731
                                                          negative_encoding=ng, guidance_rescale=phi, **kw)
    guided, _ = den(mine, x0, enc, neg, 0.0, step_noise=sn)
    whole, u8 = den(mine, x0, enc, neg, 0.7, step_noise=sn)
    assert not torch.equal(whole, guided)
    # (1) the native loop == the same steps eagerly
    assert torch.equal(whole, _eager(mine, x0, enc, neg, g, 0.7, step_noise=sn))
    # (2) captured graph on == off
    if backend != "emu":          # (the emulator has no graph: both are the same calls there)
        eager, u8e = den(mine, x0, enc, neg, 0.7, step_noise=sn, use_graph=False)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    # (3) 0.7, 0.3, 0 in a row on one handle: each the result of a fresh pipeline (a stale graph key would replay the last value)
    for phi in (0.7, 0.3, 0.0):
        got, u8g = den(mine, x0, enc, neg, phi, step_noise=sn)
        _, fresh = tg._build(kind, **cfg)
        fresh.scheduler.set_timesteps(n)
        want, u8w = den(fresh, x0, enc, neg, phi, step_noise=sn)
        assert torch.equal(got, want) and torch.equal(u8g, u8w), phi
    assert torch.equal(got, guided)                       # phi = 0: the guided loop of before
    # (4) a sample's bits do not depend on its batch
    one, u81 = den(mine, x0[1:2].contiguous(), enc[1:2].contiguous(), neg[1:2].contiguous(), 0.7,
                   step_noise=None if sn is None else sn[:, 1:2].contiguous())
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)


@pytest.mark.parametrize("backend", BACKENDS)
def test_rescaled_loop_with_device_noise_does_not_depend_on_the_batch(backend):
    dev = select(backend)
    _, mine = tg._build("ddpm")
    mine.scheduler.set_timesteps(3)
    x0, enc, neg = _randn((3, 1, 16, 16), 9).to(dev), _randn((3, 1, 12), 10).to(dev), (0.5 * _randn((3, 1, 12), 11)).to(dev)
    den = lambda x, e, ng, off: mine._denoise(x, 0, 0.0, None, None, 0, 0, encoding=e, guidance_scale=3.0, negative_encoding=ng,  # noqa: E731
                                              guidance_rescale=0.7, device_noise_seed=SEED, device_noise_row_offset=off)
    whole, u8 = den(x0, enc, neg, 4)
    assert torch.equal(whole, _eager(mine, x0, enc, neg, 3.0, 0.7, seed=SEED, row_offset=4))
    for b in range(3):
        one, u81 = den(x0[b:b + 1].contiguous(), enc[b:b + 1].contiguous(), neg[b:b + 1].contiguous(), 4 + b)
        assert torch.equal(whole[b:b + 1], one) and torch.equal(u8[b:b + 1], u81), b


# ================================================================ F. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_pipeline_keyword_rules_and_the_off_path(backend, monkeypatch):
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    dev = select(backend)
    _, mine = tg._build("ddim")
    noise, enc = _randn((2, 1, 16, 16), 1).to(dev), _randn((2, 1, 12), 2).to(dev)
    kw = dict(batch_size=2, steps=2, audio=False, return_float=True)
    # a value in (0, 1] without active guidance names guidance_scale
    for g in (None, 1.0, 0.5):
        with pytest.raises(ValueError, match="guidance_scale"):
            mine(noise=noise.clone(), encoding=enc, guidance_scale=g, guidance_rescale=0.7, **kw)
    with pytest.raises(ValueError, match="guidance_scale"):
        mine(noise=noise.clone(), guidance_rescale=1.0, **kw)
    plain = AudioDiffusionPipeline(None, UNet2DModel(**td.TINY).init_random(0), Mel(**td.MEL), DDIMScheduler())
    plain.set_progress_bar_config(disable=True)
    with pytest.raises(ValueError, match="guidance_scale"):
        plain(noise=noise.clone(), guidance_rescale=0.7, **kw)
    # a value outside [0, 1] names guidance_rescale, guided or not
    for bad in (-0.1, 1.0001, float("nan"), float("inf")):
        for g in (None, 3.0):
            with pytest.raises(ValueError, match="guidance_rescale"):
                mine(noise=noise.clone(), encoding=enc, guidance_scale=g, guidance_rescale=bad, **kw)
    # 0 and None: the guided call of before, bit for bit, and the struct says "off"; unguided with 0 / None: the unguided call
    calls = spy_sample_loop(monkeypatch)
    _, want = mine(noise=noise.clone(), encoding=enc, guidance_scale=3.0, **kw)
    _, unguided = mine(noise=noise.clone(), encoding=enc, **kw)
    for off in (0, 0.0, None):
        _, got = mine(noise=noise.clone(), encoding=enc, guidance_scale=3.0, guidance_rescale=off, **kw)
        assert torch.equal(got, want)
        _, got = mine(noise=noise.clone(), encoding=enc, guidance_rescale=off, **kw)
        assert torch.equal(got, unguided)
    assert len(calls) == 8 and all(c["guidance_rescale"] == 0.0 for c in calls)
    _, on = mine(noise=noise.clone(), encoding=enc, guidance_scale=3.0, guidance_rescale=0.7, **kw)
    assert calls[8]["guidance_rescale"] == np.float32(0.7) and calls[8]["encoding_uncond"] is not None and not torch.equal(on, want)


@pytest.mark.parametrize("backend", BACKENDS)
def test_ops_and_scheduler_keyword_rules(backend):
    from audiodiffusion import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, ops
    dev = select(backend)
    shape = (1, 1, 4, 4)
    x, c_, u_ = (_randn(shape, s).to(dev) for s in (1, 2, 3))
    table = ops.sched_coef_table(tg.ROWS, dev)
    calls = [lambda **kw: ops.sched_step(x, c_, table, 0, **kw), lambda **kw: ops.sched_threshold(x, c_, table, 0, 0.9, 2.0, **kw),
             lambda **kw: ops.sched_multistep(x, c_, table, torch.zeros(3).to(dev), torch.zeros(shape).to(dev), 0, **kw)]
    for sched in (DDIMScheduler(), DDPMScheduler(), DPMSolverMultistepScheduler()):
        sched.set_timesteps(4)
        calls.append(lambda s=sched, **kw: s.step(c_, s.timesteps[1], x, **{dict(uncond="model_output_uncond").get(k, k): v
                                                                            for k, v in kw.items()}))
        with pytest.raises(TypeError):
            sched.step(c_, sched.timesteps[1], x, None, None, None, None, None, u_, 3.0, None, 0, 0.7)      # keyword-only
    for call in calls:
        with pytest.raises(ValueError, match="guidance_scale"):
            call(guidance_rescale=0.7)
        for bad in (-0.5, 1.5, float("nan")):
            with pytest.raises(ValueError, match="guidance_rescale"):
                call(uncond=u_, guidance_scale=3.0, guidance_rescale=bad)
        call(guidance_rescale=0.0)
        call(guidance_rescale=None)
        call(uncond=u_, guidance_scale=3.0, guidance_rescale=0.7)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_version_and_refusals(backend):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    lib = N.lib()
    assert lib.adm_version() >= 115
    shape = (2, 1, 4, 8)
    x, c_, u_, out = (_randn(shape, s).to(dev) for s in (1, 2, 3, 4))
    table = ops.sched_coef_table(tg.ROWS, dev)
    scale, resc = torch.zeros(2).to(dev), torch.zeros(2).to(dev)
    lo, hi, w = ops.threshold_ranks(32, 0.9)

    def args(**fields):
        a = N.SchedStepArgs(x=N.ptr(x), eps=N.ptr(c_), out=N.ptr(out), coef_table=N.ptr(table), step=1, B=2, C=1, H=4, W=8, max_value=2.0,
                            lo=lo, hi=hi, w=w, scale=N.ptr(scale), mode=N.SCHED_THRESH, eps_uncond=N.ptr(u_), guidance_scale=3.0,
                            guidance_rescale=0.7, rescale=N.ptr(resc))
        for k, v in fields.items():
            setattr(a, k, v)
        return a
    for name, entry in (("sched_step", lib.adm_sched_step_ex), ("sched_threshold", lib.adm_sched_threshold_ex)):
        assert entry(args(), N.stream_for(x)) == 0 and entry(args(guidance_rescale=0.0, rescale=None), N.stream_for(x)) == 0
        assert entry(args(guidance_rescale=0.0, rescale=None, eps_uncond=None), N.stream_for(x)) == 0
        refused = [(dict(guidance_rescale=-0.25), "must be in [0, 1]"), (dict(guidance_rescale=1.5), "must be in [0, 1]"),
                   (dict(guidance_rescale=float("nan")), "must be in [0, 1]"), (dict(guidance_rescale=float("inf")), "must be in [0, 1]"),
                   (dict(eps_uncond=None), "needs eps_uncond"), (dict(rescale=None), "needs the rescale buffer")]
        for fields, why in refused:
            assert entry(args(**fields), N.stream_for(x)) != 0, (name, fields)
            msg = lib.adm_last_error().decode()
            assert why in msg and name + ": guidance_rescale" in msg, (name, fields, msg)      # the entry point's own name, in mode 1 too
    plain = args(mode=N.SCHED_PLAIN, scale=None)
    assert lib.adm_sched_step_ex(plain, N.stream_for(x)) == 0
    assert lib.adm_sched_step_ex(args(mode=N.SCHED_PLAIN, scale=None, rescale=None), N.stream_for(x)) != 0
    # the loop
    _, mine = tg._build("ddim")
    mine.scheduler.set_timesteps(2)
    rows = mine.scheduler.coef_rows()
    coef = (N.SchedCoef * 2)(*[N.SchedCoef(*[float(r[k]) for k in tp.FIELDS]) for r in rows])
    h = mine.unet._ensure_handle()
    xs, enc = _randn((1, 1, 16, 16), 5).to(dev), _randn((1, 1, 12), 6).to(dev)
    mine.unet._set_encoding(h, enc, 1, dev)

    def loop(**fields):
        a = N.SampleLoopArgs(x=N.ptr(xs), B=1, coef_host=coef, n_steps=2, use_graph=1, max_value=1.0, encoding_uncond=N.ptr(enc),
                             guidance_scale=3.0, guidance_rescale=0.7)
        for k, v in fields.items():
            setattr(a, k, v)
        return lib.adm_sample_loop_ex(h, a, N.stream_for(xs))
    assert loop() == 0 and loop(guidance_rescale=0.0) == 0 and loop(guidance_rescale=0.0, encoding_uncond=None) == 0
    for bad in (-0.25, 1.5, float("nan")):
        assert loop(guidance_rescale=bad) != 0 and "must be in [0, 1]" in lib.adm_last_error().decode()
    assert loop(encoding_uncond=None) != 0 and "needs encoding_uncond" in lib.adm_last_error().decode()


@pytest.mark.parametrize("backend", BACKENDS)
def test_audio_diffusion_front_end_passes_the_keyword_through(backend, tmp_path):
    from audiodiffusion import AudioDiffusion
    dev = select(backend)
    _, mine = tg._build("ddim")
    mine.save_pretrained(str(tmp_path / "pipe"))
    front = AudioDiffusion(str(tmp_path / "pipe"), cuda=backend != "emu", progress_bar=None)
    front.pipe.set_progress_bar_config(disable=True)
    noise, enc = _randn((1, 1, 16, 16), 1).to(dev), _randn((1, 1, 12), 2).to(dev)
    seen = {}
    real = front.pipe._denoise

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)
    front.pipe._denoise = spy
    img, _ = front.generate_spectrogram_and_audio(steps=2, noise=noise.clone(), encoding=enc, guidance_scale=3.0, guidance_rescale=0.7)
    assert seen["guidance_rescale"] == 0.7
    plain, _ = front.generate_spectrogram_and_audio(steps=2, noise=noise.clone(), encoding=enc, guidance_scale=3.0)
    assert seen["guidance_rescale"] == 0.0 and not np.array_equal(np.asarray(img), np.asarray(plain))


def test_train_script_flag_reaches_the_pipeline(tmp_path, monkeypatch):
    import test_train_script as ts
    select("emu")
    tr = ts._script("train_unet")
    seen = []

    class Pipe:
        def set_progress_bar_config(self, **kw):
            pass

        def __call__(self, **kw):
            seen.append(kw)
            from PIL import Image
            return [Image.new("L", (4, 4))] * 2, (4000, [np.zeros(8, dtype=np.float32)] * 2)
    enc = [torch.zeros(1, 12), torch.ones(1, 12)]
    args = tr.parse_args(["--eval_batch_size", "2", "--guidance_scale", "3.0"])
    assert args.guidance_rescale is None
    tr.write_samples(Pipe(), args, 0, str(tmp_path), torch.device("cpu"), enc)
    assert "guidance_rescale" not in seen[0]                     # unset: the call of before
    args = tr.parse_args(["--eval_batch_size", "2", "--guidance_scale", "3.0", "--guidance_rescale", "0.7"])
    tr.write_samples(Pipe(), args, 0, str(tmp_path), torch.device("cpu"), enc)
    assert seen[1]["guidance_rescale"] == 0.7 and seen[1]["guidance_scale"] == 3.0
    # ... and through the real pipeline's __call__ into the loop's struct (two steps instead of the scheduler's default)
    _, mine = tg._build("ddim")
    mine.get_default_steps = lambda: 2
    calls = spy_sample_loop(monkeypatch)
    tr.write_samples(mine, args, 0, str(tmp_path), torch.device("cpu"), [_randn((1, 12), 1), _randn((1, 12), 2)])
    assert len(calls) == 1 and calls[0]["guidance_rescale"] == np.float32(0.7) and calls[0]["guidance_scale"] == 3.0
