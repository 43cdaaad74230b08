"""UniPCMultistepScheduler (UniPC, Zhao et al. 2023; include/adm.h "UniPC" has the definition): the fused predictor-corrector step kernel
(csrc/k_unipc.hip), the coefficient rows, the eager `step`, the native loop inside the pipeline and the plumbing around them — on the
emulator and, under `-m gpu`, on the MI355X.

A. `adm_sched_step_ex` with `unipc_table` against the same formula in float64. Bar, the elementwise rule of tests/test_norm_sweep.py:
   max|d| / max|ref| <= 8 * max(e_torch_fp32, 4 * 2^-24), e_torch_fp32 the same formula in fp32 torch; for `out`, `last` and the written
   history slot.
B. Every coefficient within 1 fp32 ulp of a float64 restatement kept here: the definition's two formulas (`_corrector`, `_predictor`)
   evaluated on unit vectors, which is not how schedulers.py computes the rows.
C. Anchors that do not depend on the recalled formulas: order 1 without correctors is the DDIM update; order 2 without correctors is
   DPMSolverMultistepScheduler(midpoint); the observed orders of convergence on an analytic Gaussian model; and on the real schedule the
   corrected solvers beat the uncorrected ones.
D. The pipeline against the oracle pipeline driven by a torch restatement of the scheduler (`RefUniPC`): max|d| <= 1e-3 on the final
   floats, images within 1 LSB (the bars of tests/test_dpmsolver.py D).
E. Identities, bit for bit. F. Plumbing. (Two gloo ranks: tests/test_unipc_distributed.py.)
"""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_guidance as tg
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import mel as omel
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle.unet import UNet2DModel as OracleUNet

U = 2.0 ** -24
HUGE = 1e38
TINY, MEL = td.TINY, td.MEL


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
    print(f"UNIPC {tag} out={what} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} bound={bound:.3e}")
    assert e_kernel <= bound, (tag, what, e_kernel, e_torch, bound)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ================================================================ the definition, restated (B, C, D)
UDEFAULTS = dict(num_train_timesteps=1000, solver_order=2, solver_type="bh2", lower_order_final=True, disable_corrector=(),
                 timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero", prediction_type="epsilon",
                 rescale_betas_zero_snr=False, thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0)


def _ref_levels(acp, ts, final):
    """[(alpha, sigma, lambda)] of levels 0..N in float64, straight from alphas_cumprod."""
    acp = np.asarray(acp, dtype=np.float64)
    out = []
    for t in list(ts) + ([0] if final == "sigma_min" else []):
        a, s = math.sqrt(acp[t]), math.sqrt(1.0 - acp[t])
        out.append((a, s, math.log(a) - math.log(s) if a > 0 else -math.inf))
    if final == "zero":
        out.append((1.0, 0.0, math.inf))
    return out


def _ref_p(lv, i, start, order, lof):
    N = len(lv) - 1
    p = min(order, i - start + 1, N - i) if lof else min(order, i - start + 1)
    if p == 2 and math.isinf(lv[i - 1][2]):
        p = 1
    return p


def _phi_B(h, stype):
    if math.isinf(h):
        return -1.0, -1.0
    return math.expm1(-h), (math.expm1(-h) if stype == "bh2" else -h)


def _corrector(lv, i, q, stype, x_last, m1, m2, mt):
    """x_c of the definition: the move i-1 -> i re-done with m_i known."""
    (a_i, s_i, l_i), (a_p, s_p, l_p) = lv[i], lv[i - 1]
    h = l_i - l_p
    phi, B = _phi_B(h, stype)
    if math.isinf(h):
        q = 1
    if q == 1:
        hist, rho_last = 0.0, 0.5
    else:
        hh, r1 = -h, (lv[i - 2][2] - l_p) / h
        g, f, b = phi / hh - 1.0, 1.0, []
        for k in (1, 2):
            b.append(g * f / B)
            f *= k + 1
            g = g / hh - 1.0 / f
        rho = np.linalg.solve(np.array([[1.0, 1.0], [r1, 1.0]]), np.array(b))
        hist, rho_last = float(rho[0]) * (m2 - m1) / r1, float(rho[1])
    return (s_i / s_p) * x_last - a_i * phi * m1 - a_i * B * (hist + rho_last * (mt - m1))


def _predictor(lv, i, p, stype, xc, mt, m1):
    """x' of the definition: the move i -> i+1 from the corrected sample."""
    (a0, s0, l0), (a1, s1, l1) = lv[i], lv[i + 1]
    if math.isinf(l1):
        return mt
    if math.isinf(l0):
        return s1 * xc + a1 * mt
    h = l1 - l0
    phi, B = _phi_B(h, stype)
    out = (s1 / s0) * xc - a1 * phi * mt
    if p == 2:
        out = out - a1 * B * 0.5 * (m1 - mt) / ((lv[i - 1][2] - l0) / h)
    return out


def _ref_row(lv, i, start, cfg):
    """The thirteen numbers of row i in float64: the two formulas evaluated on unit vectors (both are linear)."""
    order, stype, lof, off = cfg["solver_order"], cfg["solver_type"], cfg["lower_order_final"], set(cfg["disable_corrector"])
    p = _ref_p(lv, i, start, order, lof)
    c = dict(c_x=0.0, c_m1=0.0, c_m2=0.0, c_t=0.0)
    if i > start and (i - 1) not in off:
        q = _ref_p(lv, i - 1, start, order, lof)
        c = dict(c_x=_corrector(lv, i, q, stype, 1.0, 0.0, 0.0, 0.0), c_m1=_corrector(lv, i, q, stype, 0.0, 1.0, 0.0, 0.0),
                 c_m2=_corrector(lv, i, q, stype, 0.0, 0.0, 1.0, 0.0) if q == 2 and not math.isinf(lv[i - 1][2]) else 0.0,
                 c_t=_corrector(lv, i, q, stype, 0.0, 0.0, 0.0, 1.0))
    c.update(k_x=_predictor(lv, i, p, stype, 1.0, 0.0, 0.0), k_x0=_predictor(lv, i, p, stype, 0.0, 1.0, 0.0),
             p_m1=_predictor(lv, i, p, stype, 0.0, 0.0, 1.0) if p == 2 and not math.isinf(lv[i + 1][2]) else 0.0,
             sqrt_alpha=lv[i][0], sqrt_beta=lv[i][1])
    if math.isinf(lv[i + 1][2]):
        c.update(k_x=0.0, k_x0=1.0)
    return c, p


def _zero_snr(betas):
    """Lin et al. 2023, algorithm 1, in fp32 torch."""
    abs_ = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = abs_[0].clone(), abs_[-1].clone()
    abs_ = (abs_ - last) * (first / (first - last))
    ab = abs_ ** 2
    return 1 - torch.cat([ab[0:1], ab[1:] / ab[:-1]])


class RefUniPC(osched._SchedulerBase):
    """Torch restatement for the oracle pipeline: fp32 tensors, float64 scalars, the definition's formulas as written, and the state
    machine of a multistep scheduler (the first `step` after `set_timesteps` starts the run)."""

    def __init__(self, **cfg):
        super().__init__()
        self.cfg = dict(UDEFAULTS, **cfg)
        self.config.update(dynamic_thresholding_ratio=self.cfg["dynamic_thresholding_ratio"], sample_max_value=self.cfg["sample_max_value"])
        if self.cfg["rescale_betas_zero_snr"]:
            self.betas = _zero_snr(self.betas)
            self.alphas = 1.0 - self.betas
            self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.seen = []

    def set_timesteps(self, n):
        c = self.cfg
        self.num_inference_steps = n
        ts = td._ref_timesteps(c["timestep_spacing"], n, c["num_train_timesteps"], c["steps_offset"])
        self.timesteps = torch.from_numpy(ts.copy())
        self._lv = _ref_levels(self.alphas_cumprod.double().numpy(), ts, c["final_sigmas_type"])
        self._start = self._last = self._m1 = self._m2 = None

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None):
        c, lv = self.cfg, self._lv
        i = int((self.timesteps == int(timestep)).nonzero()[0])
        if self._start is None:
            self._start = i
        a0, s0, _ = lv[i]
        kind = c["prediction_type"]
        m = (sample - s0 * model_output) / a0 if kind == "epsilon" else (model_output if kind == "sample" else a0 * sample - s0 * model_output)
        if c["thresholding"]:
            s = torch.quantile(m.abs().flatten(1), float(c["dynamic_thresholding_ratio"]), dim=1).clamp(min=1.0, max=float(c["sample_max_value"]))
            self.seen.append(s.clone())
            s = s.view(-1, 1, 1, 1)
            m = torch.clamp(m, -s, s) / s
        order, lof = c["solver_order"], c["lower_order_final"]
        xc = sample
        if i > self._start and (i - 1) not in set(c["disable_corrector"]):
            q = _ref_p(lv, i - 1, self._start, order, lof)
            xc = _corrector(lv, i, q, c["solver_type"], self._last, self._m1, self._m2 if self._m2 is not None else 0.0, m)
        prev = _predictor(lv, i, _ref_p(lv, i, self._start, order, lof), c["solver_type"], xc, m, self._m1)
        self._last, self._m2, self._m1 = xc, self._m1, m
        return {"prev_sample": prev, "pred_original_sample": m}


# ================================================================ A. kernel against float64
def _crow(sb, sa, k_x0, k_x, t):
    return dict(sqrt_beta=_f32(sb), sqrt_alpha=_f32(sa), clip=-1.0, k_x0=_f32(k_x0), k_x=_f32(k_x), k_eps=0.0, k_noise=0.0, timestep=t)


# three hand-made rows: no corrector and order 1; corrector q = 1 with p = 2; corrector q = 2 with p = 2
ROWS = [dict(_crow(0.91, 0.41, 0.23, 0.87, 900.0), c_x=0.0, c_m1=0.0, c_m2=0.0, c_t=0.0, p_m1=0.0),
        dict(_crow(0.62, 0.78, 0.57, 0.49, 500.0), c_x=_f32(0.93), c_m1=_f32(-0.045), c_m2=0.0, c_t=_f32(0.071), p_m1=_f32(-0.11)),
        dict(_crow(0.35, 0.94, 0.44, 0.52, 100.0), c_x=_f32(0.81), c_m1=_f32(0.052), c_m2=_f32(-0.013), c_t=_f32(0.16), p_m1=_f32(-0.24))]
SMALL = [(1, 1, 4, 4), (2, 1, 16, 16), (3, 2, 8, 12)]
BIG = (1, 1, 1032, 2048)
G_SCALE, PHI, RATIO = 3.0, 0.7, 0.9
BARE = dict(alias=False, u8=False, dev=False, mask=False)
ALL = dict(alias=True, u8=True, dev=True, mask=False)
MASK = dict(alias=True, u8=True, dev=True, mask=True)
KCASES = []
for _s in SMALL:
    _sid = "x".join(map(str, _s))
    for _r in (0, 1, 2):
        for _p in (0, 1, 2):
            for _t in (False, True):
                for _gd in ("none", "guided", "rescaled"):
                    KCASES.append(pytest.param(_s, _r, _p, _t, _gd, BARE, id=f"{_sid}-row{_r}-pred{_p}-{'th' if _t else 'raw'}-{_gd}"))
        for _p, _t, _gd in ((0, False, "none"), (1, True, "guided"), (2, True, "rescaled")):
            KCASES.append(pytest.param(_s, _r, _p, _t, _gd, ALL, id=f"{_sid}-row{_r}-pred{_p}-{'th' if _t else 'raw'}-{_gd}-alias-u8-dev"))
            if _s[1] == 1:
                KCASES.append(pytest.param(_s, _r, _p, _t, _gd, MASK, id=f"{_sid}-row{_r}-pred{_p}-{'th' if _t else 'raw'}-{_gd}-mask"))
KCASES.append(pytest.param(BIG, 0, 0, False, "none", BARE, id="1x1x1032x2048-plain"))
KCASES.append(pytest.param(BIG, 2, 2, True, "rescaled", ALL, id="1x1x1032x2048-full"))


def _formula(x, c_, u_, last, m1, m2, row, pred, thresh, guide, dtype):
    """The kernel's arithmetic in `dtype`; the row's coefficients are fp32 values, exact in either dtype. -> (out, x_c, m)"""
    x, c_, u_, last, m1, m2 = (None if t is None else t.to(dtype) for t in (x, c_, u_, last, m1, m2))
    o = c_
    if guide != "none":
        o = u_ + G_SCALE * (c_ - u_)
    if guide == "rescaled":
        r = c_.flatten(1).std(dim=1) / o.flatten(1).std(dim=1)
        o = PHI * (o * r.view(-1, 1, 1, 1)) + (1 - PHI) * o
    sa, sb = row["sqrt_alpha"], row["sqrt_beta"]
    m = (x - sb * o) / sa if pred == 0 else (o if pred == 1 else sa * x - sb * o)
    if thresh:
        s = torch.quantile(m.abs().flatten(1), torch.tensor(RATIO, dtype=dtype), dim=1).clamp(min=1.0, max=HUGE).view(-1, 1, 1, 1)
        m = torch.clamp(m, -s, s) / s
    xc = x
    if row["c_t"] != 0:
        xc = row["c_x"] * last + row["c_t"] * m
        if row["c_m1"] != 0:
            xc = xc + row["c_m1"] * m1
        if row["c_m2"] != 0:
            xc = xc + row["c_m2"] * m2
    out = row["k_x0"] * m + row["k_x"] * xc if row["k_x"] != 0 else row["k_x0"] * m
    if row["p_m1"] != 0:
        out = out + row["p_m1"] * m1
    return out, xc, m


def _inputs(shape, r):
    """x, the two model outputs, and the state the row reads; what it must not read is NaN."""
    x, c_, u_ = _randn(shape, 1), _randn(shape, 2), _randn(shape, 3)
    u_ = c_ + 0.3 * u_
    last, m1, m2 = x + 0.1 * _randn(shape, 4), _randn(shape, 5), _randn(shape, 6)
    row = ROWS[r]
    nan = torch.full(shape, float("nan"))
    last0 = last if row["c_t"] != 0 else nan
    hist0 = torch.empty((2,) + tuple(shape))
    hist0[r & 1] = m2 if row["c_m2"] != 0 else nan
    hist0[(r & 1) ^ 1] = m1 if (row["c_m1"] != 0 or row["p_m1"] != 0) else nan
    return x, c_, u_, last, m1, m2, last0, hist0


def _run_kernel(dev, shape, r, pred, thresh, guide, v, x, c_, u_, last0, hist0, mask, rows=ROWS):
    from audiodiffusion import ops
    table, utable = ops.sched_coef_table(rows, dev), ops.sched_unipc_table(rows, dev)
    B, Cc, H, W = shape
    xd, hist, last = x.clone().to(dev), hist0.clone().to(dev), last0.clone().to(dev)
    u8 = torch.zeros((B, H * W * Cc), dtype=torch.uint8, device=dev) if v["u8"] else None
    step_dev = torch.tensor([r], dtype=torch.int32).to(dev) if v["dev"] else None
    kw = {}
    if guide != "none":
        kw.update(uncond=u_.to(dev), guidance_scale=G_SCALE)
    if guide == "rescaled":
        kw.update(guidance_rescale=PHI)
    out = ops.sched_unipc(xd, c_.to(dev), table, utable, hist, last, -1 if v["dev"] else r, mask=None if mask is None else mask.to(dev),
                          mask_start=3 if v["mask"] else 0, mask_end=5 if v["mask"] else 0, out=xd if v["alias"] else None, u8_out=u8,
                          step_dev=step_dev, threshold=(RATIO, HUGE) if thresh else None, prediction=pred, **kw)
    if not v["alias"]:
        assert torch.equal(xd.cpu(), x), "x was written although out does not alias it"
    return out.cpu(), last.cpu(), hist.cpu(), None if u8 is None else u8.cpu()


@pytest.mark.parametrize("shape,r,pred,thresh,guide,v", KCASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_kernel_against_float64(backend, shape, r, pred, thresh, guide, v):
    dev = select(backend)
    B, Cc, H, W = shape
    x, c_, u_, last, m1, m2, last0, hist0 = _inputs(shape, r)
    row = ROWS[r]
    mask = _randn((B, len(ROWS), H, W), 7) if v["mask"] else None
    (o64, xc64, m64), (o32, xc32, m32) = (_formula(x, c_, u_, last, m1, m2, row, pred, thresh, guide, dt) for dt in (torch.float64, torch.float32))
    if mask is not None:
        for r_ in (o64, o32):
            r_[..., :3] = mask[:, r, None, :, :3].to(r_.dtype)
            r_[..., W - 5:] = mask[:, r, None, :, W - 5:].to(r_.dtype)
    out, lastk, hist, u8 = _run_kernel(dev, shape, r, pred, thresh, guide, v, x, c_, u_, last0, hist0, mask)
    tag = f"backend={backend} shape={shape} row={r} pred={pred} thresh={thresh} guide={guide} variant={v}"
    _judge(tag, "out", out, o64, o32)
    _judge(tag, "last", lastk, xc64, xc32)
    _judge(tag, "hist", hist[r & 1], m64, m32)           # row s writes slot s & 1 (rows s and s + 1: different slots) ...
    assert torch.equal(_bits(hist[(r & 1) ^ 1]), _bits(hist0[(r & 1) ^ 1])), "... and leaves the other slot alone"
    if row["c_t"] == 0:
        assert torch.equal(_bits(lastk), _bits(x)), "without a corrector last = x, bit for bit"
    if mask is not None:   # the mask goes on `out` only: last and the history are the solver's own
        assert torch.equal(out[..., :3], mask[:, r, None, :, :3]) and torch.equal(out[..., W - 5:], mask[:, r, None, :, W - 5:])
        assert not torch.equal(lastk[..., :3], out[..., :3]) and not torch.equal(hist[r & 1][..., :3], out[..., :3])
    if u8 is not None:
        want = ((out / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).reshape(B, -1)
        assert torch.equal(u8, want), "u8 is not the half-to-even quantisation of the kernel's own float output"
    out2, last2, hist2, u82 = _run_kernel(dev, shape, r, pred, thresh, guide, v, x, c_, u_, last0, hist0, mask)
    assert torch.equal(out, out2) and torch.equal(_bits(last2), _bits(lastk)) and torch.equal(_bits(hist), _bits(hist2))
    assert u8 is None or torch.equal(u8, u82)


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_row_that_ends_at_sigma_zero_returns_the_data_prediction_itself(backend):
    """k_x = 0, k_x0 = 1: x' = m_i, and the k_x*x_c product is not formed: a corrected sample that overflowed cannot turn into 0 * inf."""
    dev = select(backend)
    shape = (2, 1, 8, 8)
    row = dict(_crow(0.35, 0.94, 1.0, 0.0, 0.0), c_x=_f32(3e38), c_m1=0.0, c_m2=0.0, c_t=_f32(0.16), p_m1=0.0)
    x, c_ = _randn(shape, 1), _randn(shape, 2)
    last0 = torch.full(shape, 3e38)                      # c_x * last overflows: x_c = inf
    hist0 = torch.full((2,) + shape, float("nan"))
    out, lastk, hist, _ = _run_kernel(dev, shape, 0, 0, False, "none", BARE, x, c_, None, last0, hist0, None, rows=[row])
    assert bool(torch.isinf(lastk).all())
    assert bool(torch.isfinite(out).all()) and torch.equal(_bits(out), _bits(hist[0]))


@pytest.mark.parametrize("backend", BACKENDS)
def test_kernel_bits_of_a_sample_do_not_depend_on_its_batch(backend):
    dev = select(backend)
    shape = (3, 2, 8, 12)
    x, c_, u_, last, m1, m2, last0, hist0 = _inputs(shape, 2)
    for b in range(3):
        x[b] *= 10.0 ** b            # neighbours of very different scale
        c_[b] *= 10.0 ** b
        u_[b] *= 10.0 ** b
    one = lambda t: t[1:2].contiguous()   # noqa: E731
    for pred, thresh, guide in ((0, False, "none"), (2, True, "rescaled")):
        o3, l3, h3, u83 = _run_kernel(dev, shape, 2, pred, thresh, guide, ALL, x, c_, u_, last0, hist0, None)
        o1, l1, h1, u81 = _run_kernel(dev, (1,) + shape[1:], 2, pred, thresh, guide, ALL, one(x), one(c_), one(u_), one(last0),
                                      hist0[:, 1:2].contiguous(), None)
        assert torch.equal(o3[1:2], o1) and torch.equal(l3[1:2], l1) and torch.equal(h3[:, 1:2], h1) and torch.equal(u83[1:2], u81)


# ================================================================ B. rows
def _within_one_ulp(got, ref):
    return abs(float(np.float32(got)) - ref) <= float(np.spacing(np.float32(abs(ref))))


ROW_CASES = [dict(N=5), dict(N=20), dict(N=10, solver_type="bh1"), dict(N=6, solver_order=1), dict(N=8, lower_order_final=False),
             dict(N=12, timestep_spacing="leading", steps_offset=1), dict(N=15, timestep_spacing="trailing"),
             dict(N=9, disable_corrector=[1, 3]), dict(N=7, disable_corrector=list(range(7))),
             dict(N=16, final_sigmas_type="sigma_min"), dict(N=6, final_sigmas_type="sigma_min", solver_type="bh1"),
             dict(N=8, prediction_type="v_prediction", timestep_spacing="trailing", rescale_betas_zero_snr=True),
             dict(N=8, prediction_type="sample", timestep_spacing="trailing", rescale_betas_zero_snr=True, solver_type="bh1")]
FIELDS = ("sqrt_beta", "sqrt_alpha", "k_x0", "k_x", "c_x", "c_m1", "c_m2", "c_t", "p_m1")


@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("start", [0, 2])
def test_every_coefficient_is_within_one_ulp_of_the_float64_restatement(case, start):
    select("emu")
    from audiodiffusion import UniPCMultistepScheduler
    from audiodiffusion.schedulers import unipc_rows
    case = dict(case)
    N = case.pop("N")
    cfg = dict(UDEFAULTS, **case)
    s = UniPCMultistepScheduler(**case)
    s.set_timesteps(N)
    ts = td._ref_timesteps(cfg["timestep_spacing"], N, 1000, cfg["steps_offset"])
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == ts.tolist()        # the three spacings of the multistep class
    rows = s.loop_rows(start, None)
    assert len(rows) == N - start
    lv = _ref_levels(RefUniPC(**case).alphas_cumprod.double().numpy(), ts, cfg["final_sigmas_type"])
    off = set(cfg["disable_corrector"])
    for j, row in enumerate(rows):
        i = start + j
        want, p = _ref_row(lv, i, start, cfg)
        for k in FIELDS:
            assert math.isfinite(row[k]) and _within_one_ulp(row[k], want[k]), (i, k, row[k], want[k])
            assert row[k] == float(np.float32(row[k])), "rows hold the fp32 values the kernel reads"
        assert row["clip"] == -1.0 and row["k_eps"] == 0.0 and row["k_noise"] == 0.0 and row["timestep"] == float(ts[i])
        assert (row["c_t"] != 0.0) == (i > start and (i - 1) not in off)
        assert (row["p_m1"] != 0.0) == (p == 2 and not math.isinf(lv[i + 1][2]))
    assert (rows[0]["c_t"], rows[0]["c_m1"], rows[0]["c_m2"], rows[0]["p_m1"]) == (0.0, 0.0, 0.0, 0.0)     # a run starts without state
    if cfg["final_sigmas_type"] == "zero":
        assert (rows[-1]["k_x"], rows[-1]["k_x0"], rows[-1]["p_m1"]) == (0.0, 1.0, 0.0)
    if cfg["solver_order"] == 2 and not off:
        assert any(r["c_m2"] != 0.0 for r in rows) and any(r["p_m1"] != 0.0 for r in rows)
    if cfg["solver_order"] == 1:
        assert all(r["c_m2"] == 0.0 and r["p_m1"] == 0.0 for r in rows)
    if cfg["rescale_betas_zero_snr"] and start == 0:
        # the zero-SNR first row: alpha = 0, sigma = 1; k_x = sigma_1; row 1 has a corrector of order 1 and a predictor of order 1
        assert (rows[0]["sqrt_alpha"], rows[0]["sqrt_beta"]) == (0.0, 1.0) and rows[0]["k_x"] == _f32(lv[1][1]) and rows[0]["k_x0"] == _f32(lv[1][0])
        assert rows[1]["c_t"] != 0.0 and rows[1]["c_m2"] == 0.0 and rows[1]["p_m1"] == 0.0 and rows[2]["c_m2"] == 0.0 and rows[2]["p_m1"] != 0.0
        assert rows[1]["c_t"] == _f32(0.5 * lv[1][0])
    if start == 2:
        full = s.loop_rows(0, None)
        assert rows[2:] == full[4:] and s.loop_rows(2, 4) == rows[:2] and s.coef_rows() == full
        assert rows[0]["c_t"] == 0.0 and (2 - 1 in off or full[2]["c_t"] != 0.0)
    # the scheduler calls the pure function with its own levels
    again = unipc_rows(s._levels(), cfg["solver_order"], cfg["solver_type"], start, cfg["lower_order_final"], cfg["disable_corrector"])
    assert [{k: r[k] for k in FIELDS} for r in again[start:]] == [{k: r[k] for k in FIELDS} for r in rows]


@pytest.mark.parametrize("cfg,N", [(dict(), 1000), (dict(), 0), (dict(timestep_spacing="leading", steps_offset=150), 9),
                                   (dict(timestep_spacing="trailing", final_sigmas_type="sigma_min"), 700)],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_schedules_with_a_zero_length_row_are_rejected_as_by_the_multistep_class(cfg, N):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler, UniPCMultistepScheduler
    s = UniPCMultistepScheduler(**cfg)
    s.set_timesteps(4)
    before = s.timesteps.clone()
    with pytest.raises(ValueError) as mine:
        s.set_timesteps(N)
    with pytest.raises(ValueError) as theirs:
        DPMSolverMultistepScheduler(**cfg).set_timesteps(N)
    assert str(mine.value) == str(theirs.value)
    assert torch.equal(s.timesteps, before) and s.num_inference_steps == 4


def test_epsilon_is_refused_at_a_zero_snr_row():
    select("emu")
    from audiodiffusion import UniPCMultistepScheduler
    s = UniPCMultistepScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    with pytest.raises(ValueError, match="prediction_type='epsilon' cannot step from timestep 999"):
        s.set_timesteps(8)
    s = UniPCMultistepScheduler(rescale_betas_zero_snr=True)      # linspace reaches T - 1 as well
    with pytest.raises(ValueError, match="zero terminal"):
        s.set_timesteps(8)
    s = UniPCMultistepScheduler(rescale_betas_zero_snr=True, timestep_spacing="leading")
    s.set_timesteps(8)
    assert all(math.isfinite(v) for r in s.coef_rows() for v in r.values())


# ================================================================ C. anchors independent of recall
@pytest.mark.parametrize("backend", BACKENDS)
def test_order_one_without_correctors_is_the_ddim_update(backend):
    dev = select(backend)
    from audiodiffusion import UniPCMultistepScheduler
    N = 6
    s = UniPCMultistepScheduler(solver_order=1, disable_corrector=list(range(N)))
    s.set_timesteps(N)
    acp = s.alphas_cumprod.double()
    x = _randn((2, 1, 8, 8), 0)
    for i, t in enumerate(s.timesteps):
        eps = _randn(x.shape, 10 + i)
        a_t = acp[int(t)]
        a_p = acp[int(s.timesteps[i + 1])] if i + 1 < N else torch.tensor(1.0, dtype=torch.float64)
        refs = []
        for dt in (torch.float64, torch.float32):
            xx, ee, at, ap = x.to(dt), eps.to(dt), a_t.to(dt), a_p.to(dt)
            x0 = (xx - (1 - at) ** 0.5 * ee) / at ** 0.5
            refs.append(ap ** 0.5 * x0 + (1 - ap) ** 0.5 * ee)
        got = s.step(eps.to(dev), t, x.to(dev)).prev_sample
        _judge(f"backend={backend} ddim-anchor step={i}", "prev_sample", got, refs[0], refs[1])
        x = got.cpu()


@pytest.mark.parametrize("N", [5, 10, 20])
def test_order_two_without_correctors_has_the_rows_of_the_multistep_midpoint_solver(N):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler, UniPCMultistepScheduler
    u = UniPCMultistepScheduler(disable_corrector=list(range(N)))
    d = DPMSolverMultistepScheduler(solver_type="midpoint")
    u.set_timesteps(N), d.set_timesteps(N)
    assert u.timesteps.tolist() == d.timesteps.tolist()
    for i, (a, b) in enumerate(zip(u.coef_rows(), d.coef_rows())):
        for ka, kb in (("sqrt_alpha",) * 2, ("sqrt_beta",) * 2, ("k_x",) * 2, ("k_x0",) * 2, ("p_m1", "k_hist")):
            assert abs(a[ka] - b[kb]) <= float(np.spacing(np.float32(abs(b[kb])))), (i, ka, a[ka], b[kb])
        assert a["c_t"] == 0.0 and a["timestep"] == b["timestep"]
    assert sum(r["p_m1"] != 0.0 for r in u.coef_rows()) == N - 2


def _tiny_pipes(cfg=None):
    from audiodiffusion import AudioDiffusionPipeline, Mel, UNet2DModel, UniPCMultistepScheduler
    torch.manual_seed(0)
    ref_unet = OracleUNet(**TINY).eval()
    unet = UNet2DModel(**TINY).load_state_dict(ref_unet.state_dict())
    ref = opipe.AudioDiffusionPipeline(None, ref_unet, omel.Mel(**MEL), RefUniPC(**(cfg or {})))
    mine = AudioDiffusionPipeline(None, unet, Mel(**MEL), UniPCMultistepScheduler(**(cfg or {})))
    mine.set_progress_bar_config(disable=True)
    return ref, mine


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_epsilon_sampling_without_correctors_matches_the_multistep_scheduler(backend):
    """The same tiny model sampled with UniPC (every corrector off) and with DPMSolverMultistepScheduler(midpoint): the same rows (above),
    two kernels. The yardstick e_torch_fp32 is how far ANOTHER fp32 evaluation of the multistep update, the torch restatement `RefDPM` in the
    oracle pipeline, lies from the multistep scheduler's own result: two fp32 evaluations of one formula through this model. UniPC must lie
    within 8 * max(that, 4 * 2^-24) of the multistep result, the elementwise rule."""
    dev = select(backend)
    from audiodiffusion import DPMSolverMultistepScheduler
    N, B = 6, 2
    _, mine = _tiny_pipes(dict(disable_corrector=list(range(N))))
    ref, dpm = td._build()
    noise = _randn((B, 1, 16, 16), 42)
    kw = dict(batch_size=B, steps=N, audio=False, return_float=True)
    _, f_ref = ref(noise=noise.clone(), **kw)
    assert isinstance(dpm.scheduler, DPMSolverMultistepScheduler)
    _, f_dpm = dpm(noise=noise.clone().to(dev), **kw)
    _, f_uni = mine(noise=noise.clone().to(dev), **kw)
    anchor = f_dpm.cpu().double()
    e_torch, e_uni = _g(f_ref, anchor), _g(f_uni.cpu(), anchor)
    bound = 8 * max(e_torch, 4 * U)
    print(f"UNIPC backend={backend} 2M-anchor e_unipc={e_uni:.3e} e_torch_fp32={e_torch:.3e} bound={bound:.3e}")
    assert e_uni <= bound, (e_uni, e_torch, bound)


V0 = 0.25     # the data distribution N(0, V0): x0_hat(x) = a v x / (a^2 v + s^2); the ODE keeps x / sqrt(a^2 v + s^2) constant


def _uniform_levels(N):
    lam = [-2.0 + 4.0 * j / N for j in range(N + 1)]
    return [(1.0 / math.sqrt(1.0 + math.exp(-2 * l)), math.exp(-l) / math.sqrt(1.0 + math.exp(-2 * l)), l) for l in lam]


def _host_run(rows, lv, x):
    """The rows applied in float64 on the host to the analytic model. -> x at level N"""
    last = m1 = m2 = None
    for i, r in enumerate(rows):
        a, s, _ = lv[i]
        m = a * V0 / (a * a * V0 + s * s) * x if a > 0 else 0.0 * x
        xc = x
        if r["c_t"] != 0:
            xc = r["c_x"] * last + r["c_t"] * m + (r["c_m1"] * m1 if r["c_m1"] != 0 else 0.0) + (r["c_m2"] * m2 if r["c_m2"] != 0 else 0.0)
        nxt = r["k_x0"] * m + (r["k_x"] * xc if r["k_x"] != 0 else 0.0) + (r["p_m1"] * m1 if r["p_m1"] != 0 else 0.0)
        last, m2, m1, x = xc, m1, m, nxt
    return x


def _exact(x_T, lv):
    (aT, sT, _), (a, s, _) = lv[0], lv[-1]
    return x_T * math.sqrt(a * a * V0 + s * s) / math.sqrt(aT * aT * V0 + sT * sT)


def _grid_error(N, order, corrector):
    from audiodiffusion.schedulers import unipc_rows
    lv = _uniform_levels(N)
    rows = unipc_rows(lv, order, "bh2", 0, False, () if corrector else range(N))
    x_T = np.array([1.3, -0.7])
    return float(np.abs(_host_run(rows, lv, x_T.copy()) - _exact(x_T, lv)).max())


def test_convergence_orders_on_the_analytic_gaussian_model():
    """Uniform lambda grid on [-2, 2], no zero row, lower_order_final off. Reference ratios under step doubling: 8.0 (order 2 with the
    corrector), 4.0 (order 1 with it), 3.8 - 3.9 (order 2 without it): the corrector is what adds the order."""
    select("emu")
    e = {(o, c): {N: _grid_error(N, o, c) for N in (20, 40, 80)} for o, c in ((2, True), (1, True), (2, False))}
    print(f"UNIPC orders {e}")
    assert e[2, True][20] / e[2, True][40] >= 6 and e[2, True][40] / e[2, True][80] >= 6
    assert e[1, True][20] / e[1, True][40] >= 3 and e[1, True][40] / e[1, True][80] >= 3
    assert 3 <= e[2, False][40] / e[2, False][80] <= 5


@pytest.mark.parametrize("backend", BACKENDS)
def test_convergence_order_through_the_kernel(backend):
    """e(10) / e(20) >= 5 (reference 7.5; the errors, 4e-3 and 5e-4, are far above fp32 noise). The model is a `sample` model: its output is
    the data prediction of the analytic model, evaluated in float64 on what the kernel returned."""
    dev = select(backend)
    from audiodiffusion import ops
    from audiodiffusion.schedulers import unipc_rows
    err = {}
    for N in (10, 20):
        lv = _uniform_levels(N)
        rows = unipc_rows(lv, 2, "bh2", 0, False, ())
        table, utable = ops.sched_coef_table(rows, dev), ops.sched_unipc_table(rows, dev)
        x_T = torch.tensor([1.3, -0.7]).repeat(8).reshape(1, 1, 4, 4)
        x = x_T.clone().to(dev)
        hist, last = torch.full((2, 1, 1, 4, 4), float("nan")).to(dev), torch.full((1, 1, 4, 4), float("nan")).to(dev)
        for i in range(N):
            a, s, _ = lv[i]
            o = (a * V0 / (a * a * V0 + s * s) * x.double()).float()
            x = ops.sched_unipc(x, o, table, utable, hist, last, i, prediction=1)
        err[N] = float((x.cpu().double() - _exact(x_T.double(), lv)).abs().max())
    print(f"UNIPC backend={backend} kernel convergence {err} ratio={err[10] / err[20]:.2f}")
    assert err[10] / err[20] >= 5


def _real_error(N, order, corrector, spacing):
    from audiodiffusion import UniPCMultistepScheduler
    s = UniPCMultistepScheduler(solver_order=order, timestep_spacing=spacing, disable_corrector=[] if corrector else list(range(N)))
    s.set_timesteps(N)
    lv = s._levels()
    x_T = np.random.default_rng(7).standard_normal(16)
    ex = _exact(x_T, lv)
    return float(np.abs(_host_run(s.coef_rows(), lv, x_T.copy()) - ex).max() / np.abs(ex).max())


def test_the_corrected_solvers_beat_the_uncorrected_ones_on_the_real_schedule():
    """Linear betas, the model of N(0, 0.25), a full run to sigma = 0. Order 1 with the corrector against DDIM (reference margins: >= 1.5 %
    at N = 5, >= 25 % from N = 20); order 2 with the corrector against 2M at N = 10 and 20 on linspace (reference 0.184 vs 0.193 and 0.043
    vs 0.046; at N = 40 the reference itself loses, so it is not a case)."""
    select("emu")
    for spacing in ("linspace", "trailing"):
        for N in (5, 10, 20, 40, 80):
            ddim, unic = _real_error(N, 1, False, spacing), _real_error(N, 1, True, spacing)
            print(f"UNIPC real schedule {spacing} N={N} ddim={ddim:.4e} unipc1={unic:.4e}")
            assert unic < ddim, (spacing, N, ddim, unic)
    for N in (10, 20):
        m2, upc = _real_error(N, 2, False, "linspace"), _real_error(N, 2, True, "linspace")
        print(f"UNIPC real schedule linspace N={N} 2M={m2:.4e} unipc2={upc:.4e}")
        assert upc < m2, (N, m2, upc)


# ================================================================ D. pipeline against the oracle pipeline
def _cmp(tag, mi, mf, ri, rf, scale=1.0):
    err = float((mf.cpu() - rf).abs().max())
    a = np.stack([np.asarray(i).astype(int) for i in mi])
    b = np.stack([np.asarray(i).astype(int) for i in ri])
    print(f"UNIPC pipeline {tag} max|d|={err:.3e} lsb={np.abs(a - b).max()} max|ref|={float(rf.abs().max()):.3f}")
    assert err <= 1e-3 * scale
    assert a.shape == b.shape and np.abs(a - b).max() <= 1


TH = dict(thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=4.0)
ZERO_V = dict(prediction_type="v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
PIPE_CASES = [(1, 4, {}), (3, 4, {}), (1, 7, {}), (3, 7, {}), (2, 5, dict(prediction_type="v_prediction")), (2, 5, ZERO_V), (2, 5, TH),
              (2, 5, dict(prediction_type="sample", solver_type="bh1"))]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,steps,cfg", PIPE_CASES, ids=["b1-steps4", "b3-steps4", "b1-steps7", "b3-steps7", "v_prediction", "v-zero-snr-trailing",
                                                         "thresholded", "sample-bh1"])
def test_sampling_matches_the_oracle_pipeline(backend, B, steps, cfg, monkeypatch):
    dev = select(backend)
    ref, mine = _tiny_pipes(cfg)
    calls = spy_sample_loop(monkeypatch)
    noise = _randn((B, 1, 16, 16), 42)
    ri, rf = ref(batch_size=B, steps=steps, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = mine(batch_size=B, steps=steps, noise=noise.clone().to(dev), audio=False, return_float=True)
    _cmp(f"backend={backend} B={B} steps={steps} cfg={cfg}", mi, mf, ri, rf)
    assert mine.get_default_steps() == 20
    # ONE native call, with the new rows
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"] and calls[0]["unipc_host"] is not None and calls[0]["n_steps"] == steps
    assert calls[0]["mode"] == (1 if cfg.get("thresholding") else 0) and calls[0]["k_hist_host"] is None and calls[0]["step_noise"] is None
    assert calls[0]["prediction"] == {"epsilon": 0, "sample": 1, "v_prediction": 2}[cfg.get("prediction_type", "epsilon")]
    rows = mine.scheduler.loop_rows()
    assert sum(r["c_t"] != 0.0 for r in rows) == steps - 1 and sum(r["c_m2"] != 0.0 for r in rows) >= steps - 3
    if cfg.get("thresholding"):
        seen = torch.stack(ref.scheduler.seen)
        assert bool(((seen > 1.0) & (seen < 4.0)).any()), "no threshold strictly between the clamps: the selection shows nothing"
    if cfg.get("rescale_betas_zero_snr"):
        assert rows[0]["sqrt_alpha"] == 0.0 and int(mine.scheduler.timesteps[0]) == 999


@pytest.mark.parametrize("backend", BACKENDS)
def test_from_audio_late_start_and_mask(backend):
    dev = select(backend)
    ref, mine = _tiny_pipes()
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
    _cmp(f"backend={backend} from-audio", mi, mf, ri, rf)


def _cond_pipes(cfg=None):
    from audiodiffusion import AudioDiffusionPipeline, Mel, UNet2DConditionModel, UniPCMultistepScheduler
    ref_unet = tg._oracle_unet()
    unet = UNet2DConditionModel(**tg.COND).load_state_dict(ref_unet.state_dict())
    ref = opipe.AudioDiffusionPipeline(None, ref_unet, omel.Mel(**tg.MEL), RefUniPC(**(cfg or {})))
    mine = AudioDiffusionPipeline(None, unet, Mel(**tg.MEL), UniPCMultistepScheduler(**(cfg or {})))
    mine.set_progress_bar_config(disable=True)
    return ref, mine


def _rescaled_ref(u, c, g, phi):
    """fp32 torch, the order of the definition in include/adm.h ("guidance rescale")."""
    o = u + g * (c - u)
    r = (c.flatten(1).std(dim=1) / o.flatten(1).std(dim=1)).view(-1, 1, 1, 1)
    return phi * (o * r) + (1 - phi) * o


@pytest.mark.parametrize("backend", BACKENDS)
def test_conditional_unet_with_guidance_and_rescale(backend):
    dev = select(backend)
    g, phi, B, steps = 3.0, 0.7, 2, 4
    ref, mine = _cond_pipes(dict(timestep_spacing="leading"))      # (the spacing tests/test_guidance.py chose for the guided solver case)
    noise, enc = _randn((B, 1, 16, 16), 42), _randn((B, 1, 12), 43)
    kw = dict(batch_size=B, steps=steps, audio=False, return_float=True)
    _, plain = ref(noise=noise.clone(), encoding=enc, **kw)

    def predict(images, t, encoding):
        c_ = ref.unet(images, t, encoding)["sample"]
        u_ = ref.unet(images, t, torch.zeros_like(encoding))["sample"]
        return _rescaled_ref(u_, c_, g, phi)
    ref._predict = predict
    ri, rf = ref(noise=noise.clone(), encoding=enc, **kw)
    mi, mf = mine(noise=noise.clone().to(dev), encoding=enc.to(dev), guidance_scale=g, guidance_rescale=phi, **kw)
    _cmp(f"backend={backend} guided-rescaled", mi, mf, ri, rf)
    assert float((rf - plain).abs().max()) > 1e-2, "guidance changes nothing here: the comparison shows nothing"


@pytest.mark.parametrize("backend", BACKENDS)
def test_latent_pipeline(backend):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, AutoencoderKL, Mel, UNet2DModel, UniPCMultistepScheduler
    from oracle.vae import AutoencoderKL as OracleVAE
    torch.manual_seed(0)
    ref_unet, ref_vae = OracleUNet(**TINY).eval(), OracleVAE(**td.VAE_TINY).eval()
    unet = UNet2DModel(**TINY).load_state_dict(ref_unet.state_dict())
    vae = AutoencoderKL(**td.VAE_TINY).load_state_dict(ref_vae.state_dict())
    ref = opipe.AudioDiffusionPipeline(ref_vae, ref_unet, omel.Mel(**td.MEL32), RefUniPC())
    mine = AudioDiffusionPipeline(vae, unet, Mel(**td.MEL32), UniPCMultistepScheduler())
    mine.set_progress_bar_config(disable=True)
    noise = _randn((2, 1, 16, 16), 11)
    ri, rf = ref(batch_size=2, steps=4, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)
    assert rf.shape == mf.shape == (2, 1, 32, 32)
    _cmp(f"backend={backend} latent", mi, mf, ri, rf, scale=max(1.0, float(rf.abs().max())))


# ================================================================ E. identities, bit for bit
@pytest.mark.parametrize("cfg", [{}, dict(ZERO_V, **TH)], ids=["epsilon", "v-zero-snr-thresholded"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_bit_identities(backend, cfg):
    dev = select(backend)
    from audiodiffusion import DDIMScheduler, DPMSolverMultistepScheduler
    _, mine = _tiny_pipes(cfg)
    sched, n = mine.scheduler, 3      # a row without state, a corrector of order 1 with a predictor of order 2, a corrector of order 2
    x0 = _randn((2, 1, 16, 16), 9).to(dev)
    den = lambda x, start=0, **kw: mine._denoise(x, start, 0.0, None, None, 0, 0, **kw)   # noqa: E731
    # the DDIM loop on this handle, before any UniPC run
    mine.scheduler = DDIMScheduler()
    mine.scheduler.set_timesteps(n)
    ddim_before, _ = den(x0)
    mine.scheduler = sched
    sched.set_timesteps(n)
    whole, u8 = den(x0)
    # (1) one native loop == the same steps one by one through scheduler.step
    y = x0
    for t in sched.timesteps:
        y = sched.step(mine.unet(y, t)["sample"], t, y).prev_sample
    assert torch.equal(whole, y)
    # (2) captured graph on / off
    if backend != "emu":             # (the emulator has no graph: both settings are the same code there)
        eager, u8e = den(x0, use_graph=False)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    # (3) a second call on the same model: the first row reads no state, so the stale state of the last run is harmless
    again, u8a = den(x0)
    assert torch.equal(whole, again) and torch.equal(u8, u8a)
    # (4) a sample's bits do not depend on its batch
    one, u81 = den(x0[1:2].contiguous())
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)
    # (5) a late start is the same run as the eager steps from there (another slot parity: the loop's rows count from its first)
    late, _ = den(x0, 1)
    sched.set_timesteps(n)
    y = x0
    for t in sched.timesteps[1:]:
        y = sched.step(mine.unet(y, t)["sample"], t, y).prev_sample
    assert torch.equal(late, y)
    if cfg:
        return
    # (6) replay after other schedulers used the same handle: the graph key tells the three step kernels apart
    mine.scheduler = DPMSolverMultistepScheduler()
    mine.scheduler.set_timesteps(n)
    dpm, _ = den(x0)
    mine.scheduler = DDIMScheduler()
    mine.scheduler.set_timesteps(n)
    ddim_after, _ = den(x0)
    assert torch.equal(ddim_before, ddim_after) and not torch.equal(ddim_before, whole) and not torch.equal(dpm, whole)
    mine.scheduler = sched
    sched.set_timesteps(n)
    back, u8b = den(x0)
    assert torch.equal(whole, back) and torch.equal(u8, u8b)


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_loop_identities(backend):
    dev = select(backend)
    _, mine = _cond_pipes()
    sched, n, g = mine.scheduler, 2, 3.0
    x0, enc, neg = _randn((2, 1, 16, 16), 9).to(dev), _randn((2, 1, 12), 10).to(dev), (0.5 * _randn((2, 1, 12), 11)).to(dev)
    sched.set_timesteps(n)
    den = lambda phi, **kw: mine._denoise(x0, 0, 0.0, None, None, 0, 0, encoding=enc, guidance_scale=g, negative_encoding=neg,   # noqa: E731
                                          guidance_rescale=phi, **kw)
    zero, u80 = den(0.0)
    none, u8n = den(None)
    assert torch.equal(zero, none) and torch.equal(u80, u8n)          # guidance_rescale = 0 is None
    resc, _ = den(0.7)
    assert not torch.equal(resc, zero)
    for phi, want in ((None, zero), (0.7, resc)):                      # the loop == the eager steps
        sched.set_timesteps(n)
        y = x0
        for t in sched.timesteps:
            c_, u_ = mine.unet(y, t, enc)["sample"], mine.unet(y, t, neg)["sample"]
            y = sched.step(c_, t, y, model_output_uncond=u_, guidance_scale=g, guidance_rescale=phi).prev_sample
        assert torch.equal(want, y)
    if backend != "emu":
        assert torch.equal(resc, den(0.7, use_graph=False)[0])
    assert torch.equal(zero, den(0.0)[0])                             # after the rescaled run: the graph key holds phi


@pytest.mark.parametrize("backend", BACKENDS)
def test_device_noise_seed_only_picks_the_initial_latent(backend):
    dev = select(backend)
    from audiodiffusion import ops
    _, mine = _tiny_pipes()
    kw = dict(batch_size=2, steps=4, audio=False, return_float=True)
    _, a = mine(device_noise_seed=11, **kw)
    latent = ops.randn((2, 1, 16, 16), 11, noise_stream=1, device=dev)
    _, b = mine(noise=latent, **kw)
    assert torch.equal(a, b)


# ================================================================ F. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_save_load_round_trip_keeps_the_class_and_samples_the_same(backend, tmp_path):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, UniPCMultistepScheduler
    cfg = dict(solver_type="bh1", prediction_type="v_prediction", disable_corrector=[2], timestep_spacing="trailing", **TH)
    _, mine = _tiny_pipes(cfg)
    mine.scheduler.save_pretrained(str(tmp_path / "s"))
    d = json.load(open(tmp_path / "s" / "scheduler_config.json"))
    assert d["_class_name"] == "UniPCMultistepScheduler" and d["solver_type"] == "bh1" and d["disable_corrector"] == [2] and d["thresholding"] is True
    s2 = UniPCMultistepScheduler.from_pretrained(str(tmp_path / "s"))
    assert dict(s2.config) == dict(mine.scheduler.config)
    mine.save_pretrained(str(tmp_path / "m"))
    assert json.load(open(tmp_path / "m" / "model_index.json"))["scheduler"] == ["diffusers", "UniPCMultistepScheduler"]
    again = AudioDiffusionPipeline.from_pretrained(str(tmp_path / "m")).to(dev)
    again.set_progress_bar_config(disable=True)
    assert type(again.scheduler) is UniPCMultistepScheduler and dict(again.scheduler.config) == dict(mine.scheduler.config)
    assert again.get_default_steps() == 20
    noise = _randn((1, 1, 16, 16), 1)
    a = mine(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    b = again(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    assert torch.equal(a, b)
    # the usual way in: from the config of the scheduler a checkpoint came with; foreign keys are dropped
    s3 = UniPCMultistepScheduler.from_config(DDIMScheduler(prediction_type="v_prediction", rescale_betas_zero_snr=True,
                                                           timestep_spacing="trailing", **TH).config)
    assert s3.config.prediction_type == "v_prediction" and s3.config.rescale_betas_zero_snr is True and s3.config.thresholding is True
    assert s3.config.solver_order == 2 and "clip_sample" not in s3.config and "set_alpha_to_one" not in s3.config
    assert s3.init_noise_sigma == 1.0 and s3.scale_model_input(noise) is noise
    s3.set_timesteps(6)
    assert all(math.isfinite(v) for r in s3.coef_rows() for v in r.values())


@pytest.mark.parametrize("bad", [dict(solver_order=3), dict(predict_x0=False), dict(solver_p="dpm"), dict(use_karras_sigmas=True),
                                 dict(solver_type="heun"), dict(final_sigmas_type="sigma_max")],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_unsupported_config_raises_and_names_the_key(bad):
    select("emu")
    from audiodiffusion import UniPCMultistepScheduler
    with pytest.raises(NotImplementedError, match=next(iter(bad))):
        UniPCMultistepScheduler(**bad)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_refusals_carry_messages(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    assert N.lib().adm_version() >= 116
    shape = (1, 1, 4, 4)
    x, e = _randn(shape, 1).to(dev), _randn(shape, 2).to(dev)
    table, utable = ops.sched_coef_table(ROWS, dev), ops.sched_unipc_table(ROWS, dev)
    hist, last, out = torch.zeros((2,) + shape).to(dev), torch.zeros(shape).to(dev), torch.zeros(shape).to(dev)

    def refused(**fields):
        a, _ = ops._sched_args(x, e, table, 0, None, 0, None, None, out)
        a.unipc_table, a.hist, a.last = N.ptr(utable), N.ptr(hist), N.ptr(last)
        for k, v in fields.items():
            setattr(a, k, v)
        assert N.lib().adm_sched_step_ex(a, N.stream_for(x)) != 0
        return N.lib().adm_last_error().decode()
    assert "mode must be 0" in refused(mode=2)
    assert "noise must be NULL" in refused(noise=N.ptr(e))
    assert "noise_source must be 0" in refused(noise_source=1)
    assert "needs last" in refused(last=None)
    assert "needs scale" in refused(mode=1)
    with pytest.raises(N.NativeError, match="noise must be NULL"):
        ops.sched_unipc(x, e, table, utable, hist, last, 0, noise=e)
    assert torch.equal(out.cpu(), torch.zeros(shape)), "a refused call wrote"
    # the loop: the first row of a run has no corrector
    _, mine = _tiny_pipes()
    mine = mine.to(dev)
    h = mine.unet._ensure_handle()
    xs = _randn((1, 1, 16, 16), 3).to(dev)
    rows = [dict(ROWS[1]), dict(ROWS[2])]

    def loop(**fields):
        coef = (N.SchedCoef * 2)(*[N.SchedCoef(*[float(r[k]) for k in ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise",
                                                                         "timestep")]) for r in rows])
        uc = (N.SchedUnipcCoef * 2)(*[N.SchedUnipcCoef(*[float(r[k]) for k in ops.UNIPC_FIELDS]) for r in rows])
        args = N.SampleLoopArgs(x=N.ptr(xs), B=1, coef_host=coef, n_steps=2, use_graph=1, max_value=1.0, guidance_scale=1.0, unipc_host=uc)
        for k, v in fields.items():
            setattr(args, k, v)
        assert N.lib().adm_sample_loop_ex(h, args, N.stream_for(xs)) != 0
        return N.lib().adm_last_error().decode()
    assert "first row of a UniPC run" in loop()
    rows[0] = dict(ROWS[0])
    assert "mode must be 0" in loop(mode=2, k_hist_host=(C.c_float * 2)(0.0, 0.0))
    assert "noise_source must be 0" in loop(noise_source=1)
    assert torch.equal(xs.cpu(), _randn((1, 1, 16, 16), 3)), "a refused loop wrote"


def test_the_unipc_file_builds_exactly_its_twelve_kernels_without_scratch():
    import sched_kernels
    import unipc_kernels
    unipc_kernels.assert_kernel_set_and_no_scratch()
    sched_kernels.assert_kernel_set_and_no_scratch()      # k_sched.hip, whose helpers moved into the shared header: its set is what it was
