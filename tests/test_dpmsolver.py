"""DPMSolverMultistepScheduler (DPM-Solver++ 2M): the fused multistep step kernel, the coefficient tables, the eager `step`, the native
loop (`adm_sample_loop_multistep`) inside the pipeline, and the plumbing around them — on the emulator and, under `-m gpu`, on the MI355X.

A. `adm_sched_multistep` against the same formula in float64. Bar, the elementwise rule of tests/test_norm_sweep.py:
   max|d| / max|ref| <= 8 * max(e_torch_fp32, 4 * 2^-24), e_torch_fp32 the same formula in fp32 torch; for `out` and for `hist`.
B. Timesteps against the closed forms, every coefficient within 1 fp32 ulp of a float64 restatement kept here (`_ref_coefs`).
C. Anchors that do not depend on the recalled formulas: order 1 is the DDIM update; on an analytic Gaussian model the second-order rows
   beat the first-order ones against the exact solution of the probability-flow ODE.
D. The pipeline against the oracle pipeline driven by a torch restatement of the scheduler (`RefDPM`): max|d| <= 1e-3 on the final floats,
   images within 1 LSB (the bars of tests/test_pipeline.py, without the identical-pixel share: 512 pixels are too few for that cap).
E. Plumbing: save / load, unsupported configs, default steps. (Two gloo ranks: tests/test_dpmsolver_distributed.py.)
"""
import json
import math

import numpy as np
import pytest
import torch

from native_backend import BACKENDS, select
from oracle import mel as omel
from oracle import pipeline as opipe
from oracle import schedulers as osched
from oracle.unet import UNet2DModel as OracleUNet

U = 2.0 ** -24
TINY = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 64),
            down_block_types=("DownBlock2D", "AttnDownBlock2D"), up_block_types=("AttnUpBlock2D", "UpBlock2D"))
MEL = dict(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=2, sample_rate=4000)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _g(a, ref):
    return float((a.double() - ref).abs().max() / ref.abs().max())


def _judge(tag, what, got, ref64, ref32):
    got = got.detach().cpu()
    assert got.shape == ref64.shape == ref32.shape
    assert bool(torch.isfinite(got).all()), (tag, what, "kernel output is not finite")
    e_kernel, e_torch = _g(got, ref64), _g(ref32, ref64)
    bound = 8 * max(e_torch, 4 * U)
    print(f"DPMSOLVER {tag} out={what} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} bound={bound:.3e}")
    assert e_kernel <= bound, (tag, what, e_kernel, e_torch, bound)


# ================================================================ float64 restatement of the solver (B, D)
DEFAULTS = dict(num_train_timesteps=1000, solver_order=2, solver_type="midpoint", lower_order_final=True, euler_at_final=False,
                timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero")


def _ref_timesteps(spacing, N, T=1000, offset=0):
    if spacing == "linspace":
        return np.linspace(0, T - 1, N + 1).round()[::-1][:-1].astype(np.int64)
    if spacing == "leading":
        return ((np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1] + offset).astype(np.int64)
    return (np.arange(T, 0, -T / N).round() - 1).astype(np.int64)


def _ref_sigmas(acp, ts, final):
    acp = np.asarray(acp, dtype=np.float64)
    sig = ((1 - acp[ts]) / acp[ts]) ** 0.5
    return np.concatenate([sig, [0.0 if final == "zero" else ((1 - acp[0]) / acp[0]) ** 0.5]])


def _alpha_s_lambda(sigma):
    a = 1.0 / math.sqrt(sigma ** 2 + 1.0)
    return a, sigma * a, (math.log(a) - math.log(sigma * a)) if sigma > 0 else math.inf


def _ref_first_order(cfg, i, N, start):
    last = i == N - 1
    return (cfg["solver_order"] == 1 or i == start or
            (last and (cfg["euler_at_final"] or (cfg["lower_order_final"] and N < 15) or cfg["final_sigmas_type"] == "zero")))


def _ref_coefs(sig, i, first, solver_type):
    """(k_x, k_x0, k_hist) of row i in float64, in the shape the solver is usually written:
    x' = (s1/s0) x - a1 expm1(-h) D0 - 0.5 a1 expm1(-h) D1 (midpoint) | + a1 (expm1(-h)/h + 1) D1 (heun), D0 = m0, D1 = (m0 - m1) / r."""
    a0, s0, l0 = _alpha_s_lambda(sig[i])
    a1, s1, l1 = _alpha_s_lambda(sig[i + 1])
    if sig[i + 1] == 0.0:
        return 0.0, 1.0, 0.0
    h = l1 - l0
    c = -a1 * math.expm1(-h)
    if first:
        return s1 / s0, c, 0.0
    r = (l0 - _alpha_s_lambda(sig[i - 1])[2]) / h
    d1 = 0.5 * c if solver_type == "midpoint" else a1 * (math.expm1(-h) / h + 1.0)
    return s1 / s0, c + d1 / r, -d1 / r


class RefDPM(osched._SchedulerBase):
    """Torch restatement for the oracle pipeline: fp32 tensors, float64 scalars, the state machine of a multistep scheduler
    (the first `step` after `set_timesteps` is first order)."""

    def __init__(self, **cfg):
        super().__init__()
        self.cfg = dict(DEFAULTS, **cfg)

    def set_timesteps(self, n):
        c = self.cfg
        self.num_inference_steps = n
        ts = _ref_timesteps(c["timestep_spacing"], n, c["num_train_timesteps"], c["steps_offset"])
        self.timesteps = torch.from_numpy(ts.copy())
        self._sig = _ref_sigmas(self.alphas_cumprod.double().numpy(), ts, c["final_sigmas_type"])
        self._m1, self._start = None, None

    def step(self, model_output, timestep, sample, generator=None, variance_noise=None):
        i = int((self.timesteps == int(timestep)).nonzero()[0])
        if self._m1 is None:
            self._start = i
        a0, s0, _ = _alpha_s_lambda(self._sig[i])
        m0 = (sample - s0 * model_output) / a0
        first = _ref_first_order(self.cfg, i, self.num_inference_steps, self._start)
        k_x, k_x0, k_hist = _ref_coefs(self._sig, i, first, self.cfg["solver_type"])
        prev = k_x0 * m0 + k_x * sample
        if k_hist != 0.0:
            prev = prev + k_hist * self._m1
        self._m1 = m0
        return {"prev_sample": prev, "pred_original_sample": m0}


# ================================================================ A. kernel against float64
def _formula(x, e, m1, nz, c, k_hist, dtype):
    """The kernel's arithmetic in `dtype`; c: the eight fp32 coefficients of the row (exact in either dtype)."""
    x, e, m1, nz = (None if t is None else t.to(dtype) for t in (x, e, m1, nz))
    m0 = (x - c["sqrt_beta"] * e) / c["sqrt_alpha"]
    if c["clip"] >= 0:
        m0 = m0.clamp(-c["clip"], c["clip"])
    prev = c["k_x0"] * m0 + c["k_x"] * x
    if k_hist != 0:
        prev = prev + k_hist * m1
    if nz is not None and c["k_noise"] != 0:
        prev = prev + c["k_noise"] * nz
    return prev, m0


def _f32(v):
    return float(np.float32(v))


ROWS = [dict(sqrt_beta=_f32(0.91), sqrt_alpha=_f32(0.41), clip=-1.0, k_x0=_f32(0.23), k_x=_f32(0.87), k_eps=0.0, k_noise=0.0,
             timestep=900.0, k_hist=_f32(-0.11)),
        dict(sqrt_beta=_f32(0.62), sqrt_alpha=_f32(0.78), clip=-1.0, k_x0=_f32(0.57), k_x=_f32(0.49), k_eps=0.0, k_noise=0.0,
             timestep=500.0, k_hist=_f32(-0.31)),
        dict(sqrt_beta=_f32(0.35), sqrt_alpha=_f32(0.94), clip=1.0, k_x0=_f32(0.44), k_x=_f32(0.52), k_eps=0.0,
             k_noise=_f32(0.2), timestep=100.0, k_hist=_f32(-0.17))]
SHAPES = [(1, 1, 4, 4), (2, 1, 16, 16), (3, 2, 8, 12), (1, 1, 1032, 2048)]
# variant: (k_hist zero, out aliases x, u8, step from step_dev, mask, row)
PLAIN = dict(zero=True, alias=False, u8=False, dev=False, mask=False, row=0)
FULL = dict(zero=False, alias=True, u8=True, dev=True, mask=False, row=1)
ZERO_DEV = dict(zero=True, alias=True, u8=True, dev=True, mask=False, row=1)
HIST_IMM = dict(zero=False, alias=False, u8=False, dev=False, mask=False, row=0)
CLIP_NOISE = dict(zero=False, alias=False, u8=True, dev=False, mask=False, row=2)
MASK = dict(zero=False, alias=True, u8=True, dev=True, mask=True, row=1)
MASK_ZERO = dict(zero=True, alias=False, u8=False, dev=False, mask=True, row=2)
KCASES = []
for _s in SHAPES:
    _big = _s[2] > 1000
    for _name, _v in (("plain", PLAIN), ("full", FULL)) + (() if _big else (("zero-dev", ZERO_DEV), ("hist-imm", HIST_IMM),
                                                                           ("clip-noise", CLIP_NOISE))):
        KCASES.append(pytest.param(_s, _v, id="x".join(map(str, _s)) + "-" + _name))
    if _s[1] == 1 and not _big:
        KCASES.append(pytest.param(_s, MASK, id="x".join(map(str, _s)) + "-mask"))
        KCASES.append(pytest.param(_s, MASK_ZERO, id="x".join(map(str, _s)) + "-mask-zero"))


def _run_kernel(dev, shape, v, x, e, hist0, nz, mask):
    from audiodiffusion import ops
    table = ops.sched_coef_table(ROWS, dev)
    kh = torch.tensor([0.0 if v["zero"] else r["k_hist"] for r in ROWS], dtype=torch.float32).to(dev)
    xd, hist = x.clone().to(dev), hist0.clone().to(dev)
    B, C, H, W = shape
    u8 = torch.zeros((B, H * W * C), dtype=torch.uint8, device=dev) if v["u8"] else None
    step_dev = torch.tensor([v["row"]], dtype=torch.int32).to(dev) if v["dev"] else None
    out = ops.sched_multistep(xd, e.to(dev), table, kh, hist, -1 if v["dev"] else v["row"],
                              noise=None if nz is None else nz.to(dev), mask=None if mask is None else mask.to(dev),
                              mask_start=3 if v["mask"] else 0, mask_end=5 if v["mask"] else 0,
                              out=xd if v["alias"] else None, u8_out=u8, step_dev=step_dev)
    if not v["alias"]:
        assert torch.equal(xd.cpu(), x), "x was written although out does not alias it"
    return out.cpu(), hist.cpu(), None if u8 is None else u8.cpu()


@pytest.mark.parametrize("shape,v", KCASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_kernel_against_float64(backend, shape, v):
    dev = select(backend)
    B, C, H, W = shape
    x, e, m1 = _randn(shape, 1), _randn(shape, 2), _randn(shape, 3)
    nz = _randn(shape, 4) if v["row"] == 2 else None
    mask = _randn((B, len(ROWS), H, W), 5) if v["mask"] else None
    hist0 = torch.full(shape, float("nan")) if v["zero"] else m1
    c = ROWS[v["row"]]
    k_hist = 0.0 if v["zero"] else c["k_hist"]
    (ref64, m64), (ref32, m32) = (_formula(x, e, m1, nz, c, k_hist, dt) for dt in (torch.float64, torch.float32))
    if mask is not None:
        for r_ in (ref64, ref32):
            r_[..., :3] = mask[:, v["row"], None, :, :3].to(r_.dtype)
            r_[..., W - 5:] = mask[:, v["row"], None, :, W - 5:].to(r_.dtype)
    out, hist, u8 = _run_kernel(dev, shape, v, x, e, hist0, nz, mask)
    tag = f"backend={backend} shape={shape} variant={v}"
    _judge(tag, "out", out, ref64, ref32)
    _judge(tag, "hist", hist, m64, m32)          # (with a mask: the history is m0, not the masked value)
    if mask is not None:
        assert torch.equal(out[..., :3], mask[:, v["row"], None, :, :3]) and torch.equal(out[..., W - 5:], mask[:, v["row"], None, :, W - 5:])
        assert not torch.equal(hist[..., :3], out[..., :3])
    if u8 is not None:
        want = ((out / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).reshape(B, -1)
        assert torch.equal(u8, want), "u8 is not the half-to-even quantisation of the kernel's own float output"
    out2, hist2, u82 = _run_kernel(dev, shape, v, x, e, hist0, nz, mask)
    assert torch.equal(out, out2) and torch.equal(hist, hist2) and (u8 is None or torch.equal(u8, u82))


@pytest.mark.parametrize("backend", BACKENDS)
def test_sign_of_zero_tells_the_three_update_tails_apart(backend):
    """x = -0.0, eps = +0.0: x0 and k_x0*x0 + k_x*x are -0.0 (sums and products of zeros are exact, fused or not). The plain and the
    thresholded step then add k_eps*eps = +0.0 unconditionally, which gives +0.0; the multistep step has no k_eps term and skips the
    history (k_hist == 0) and the noise, so it keeps -0.0, in `out` and in `hist`, and never reads the NaN-filled history."""
    from audiodiffusion import ops
    dev = select(backend)
    shape = (1, 1, 4, 8)
    row = dict(sqrt_beta=_f32(0.6), sqrt_alpha=_f32(0.8), clip=-1.0, k_x0=_f32(0.9), k_x=_f32(0.3), k_eps=_f32(0.2), k_noise=0.0,
               timestep=0.0)
    table = ops.sched_coef_table([row], dev)
    x, e = torch.full(shape, -0.0).to(dev), torch.zeros(shape).to(dev)
    hist = torch.full(shape, float("nan")).to(dev)
    kh = torch.zeros((1,), dtype=torch.float32).to(dev)

    def bits(t):
        return t.cpu().view(torch.int32).flatten().tolist()

    n = x.numel()
    assert bits(x) == [-0x80000000] * n
    assert bits(ops.sched_step(x, e, table, 0)) == [0] * n
    assert bits(ops.sched_step(x, e, table, 0, threshold=(0.995, 2.0))) == [0] * n
    assert bits(ops.sched_multistep(x, e, table, kh, hist, 0)) == [-0x80000000] * n
    assert bits(hist) == [-0x80000000] * n


@pytest.mark.parametrize("backend", BACKENDS)
def test_kernel_bits_of_a_sample_do_not_depend_on_its_batch(backend):
    dev = select(backend)
    shape = (3, 2, 8, 12)
    x, e, m1 = _randn(shape, 1), _randn(shape, 2), _randn(shape, 3)
    out3, hist3, u83 = _run_kernel(dev, shape, FULL, x, e, m1, None, None)
    out1, hist1, u81 = _run_kernel(dev, (1,) + shape[1:], FULL, x[1:2].contiguous(), e[1:2].contiguous(), m1[1:2].contiguous(),
                                   None, None)
    assert torch.equal(out3[1:2], out1) and torch.equal(hist3[1:2], hist1) and torch.equal(u83[1:2], u81)


# ================================================================ B. tables
@pytest.mark.parametrize("spacing", ["linspace", "leading", "trailing"])
@pytest.mark.parametrize("N", [4, 15, 20])
def test_timesteps_follow_the_closed_forms(spacing, N):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(timestep_spacing=spacing, steps_offset=1 if spacing == "leading" else 0)
    s.set_timesteps(N)
    T = 1000
    if spacing == "linspace":
        want = np.linspace(0, T - 1, N + 1).round()[::-1][:-1]
    elif spacing == "leading":
        want = (np.arange(N + 1) * (T // (N + 1))).round()[::-1][:-1] + 1
    else:
        want = np.arange(T, 0, -T / N).round() - 1
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want.astype(np.int64).tolist()
    assert len(want) == N and want[0] > want[-1] >= 0 and want[0] <= T - 1


def _within_one_ulp(got, ref):
    return abs(float(np.float32(got)) - ref) <= float(np.spacing(np.float32(abs(ref))))


TABLE_CASES = [dict(N=4), dict(N=4, solver_type="heun"), dict(N=4, solver_order=1), dict(N=20), dict(N=20, solver_type="heun"),
               dict(N=15, final_sigmas_type="sigma_min"), dict(N=16, final_sigmas_type="sigma_min"),
               dict(N=16, final_sigmas_type="sigma_min", solver_type="heun"), dict(N=16, final_sigmas_type="sigma_min", solver_order=1),
               dict(N=4, final_sigmas_type="sigma_min"), dict(N=16, final_sigmas_type="sigma_min", euler_at_final=True),
               dict(N=10, final_sigmas_type="sigma_min", lower_order_final=False), dict(N=15, timestep_spacing="trailing"),
               dict(N=20, timestep_spacing="leading", steps_offset=1, solver_type="heun")]


@pytest.mark.parametrize("case", TABLE_CASES, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
@pytest.mark.parametrize("start", [0, 2])
def test_every_coefficient_is_within_one_ulp_of_the_float64_restatement(case, start):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    case = dict(case)
    N = case.pop("N")
    cfg = dict(DEFAULTS, **case)
    s = DPMSolverMultistepScheduler(**case)
    s.set_timesteps(N)
    rows = s.loop_rows(start, None)
    assert len(rows) == N - start
    ts = _ref_timesteps(cfg["timestep_spacing"], N, 1000, cfg["steps_offset"])
    sig = _ref_sigmas(s.alphas_cumprod.double().numpy(), ts, cfg["final_sigmas_type"])
    n_second = 0
    for j, row in enumerate(rows):
        i = start + j
        first = _ref_first_order(cfg, i, N, start)
        k_x, k_x0, k_hist = _ref_coefs(sig, i, first, cfg["solver_type"])
        a0, s0, _ = _alpha_s_lambda(sig[i])
        want = dict(sqrt_beta=s0, sqrt_alpha=a0, k_x0=k_x0, k_x=k_x, k_hist=k_hist)
        for k, w in want.items():
            assert _within_one_ulp(row[k], w), (i, k, row[k], w)
            assert row[k] == float(np.float32(row[k])), "rows hold the fp32 values the kernel reads"
        assert row["clip"] == -1.0 and row["k_eps"] == 0.0 and row["k_noise"] == 0.0 and row["timestep"] == float(ts[i])
        assert (row["k_hist"] == 0.0) == first
        n_second += not first
    assert rows[0]["k_hist"] == 0.0                                          # a run starts first order, wherever it starts
    if cfg["final_sigmas_type"] == "zero":
        assert (rows[-1]["k_x"], rows[-1]["k_x0"], rows[-1]["k_hist"]) == (0.0, 1.0, 0.0)
    if cfg["solver_order"] == 2:
        assert n_second >= 1 or start > 0
        if N == 16 and not cfg["euler_at_final"]:
            assert rows[-1]["k_hist"] != 0.0                                 # sigma_min at N >= 15: a second-order final row
        if N == 4 or cfg["euler_at_final"]:
            assert rows[-1]["k_hist"] == 0.0
    else:
        assert n_second == 0
    if start == 2:
        full = s.loop_rows(0, None)
        assert rows[1:] == full[3:] and (cfg["solver_order"] == 1 or rows[0] != full[2])
        assert s.loop_rows(2, 4) == rows[:2] and s.coef_rows() == full


# ================================================================ C. independent anchors
@pytest.mark.parametrize("backend", BACKENDS)
def test_order_one_is_the_ddim_update(backend):
    dev = select(backend)
    from audiodiffusion import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=1)
    N = 6
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


def _gaussian_error(dev, order, N, c=0.5):
    """max|x_N - exact| / max|exact| of `scheduler.step` on the model whose data distribution is N(0, c^2): eps*(x, t) =
    s_t x / (a_t^2 c^2 + s_t^2), and the probability-flow ODE keeps x / sqrt(a_t^2 c^2 + s_t^2) constant."""
    from audiodiffusion import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(solver_order=order, timestep_spacing="linspace", solver_type="midpoint", final_sigmas_type="zero")
    s.set_timesteps(N)
    acp = s.alphas_cumprod.double()
    x_T = _randn((1, 1, 4, 4), 7)
    x = x_T.to(dev)
    for t in s.timesteps:
        a2, s2 = float(acp[int(t)]), 1.0 - float(acp[int(t)])
        eps = (math.sqrt(s2) / (a2 * c * c + s2) * x.double()).float()
        x = s.step(eps, t, x).prev_sample
    a2, s2 = float(acp[int(s.timesteps[0])]), 1.0 - float(acp[int(s.timesteps[0])])
    exact = x_T.double() * math.sqrt(1.0 * c * c + 0.0) / math.sqrt(a2 * c * c + s2)
    return float((x.cpu().double() - exact).abs().max() / exact.abs().max())


@pytest.mark.parametrize("backend", BACKENDS)
def test_second_order_converges_faster_on_the_analytic_gaussian_model(backend):
    dev = select(backend)
    e1 = {N: _gaussian_error(dev, 1, N) for N in (10, 20, 40, 80)}
    e2 = {N: _gaussian_error(dev, 2, N) for N in (10, 20, 40)}
    print(f"DPMSOLVER backend={backend} gaussian first-order={e1} second-order={e2}")
    for N in (10, 20, 40):
        assert e2[N] < e1[N], (N, e1, e2)
    assert e2[20] < e1[40] and e2[40] < e1[80], (e1, e2)


# ================================================================ D. pipeline against the oracle pipeline
def _build(cfg=None, unet_cfg=TINY, cond=False):
    from audiodiffusion import AudioDiffusionPipeline, DPMSolverMultistepScheduler, Mel, UNet2DConditionModel, UNet2DModel
    torch.manual_seed(0)
    if cond:
        from oracle.unet_condition import UNet2DConditionModel as OracleCond
        ref_unet = OracleCond(**unet_cfg).eval()
        unet = UNet2DConditionModel(**unet_cfg).load_state_dict(ref_unet.state_dict())
    else:
        ref_unet = OracleUNet(**unet_cfg).eval()
        unet = UNet2DModel(**unet_cfg).load_state_dict(ref_unet.state_dict())
    ref = opipe.AudioDiffusionPipeline(None, ref_unet, omel.Mel(**MEL), RefDPM(**(cfg or {})))
    mine = AudioDiffusionPipeline(None, unet, Mel(**MEL), DPMSolverMultistepScheduler(**(cfg or {})))
    mine.set_progress_bar_config(disable=True)
    return ref, mine


def _cmp(mi, mf, ri, rf, scale=1.0):
    err = float((mf.cpu() - rf).abs().max())
    a = np.stack([np.asarray(i).astype(int) for i in mi])
    b = np.stack([np.asarray(i).astype(int) for i in ri])
    print(f"DPMSOLVER pipeline max|d|={err:.3e} lsb={np.abs(a - b).max()}")
    assert err <= 1e-3 * scale
    assert a.shape == b.shape and np.abs(a - b).max() <= 1


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,steps,cfg", [(2, 4, {}), (1, 16, dict(final_sigmas_type="sigma_min")), (2, 5, dict(solver_type="heun"))],
                         ids=["b2-steps4", "b1-steps16-sigma_min", "b2-steps5-heun"])
def test_sampling_matches_the_oracle_pipeline(backend, B, steps, cfg):
    dev = select(backend)
    ref, mine = _build(cfg)
    noise = _randn((B, 1, 16, 16), 42)
    ri, rf = ref(batch_size=B, steps=steps, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = mine(batch_size=B, steps=steps, noise=noise.clone().to(dev), audio=False, return_float=True)
    _cmp(mi, mf, ri, rf)
    assert mine.get_default_steps() == 20
    rows = mine.scheduler.loop_rows()
    # first-order start; with sigma 0 at the end a first-order final row as well, with sigma_min (N >= 15) a second-order one
    assert sum(r["k_hist"] != 0.0 for r in rows) == (steps - 1 if cfg.get("final_sigmas_type") == "sigma_min" else steps - 2)


@pytest.mark.parametrize("backend", BACKENDS)
def test_from_audio_late_start_and_mask(backend):
    dev = select(backend)
    ref, mine = _build()
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
    _cmp(mi, mf, ri, rf)


COND = dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 64),
            down_block_types=("CrossAttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "CrossAttnUpBlock2D"),
            cross_attention_dim=12, attention_head_dim=4)


@pytest.mark.parametrize("backend", BACKENDS)
def test_conditional_unet_in_the_multistep_loop(backend):
    dev = select(backend)
    ref, mine = _build(unet_cfg=COND, cond=True)
    noise, enc = _randn((2, 1, 16, 16), 42), _randn((2, 1, 12), 43)
    ri, rf = ref(batch_size=2, steps=4, noise=noise.clone(), encoding=enc, audio=False, return_float=True)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), encoding=enc.to(dev), audio=False, return_float=True)
    _cmp(mi, mf, ri, rf)


VAE_TINY = dict(sample_size=(32, 32), in_channels=1, out_channels=1, latent_channels=1, layers_per_block=1,
                block_out_channels=(32, 64), down_block_types=("DownEncoderBlock2D",) * 2, up_block_types=("UpDecoderBlock2D",) * 2)
MEL32 = dict(x_res=32, y_res=32, hop_length=64, n_fft=256, n_iter=2, sample_rate=4000)


@pytest.mark.parametrize("backend", BACKENDS)
def test_latent_pipeline_with_the_multistep_scheduler(backend):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, AutoencoderKL, DPMSolverMultistepScheduler, Mel, UNet2DModel
    from oracle.vae import AutoencoderKL as OracleVAE
    torch.manual_seed(0)
    ref_unet, ref_vae = OracleUNet(**TINY).eval(), OracleVAE(**VAE_TINY).eval()
    unet = UNet2DModel(**TINY).load_state_dict(ref_unet.state_dict())
    vae = AutoencoderKL(**VAE_TINY).load_state_dict(ref_vae.state_dict())
    ref = opipe.AudioDiffusionPipeline(ref_vae, ref_unet, omel.Mel(**MEL32), RefDPM())
    mine = AudioDiffusionPipeline(vae, unet, Mel(**MEL32), DPMSolverMultistepScheduler())
    mine.set_progress_bar_config(disable=True)
    noise = _randn((2, 1, 16, 16), 11)
    ri, rf = ref(batch_size=2, steps=4, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)
    assert rf.shape == mf.shape == (2, 1, 32, 32)
    _cmp(mi, mf, ri, rf, scale=max(1.0, float(rf.abs().max())))


@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_bit_identities(backend):
    dev = select(backend)
    from audiodiffusion import DDIMScheduler
    _, mine = _build()
    sched, n = mine.scheduler, 4
    x0 = _randn((3, 1, 16, 16), 9).to(dev)
    # the DDIM loop on this handle, before any multistep run
    mine.scheduler = DDIMScheduler()
    mine.scheduler.set_timesteps(n)
    ddim_before, _ = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    mine.scheduler = sched
    sched.set_timesteps(n)
    whole, u8 = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    # (1) one native loop == the same steps one by one through scheduler.step
    y = x0
    for k, t in enumerate(sched.timesteps):
        eps = mine.unet(y, t)["sample"]
        y = sched.step(eps, t, y).prev_sample
    assert torch.equal(whole, y)
    # (2) captured graph on / off, (3) a second call on the same model (the k_hist = 0 first row makes the stale history harmless)
    if backend != "emu":             # (the emulator has no graph: both settings are the same code there)
        eager, u8e = mine._denoise(x0, 0, 0.0, None, None, 0, 0, use_graph=False)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    again, u8a = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    assert torch.equal(whole, again) and torch.equal(u8, u8a)
    # (4) a sample's bits do not depend on its batch
    one, u81 = mine._denoise(x0[1:2].contiguous(), 0, 0.0, None, None, 0, 0)
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)
    # (5) a late start is the same run as the eager steps from there
    late, _ = mine._denoise(x0, 2, 0.0, None, None, 0, 0)
    sched.set_timesteps(n)
    y = x0
    for t in sched.timesteps[2:]:
        y = sched.step(mine.unet(y, t)["sample"], t, y).prev_sample
    assert torch.equal(late, y)
    # (6) the DDIM loop on the same handle is what it was
    mine.scheduler = DDIMScheduler()
    mine.scheduler.set_timesteps(n)
    ddim_after, _ = mine._denoise(x0, 0, 0.0, None, None, 0, 0)
    assert torch.equal(ddim_before, ddim_after)
    assert not torch.equal(ddim_before, whole)


# ================================================================ E. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_save_load_round_trip_keeps_the_class_and_samples_the_same(backend, tmp_path):
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, DPMSolverMultistepScheduler
    _, mine = _build(dict(solver_type="heun", final_sigmas_type="sigma_min", timestep_spacing="trailing"))
    mine.scheduler.save_pretrained(str(tmp_path / "s"))
    d = json.load(open(tmp_path / "s" / "scheduler_config.json"))
    assert d["_class_name"] == "DPMSolverMultistepScheduler" and d["solver_type"] == "heun" and d["lambda_min_clipped"] == -math.inf
    s2 = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path / "s"))
    assert dict(s2.config) == dict(mine.scheduler.config)
    mine.save_pretrained(str(tmp_path / "m"))
    index = json.load(open(tmp_path / "m" / "model_index.json"))
    assert index["scheduler"] == ["diffusers", "DPMSolverMultistepScheduler"]
    again = AudioDiffusionPipeline.from_pretrained(str(tmp_path / "m")).to(dev)
    again.set_progress_bar_config(disable=True)
    assert type(again.scheduler) is DPMSolverMultistepScheduler and dict(again.scheduler.config) == dict(mine.scheduler.config)
    assert again.get_default_steps() == 20
    noise = _randn((1, 1, 16, 16), 1)
    a = mine(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    b = again(steps=4, noise=noise.clone().to(dev), audio=False, return_float=True)[1]
    assert torch.equal(a, b)
    # the usual way in: from the config of the scheduler a checkpoint came with
    s3 = DPMSolverMultistepScheduler.from_config(DDIMScheduler().config)
    assert s3.config.timestep_spacing == "leading" and s3.config.solver_order == 2 and "clip_sample" not in s3.config
    assert s3.init_noise_sigma == 1.0 and s3.scale_model_input(noise) is noise
    x = s3.add_noise(noise.to(dev), noise.to(dev), torch.tensor([10]))
    assert x.shape == noise.shape


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_swapping_the_scheduler_of_a_loaded_checkpoint_samples_like_the_oracle(backend, kind, tmp_path):
    """a saved pipeline whose model_index.json names DDPMScheduler (or DDIMScheduler), loaded, then
    `pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)` and sampled."""
    dev = select(backend)
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler
    ref, mine = _build(dict(timestep_spacing="leading"))     # what the swapped config inherits from either scheduler
    mine.scheduler = DDPMScheduler() if kind == "ddpm" else DDIMScheduler()
    mine.save_pretrained(str(tmp_path / "ckpt"))
    assert json.load(open(tmp_path / "ckpt" / "model_index.json"))["scheduler"][1] == type(mine.scheduler).__name__
    pipe = AudioDiffusionPipeline.from_pretrained(str(tmp_path / "ckpt")).to(dev)
    pipe.set_progress_bar_config(disable=True)
    assert type(pipe.scheduler) is type(mine.scheduler) and pipe.get_default_steps() == (1000 if kind == "ddpm" else 50)
    if kind == "ddpm":
        assert pipe.scheduler.config.variance_type == "fixed_small"
    pipe.scheduler = DPMSolverMultistepScheduler.from_config(pipe.scheduler.config)
    pipe.save_pretrained(str(tmp_path / "swapped"))                             # the swapped scheduler is what is saved
    assert json.load(open(tmp_path / "swapped" / "model_index.json"))["scheduler"][1] == "DPMSolverMultistepScheduler"
    cfg = pipe.scheduler.config
    assert cfg.timestep_spacing == "leading" and cfg.solver_order == 2 and cfg.num_train_timesteps == 1000
    assert "clip_sample" not in cfg and "set_alpha_to_one" not in cfg
    assert pipe.get_default_steps() == 20
    noise = _randn((2, 1, 16, 16), 42)
    ri, rf = ref(batch_size=2, steps=5, noise=noise.clone(), audio=False, return_float=True)
    mi, mf = pipe(batch_size=2, steps=5, noise=noise.clone().to(dev), audio=False, return_float=True)
    _cmp(mi, mf, ri, rf)


@pytest.mark.parametrize("vt", [None, "fixed_small", "fixed_small_log", "fixed_large", "fixed_large_log"])
def test_fixed_variance_types_of_a_ddpm_config_are_accepted(vt):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    s, d = DPMSolverMultistepScheduler(variance_type=vt), DPMSolverMultistepScheduler()
    s.set_timesteps(4), d.set_timesteps(4)
    assert s.config.variance_type == vt and s.coef_rows() == d.coef_rows()      # the solver has no noise term: the key changes nothing


@pytest.mark.parametrize("cfg,N", [(dict(), 1000), (dict(), 1001), (dict(), 0), (dict(timestep_spacing="leading"), 1000),
                                   (dict(timestep_spacing="leading", steps_offset=150), 9),
                                   (dict(timestep_spacing="trailing", final_sigmas_type="sigma_min"), 700)],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_schedules_with_a_zero_length_row_are_rejected(cfg, N):
    """Repeated timesteps (N close to num_train_timesteps), timesteps out of range, or sigma_min reached before the final row:
    h = 0 on some row, which the second-order coefficients divide by. A ValueError at set_timesteps, and the state is kept."""
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(**cfg)
    s.set_timesteps(4)
    before = s.timesteps.clone()
    with pytest.raises(ValueError):
        s.set_timesteps(N)
    assert torch.equal(s.timesteps, before) and s.num_inference_steps == 4


@pytest.mark.parametrize("cfg,N", [(dict(), 999), (dict(solver_type="heun"), 999), (dict(timestep_spacing="leading"), 499),
                                   (dict(timestep_spacing="trailing"), 1000),
                                   (dict(timestep_spacing="trailing", final_sigmas_type="sigma_min", solver_type="heun"), 500)],
                         ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else str(v))
def test_the_longest_accepted_schedules_have_finite_rows(cfg, N):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    s = DPMSolverMultistepScheduler(**cfg)
    s.set_timesteps(N)
    rows = s.coef_rows()
    assert len(rows) == N and all(math.isfinite(v) for r in rows for v in r.values())
    assert sum(r["k_hist"] != 0.0 for r in rows) >= N - 2


@pytest.mark.parametrize("bad", [dict(solver_order=3), dict(algorithm_type="dpmsolver"), dict(algorithm_type="sde-dpmsolver++"),
                                 dict(algorithm_type="sde-dpmsolver"), dict(thresholding=True), dict(use_karras_sigmas=True),
                                 dict(use_lu_lambdas=True), dict(prediction_type="v_prediction"), dict(prediction_type="sample"),
                                 dict(variance_type="learned"), dict(variance_type="learned_range")],
                         ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_unsupported_config_raises_and_names_the_key(bad):
    select("emu")
    from audiodiffusion import DPMSolverMultistepScheduler
    with pytest.raises(NotImplementedError, match=next(iter(bad))):
        DPMSolverMultistepScheduler(**bad)
