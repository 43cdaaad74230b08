"""DDIM inversion for every model family the sampler runs: the inversion step of the three prediction types (`adm_encode_step`,
`ops.encode_step`), the loop (`adm_encode_loop_ex`: conditional models through the handle's encoding, wide samples through the windowed
step), the rows (`DDIMScheduler.encode_rows(level=...)`) and the front end (`AudioDiffusionPipeline.encode`) -- on the emulator and,
under `-m gpu`, on the MI355X. (`longform`: tests/test_inversion_longform.py.)

x is the sample at level s, o the model output, t the target level, c the level of the timestep the model was given; sa =
sqrt(alphas_cumprod), sb = sqrt(1 - alphas_cumprod):

    e  = o (epsilon)      e = (x - sa_c*o) / sb_c (sample)      e = sa_c*o + sb_c*x (v_prediction)
    x' = ((x - sb_s*e) * (1/sa_s)) * sa_t + sb_t*e
    level "reference": the model is given t, c = t.    level "matched": the model is given max(t_s, 0), c = alphas_cumprod there.

A. One step against that table in float64, the bar of tests/test_prediction_types.py (`_judge`): max|d| / max|ref| <= 8 * max(e_torch_fp32,
   4 * 2^-24); rows of both levels, the first row with final_alpha_cumprod = 1 and the zero-SNR last row included; the row read through
   the host index and through step_dev; one shape past the grid cap.
B. Anchors that do not rest on the recalled table: (i) epsilon through the new entry points has the bits of `adm_encode_loop`; (ii) three
   parameterisations of ONE model output agree within 8 * 2^-24 / min(sa_c, sb_c) of max|ref|; (iii) the point-mass model: a "matched"
   schedule driven with the exact model of a one-image distribution lands on the closed form sa_T*mu + sb_T*e0.
   Measured, B(iii), five steps, relative to max|ref|: the kernel against the float64 recurrence under "matched", and the bound (the sum
   over the steps of bar A, each from the torch-fp32 step on the float64 trajectory):
       MI355X    epsilon 3.5e-06 (9.5e-06)   sample 1.8e-06 (2.5e-05)   v_prediction 1.8e-07 (9.5e-06)
       emulator  epsilon 3.5e-06 (9.5e-06)   sample 1.8e-06 (2.5e-05)   v_prediction 2.1e-07 (9.5e-06)
   the float64 recurrence against the closed form: 6.5e-15, 2.6e-16, 3.9e-16; the same drive under "reference" ends 0.97, 1.00, 1.00 of
   max|ref| away from the closed form (recorded, not asserted: the reference's rule asks the model at the wrong level).
C. A sample's bits do not depend on its batch, for each type and for the windowed loop.
D. The loop: equal to the eager composition bit for bit; on the MI355X graph on equals graph off on a second handle; what keys the
   captured step; every field the entry point does not honour is refused by name.
E. `pipe.encode` against a test-local CPU restatement (oracle forwards + the table above in fp32), max|d| <= 1e-3 * max|ref|; then
   `pipe(noise=pipe.encode(...))` is accepted and its distance from the input is printed (profiles/inversion.md), not asserted.
F. The refusals of the front end, each before any native call.
"""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

import test_dpmsolver as td
import test_guidance as tg
import test_prediction_types as tp
import test_windowed as tw
import test_windowed_latent as twl
from native_backend import BACKENDS, select
from test_prediction_types import PRED, SHAPES, SID, U, _f32, _g, _judge, _randn, _same_bits

TYPES = ["epsilon", "sample", "v_prediction"]
LEVELS = ["reference", "matched"]
N_STEPS = 5
BIG = (3, 1, 1024, 1024)      # 786432 float4 > 2048 blocks * 256 lanes: the grid-stride loop turns over


def _table(pred, x, o, c, dtype):
    """The table of the module docstring in `dtype`; c: the fields of an inversion row (include/adm.h "DDIM inversion")."""
    x, o = x.to(dtype), o.to(dtype)
    sa_c, sb_c = c["k_x"], c["k_noise"]
    e = o if pred == 0 else ((x - sa_c * o) / sb_c if pred == 1 else sa_c * o + sb_c * x)
    return ((x - c["sqrt_beta"] * e) * c["sqrt_alpha"]) * c["k_x0"] + c["k_eps"] * e


def _scheduler(pred_name, zero_snr=None, **kw):
    """epsilon: the default schedule; the other two: trailing spacing on rescaled betas, so that the last row is the zero-SNR one."""
    from audiodiffusion import DDIMScheduler
    zero_snr = pred_name != "epsilon" if zero_snr is None else zero_snr
    cfg = dict(timestep_spacing="trailing", rescale_betas_zero_snr=True) if zero_snr else {}
    s = DDIMScheduler(prediction_type=pred_name, **cfg, **kw)
    s.set_timesteps(N_STEPS)
    return s


def _levels(sched, level):
    """Test-local restatement of the rows' levels, in float64: per row (acp_s, acp_t, acp_c, the timestep the model is given)."""
    ratio = sched.config.num_train_timesteps // sched.num_inference_steps
    acp = sched.alphas_cumprod.double()
    out = []
    for t in sorted(sched.timesteps.tolist()):
        ts = t - ratio
        tm = t if level == "reference" else max(ts, 0)
        out.append((float(acp[ts]) if ts >= 0 else float(sched.final_alpha_cumprod), float(acp[t]), float(acp[tm]), tm))
    return out


def _row_of(lv):
    a_s, a_t, a_c, tm = lv
    return dict(sqrt_beta=(1 - a_s) ** 0.5, sqrt_alpha=a_s ** -0.5, clip=-1.0, k_x0=a_t ** 0.5, k_x=a_c ** 0.5, k_eps=(1 - a_t) ** 0.5,
                k_noise=(1 - a_c) ** 0.5, timestep=float(tm))


def _encode_step(dev, pred, x, o, rows, row, step_dev=False):
    from audiodiffusion import ops
    table = ops.sched_coef_table(rows, dev)
    xd, od = x.clone().to(dev), o.to(dev)
    sd = torch.tensor([row], dtype=torch.int32).to(dev) if step_dev else None
    out = ops.encode_step(xd, od, table, -1 if step_dev else row, prediction=pred, step_dev=sd)
    assert out.data_ptr() == xd.data_ptr()
    assert torch.equal(od.cpu(), o), "the model output was written"
    return out.cpu()


# ================================================================ the rows
@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("pred_name", TYPES)
def test_rows_are_the_restated_levels(pred_name, level):
    select("emu")
    sched = _scheduler(pred_name)
    rows, want = sched.encode_rows(level), [_row_of(lv) for lv in _levels(sched, level)]
    assert len(rows) == N_STEPS
    for r, w in zip(rows, want):
        for k in tp.FIELDS:
            if pred_name == "epsilon" and k in ("k_x", "k_noise"):
                assert r[k] == 0.0                       # an epsilon row reads no conversion pair: the zeros it always had
            else:
                assert abs(r[k] - w[k]) <= 4 * U * max(1.0, abs(w[k])), (k, r[k], w[k])
        assert all(np.isfinite(r[k]) for k in tp.FIELDS)
    assert rows[0]["sqrt_beta"] == 0.0 and rows[0]["sqrt_alpha"] == 1.0          # final_alpha_cumprod = 1: x0 = x exactly
    if pred_name != "epsilon":
        assert rows[-1]["k_x0"] == 0.0 and rows[-1]["k_eps"] == 1.0              # the zero-SNR target
        assert (rows[-1]["k_x"] == 0.0) == (level == "reference")                # "reference" evaluates the model there: e = x
    assert [r["timestep"] for r in rows] == [float(lv[3]) for lv in _levels(sched, level)]


def test_reference_rows_of_an_epsilon_model_are_the_rows_they_were():
    """`encode_rows()` of the parent commit, restated: the bytes of an epsilon "reference" row do not move."""
    select("emu")
    for name in ("sample", "v_prediction"):          # no default rule for the other two: the refusal they always had
        with pytest.raises(NotImplementedError, match="prediction_type"):
            _scheduler(name).encode_rows()
    sched = _scheduler("epsilon")
    rows = []
    for t in torch.flip(sched.timesteps, (0,)).tolist():
        a_t, a_prev = sched.alphas_cumprod[t], sched._prev_acp(t)
        rows.append(dict(sqrt_beta=float((1 - a_prev) ** 0.5), sqrt_alpha=float(a_prev ** (-0.5)), clip=-1.0, k_x0=float(a_t ** 0.5),
                         k_x=0.0, k_eps=float((1 - a_t) ** 0.5), k_noise=0.0, timestep=float(t)))
    assert sched.encode_rows() == rows and sched.encode_rows("reference") == rows
    with pytest.raises(ValueError, match="level"):
        sched.encode_rows("current")


def test_inversion_stays_ddim_only_and_epsilon_stays_refused_at_zero_snr():
    select("emu")
    import audiodiffusion as ad
    for cls in (ad.DDPMScheduler, ad.DPMSolverMultistepScheduler, ad.UniPCMultistepScheduler):
        assert not hasattr(cls, "encode_rows")
    s = ad.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    with pytest.raises(ValueError, match="prediction_type"):
        s.set_timesteps(4)
    s = ad.DDIMScheduler(rescale_betas_zero_snr=True)
    s.set_timesteps(4)
    s.timesteps = torch.tensor([999, 500])
    with pytest.raises(ValueError, match="prediction_type"):
        s.encode_rows("matched")


# ================================================================ A. one step against the table in float64
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
@pytest.mark.parametrize("pred_name", TYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_step_against_float64(backend, pred_name, shape):
    dev = select(backend)
    pred, sched = PRED[pred_name], _scheduler(pred_name)
    x, o = 1.2 * _randn(shape, 1), _randn(shape, 2)
    for level in LEVELS:
        rows = sched.encode_rows(level)
        for row in (0, 2, N_STEPS - 1):      # the first row (sb_s = 0), one in the middle, the last (zero-SNR for sample / v)
            c = rows[row]
            ref64, ref32 = _table(pred, x, o, c, torch.float64), _table(pred, x, o, c, torch.float32)
            for step_dev in (False, True):
                out = _encode_step(dev, pred, x, o, rows, row, step_dev=step_dev)
                _judge(f"backend={backend} inversion type={pred_name} level={level} shape={shape} row={row} step_dev={step_dev}", "out", out,
                       ref64, ref32)


@pytest.mark.parametrize("pred_name", TYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_step_past_the_grid_cap(backend, pred_name):
    dev = select(backend)
    pred, sched = PRED[pred_name], _scheduler(pred_name)
    x, o = 1.2 * _randn(BIG, 1), _randn(BIG, 2)
    rows = sched.encode_rows("matched")
    ref64, ref32 = _table(pred, x, o, rows[2], torch.float64), _table(pred, x, o, rows[2], torch.float32)
    out = _encode_step(dev, pred, x, o, rows, 2)
    _judge(f"backend={backend} inversion type={pred_name} shape={BIG} row=2", "out", out, ref64, ref32)
    tail = slice(2048 * 256 * 4, None)       # what the second turn of the grid-stride loop wrote
    assert float((out.flatten()[tail].double() - ref64.flatten()[tail]).abs().max()) <= 8 * 4 * U * float(ref64.abs().max())


# ================================================================ B. anchors
def _tiny(pred_name="epsilon", **cfg):
    """(oracle pipeline, this package's pipeline) over the TINY weights of tests/test_prediction_types.py."""
    return tp._build("ddim", pred_name, **cfg)


def _coef(rows):
    from audiodiffusion import _native as N
    return (N.SchedCoef * len(rows))(*[N.SchedCoef(*[float(r[k]) for k in tp.FIELDS]) for r in rows])


def _loop(h, x, rows, pred, window=None, use_graph=1, symbol="adm_encode_loop_ex", **extra):
    """`adm_encode_loop_ex` on x IN PLACE. window: None or (stride, wrap), x is then the wide sample."""
    from audiodiffusion import _native as N
    a = N.SampleLoopArgs(x=N.ptr(x), B=x.shape[0], coef_host=_coef(rows), n_steps=len(rows), use_graph=int(use_graph), prediction=pred)
    if window is not None:
        a.window_total_w, a.window_stride, a.window_wrap = x.shape[3], window[0], int(window[1])
    for k, v in extra.items():
        setattr(a, k, N.ptr(v) if isinstance(v, torch.Tensor) else v)
    N.check(getattr(N.lib(), symbol)(h, a, N.stream_for(x)))
    return x


@pytest.mark.parametrize("backend", BACKENDS)
def test_epsilon_through_the_new_entry_points_has_the_old_bits(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    _, mine = _tiny()
    mine.scheduler.set_timesteps(3)
    rows = mine.scheduler.encode_rows()
    x0 = _randn((2, 1, 16, 16), 9).to(dev)
    h = mine.unet._ensure_handle()
    old = x0.clone()
    N.check(N.lib().adm_encode_loop(h, N.ptr(old), 2, _coef(rows), len(rows), 1, N.stream_for(old)))
    new = _loop(h, x0.clone(), rows, 0)
    assert _same_bits(old, new) and not torch.equal(old.cpu(), x0.cpu())
    # a conversion pair in an epsilon row is not read
    assert _same_bits(old, _loop(h, x0.clone(), [dict(r, k_x=0.3, k_noise=0.7) for r in rows], 0))


@pytest.mark.parametrize("sa", tp.SA_VALUES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_three_parameterisations_of_one_model_output_agree(backend, sa):
    dev = select(backend)
    sa_c = _f32(sa)
    sb_c = _f32(np.sqrt(1.0 - np.float64(sa_c) ** 2))
    x, e = 1.2 * _randn((2, 1, 16, 16), 7), _randn((2, 1, 16, 16), 1007)
    o_sample = (x.double() - sb_c * e.double()) / sa_c
    o_v = sa_c * e.double() - sb_c * o_sample
    row = dict(sqrt_beta=_f32(0.45), sqrt_alpha=_f32(1 / 0.89), clip=-1.0, k_x0=_f32(0.8), k_x=sa_c, k_eps=_f32(0.6), k_noise=sb_c, timestep=500.0)
    ref = _table(0, x, e, row, torch.float64)
    unit = U / min(sa_c, sb_c)
    for name, o in (("epsilon", e), ("sample", o_sample.float()), ("v_prediction", o_v.float())):
        out = _encode_step(dev, PRED[name], x, o, [row], 0)
        assert bool(torch.isfinite(out).all())
        ratio = _g(out, ref) / unit
        print(f"INVERSION backend={backend} one-output sa_c={sa_c} sb_c={sb_c} type={name} err={ratio:.3f} x 2^-24/min(sa_c,sb_c)")
        assert ratio <= 8.0, (name, sa_c, ratio)


def _point_mass_output(pred, x, mu, a_c):
    """The exact model of the distribution that is the single image mu, asked at level c, in float64: e = (x - sa_c*mu) / sb_c."""
    sa_c, sb_c = a_c ** 0.5, (1 - a_c) ** 0.5
    e = (x - sa_c * mu) / sb_c
    return e if pred == 0 else (mu if pred == 1 else sa_c * e - sb_c * mu)


@pytest.mark.parametrize("pred_name", TYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_point_mass_model_lands_on_the_closed_form(backend, pred_name):
    """DDIM trajectories of a one-image distribution are sa*mu + sb*e0 with a constant e0. The schedule starts at alphas_cumprod[0]
    (set_alpha_to_one=False), where the first "matched" row asks the model at the sample's own level exactly."""
    dev = select(backend)
    from audiodiffusion import ops
    pred = PRED[pred_name]
    sched = _scheduler(pred_name, set_alpha_to_one=False)
    mu, e0 = 0.7 * _randn((2, 1, 16, 16), 3).double(), _randn((2, 1, 16, 16), 4).double()
    a_first, a_last = _levels(sched, "matched")[0][0], _levels(sched, "matched")[-1][1]
    start = (a_first ** 0.5 * mu + (1 - a_first) ** 0.5 * e0).float()
    e0 = (start.double() - a_first ** 0.5 * mu) / (1 - a_first) ** 0.5          # the e0 of the fp32 start
    closed = a_last ** 0.5 * mu + (1 - a_last) ** 0.5 * e0
    dist = {}
    for level in LEVELS:
        lvs, rows = _levels(sched, level), sched.encode_rows(level)
        table = ops.sched_coef_table(rows, dev)
        x64, xk, bound = start.double(), start.clone().to(dev), 0.0
        for i, lv in enumerate(lvs):
            c64 = _row_of(lv)
            # bar A of this step, from the float64 trajectory: the torch-fp32 step against the float64 step
            o = _point_mass_output(pred, x64, mu, lv[2])
            nxt = _table(pred, x64, o, c64, torch.float64)
            e_torch = _g(_table(pred, x64.float(), o.float(), rows[i], torch.float32), nxt)
            bound += 8 * max(e_torch, 4 * U)
            x64 = nxt
            ok = _point_mass_output(pred, xk.cpu().double(), mu, lv[2]).float().to(dev)      # the model's answer to the kernel's own x
            ops.encode_step(xk, ok, table, i, prediction=pred)
        dist[level] = _g(x64, closed)
        err = _g(xk.cpu(), x64)
        print(f"INVERSION backend={backend} point-mass type={pred_name} level={level} steps={len(lvs)} float64-vs-closed={dist[level]:.3e} "
              f"kernel-vs-float64={err:.3e} bound(sum of bar A)={bound:.3e}")
        assert bool(torch.isfinite(xk).all())
        if level == "matched":
            assert dist[level] <= 1e-10
            assert err <= bound
    assert dist["reference"] > 1e-3        # (recorded above, not a bar: the reference's rule does not reach the closed form)


# ================================================================ C. batch independence
WINDOWS = [None, (8, False), (8, True)]
WID = lambda w: "model-width" if w is None else f"wide-{w[0]}-{'circular' if w[1] else 'open'}"  # noqa: E731


@pytest.mark.parametrize("window", WINDOWS, ids=WID)
@pytest.mark.parametrize("pred_name", TYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_bits_of_a_sample_do_not_depend_on_its_batch(backend, pred_name, window):
    dev = select(backend)
    _, mine = _tiny(pred_name)
    sched = _scheduler(pred_name)
    rows = sched.encode_rows("matched")[:3]
    x = _randn((2, 1, 16, 16 if window is None else 32), 11)
    x[1] *= 30.0
    h = mine.unet._ensure_handle()
    two = _loop(h, x.clone().to(dev), rows, PRED[pred_name], window)
    one = _loop(h, x[:1].clone().to(dev), rows, PRED[pred_name], window)
    assert bool(torch.isfinite(two).all()) and _same_bits(two[:1], one)


# ================================================================ D. the loop
def _eager(mine, x, rows, pred, window=None, encoding=None):
    """The composition of the public pieces: gather, forward, blend, `ops.encode_step`."""
    from audiodiffusion import ops
    table = ops.sched_coef_table(rows, x.device)
    x = x.clone()
    for i, r in enumerate(rows):
        fx = x if window is None else ops.window_gather(x, 16, window[0], window[1])
        args = (fx, r["timestep"]) if encoding is None else (fx, r["timestep"], encoding.repeat_interleave(fx.shape[0] // x.shape[0], dim=0))
        o = mine.unet(*args)["sample"]
        if window is not None:
            o = ops.window_blend(o, x.shape[3], window[0], window[1])
        ops.encode_step(x, o, table, i, prediction=pred)
    return x


@pytest.mark.parametrize("window", WINDOWS, ids=WID)
@pytest.mark.parametrize("pred_name", TYPES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_equals_the_eager_composition(backend, pred_name, window):
    dev = select(backend)
    _, mine = _tiny(pred_name)
    rows = _scheduler(pred_name).encode_rows("matched")[:3]
    x0 = _randn((2, 1, 16, 16 if window is None else 32), 12).to(dev)
    whole = _loop(mine.unet._ensure_handle(), x0.clone(), rows, PRED[pred_name], window)
    assert _same_bits(whole, _eager(mine, x0, rows, PRED[pred_name], window))
    assert not torch.equal(whole, _loop(mine.unet._ensure_handle(), x0.clone(), rows, (PRED[pred_name] + 1) % 3, window))


@pytest.mark.parametrize("backend", BACKENDS)
def test_conditional_loop_equals_the_eager_composition(backend):
    dev = select(backend)
    _, mine = tg._build("ddim", prediction_type="v_prediction")
    mine.scheduler.set_timesteps(3)
    rows = mine.scheduler.encode_rows("matched")
    x0, enc = _randn((2, 1, 16, 16), 13).to(dev), _randn((2, 1, 12), 14).to(dev)
    for window in (None, (8, False)):
        xs = x0 if window is None else _randn((2, 1, 16, 32), 15).to(dev)
        nW = 1 if window is None else 3
        h = mine.unet._ensure_handle()
        mine.unet._set_encoding(h, enc.repeat_interleave(nW, dim=0), 2 * nW, dev)
        whole = _loop(h, xs.clone(), rows, 2, window)
        assert _same_bits(whole, _eager(mine, xs, rows, 2, window, encoding=enc))
    other = _randn((2, 1, 12), 16).to(dev)
    mine.unet._set_encoding(h, other.repeat_interleave(3, dim=0), 6, dev)
    assert not torch.equal(whole, _loop(h, xs.clone(), rows, 2, window)), "the encoding changed nothing"


def _captures(h):
    from audiodiffusion import _native as N
    return N.lib().adm_unet_loop_captures(h)


@pytest.mark.parametrize("backend", BACKENDS)
def test_what_keys_the_captured_inversion_step(backend):
    """ONE handle, one x and one wide x refilled in place; per call by how much the capture counter went up (the contract of
    tests/test_loop_graph_key.py), and on the MI355X the bits of the same call with use_graph=0 on a second handle."""
    dev = select(backend)
    from audiodiffusion import UNet2DModel
    _, mine = _tiny("v_prediction")
    second = UNet2DModel(**tp.TINY).load_state_dict(mine.unet.state_dict()) if dev.type == "cuda" else None
    sched = _scheduler("v_prediction")
    ref_rows, matched_rows = sched.encode_rows("reference")[:2], sched.encode_rows("matched")[:2]
    sched.set_timesteps(2)
    sample_rows = sched.coef_rows(0.0)
    h = mine.unet._ensure_handle()
    x, wide = torch.empty((2, 1, 16, 16), device=dev), torch.empty((2, 1, 16, 32), device=dev)
    state = {"n": _captures(h)}

    def call(buf, seed, rows, pred, window=None, symbol="adm_encode_loop_ex"):
        src = _randn(buf.shape, seed)
        buf.copy_(src)
        got = _loop(h, buf, rows, pred, window, symbol=symbol).clone()
        if second is not None:
            assert _same_bits(got, _loop(second._ensure_handle(), src.clone().to(dev), rows, pred, window, use_graph=0, symbol=symbol))
        assert bool(torch.isfinite(got).all())
        n, state["n"] = state["n"], _captures(h)
        return state["n"] - n

    assert call(x, 1, ref_rows, 2) == 1
    assert call(x, 1, ref_rows, 2) == 0                                 # the same call
    assert call(x, 2, ref_rows, 2) == 0                                 # new contents at the same address
    assert call(x, 2, matched_rows, 2) == 0                             # new table values at the same n_steps: a switch of level
    assert call(x, 2, matched_rows, 1) == 1                             # another prediction
    assert call(x, 2, matched_rows, 2) == 1                             # ... and back
    assert call(wide, 3, matched_rows, 2, (8, False)) == 1              # a window placement
    assert call(wide, 3, matched_rows, 2, (8, True)) == 1               # another placement
    assert call(x, 2, matched_rows, 2) == 1                             # ... and back
    assert call(x, 4, sample_rows, 2, symbol="adm_sample_loop_ex") == 1   # a sampling loop on the same handle
    assert call(x, 2, matched_rows, 2) == 1                             # ... and the inversion again


REFUSED = ["mode", "k_hist_host", "unipc_host", "step_noise", "noise_source", "seed", "row_offset", "mask", "mask_start", "mask_end", "u8_out",
           "lo", "hi", "w", "max_value", "encoding_uncond", "guidance_scale", "guidance_rescale", "keep", "known", "known_noise",
           "known_coef_host", "known_batched", "keep_batched"]


@pytest.mark.parametrize("field", REFUSED)
@pytest.mark.parametrize("backend", BACKENDS)
def test_a_field_the_inversion_loop_does_not_honour_is_refused_by_name(backend, field):
    dev = select(backend)
    from audiodiffusion import _native as N
    _, mine = _tiny()
    mine.scheduler.set_timesteps(2)
    rows = mine.scheduler.encode_rows()
    x = _randn((1, 1, 16, 16), 5).to(dev)
    keep = x.clone()
    other = torch.zeros((1, 1, 16, 16), device=dev)
    value = {"mode": 1, "k_hist_host": (C.c_float * 2)(), "unipc_host": (N.SchedUnipcCoef * 2)(), "known_coef_host": (C.c_float * 4)(),
             "seed": 7, "w": 0.5, "max_value": 1.0, "guidance_scale": 1.0, "guidance_rescale": 0.5,
             "u8_out": torch.zeros((1, 16, 16, 1), dtype=torch.uint8, device=dev),
             "keep": torch.zeros((1, 16, 16), dtype=torch.uint8, device=dev)}.get(field)
    if value is None:
        value = other if field in ("step_noise", "mask", "encoding_uncond", "known", "known_noise") else 1
    h = mine.unet._ensure_handle()
    before = _captures(h)
    with pytest.raises(N.NativeError, match=rf"encode_loop: {field} "):
        _loop(h, x, rows, 0, **{field: value})
    assert torch.equal(x, keep) and _captures(h) == before, "refused after work was done"
    if field == "mode":      # the multistep mode as well; and the sampling entry point has no inversion mode
        with pytest.raises(N.NativeError, match="encode_loop: mode "):
            _loop(h, x, rows, 0, mode=2)
        with pytest.raises(N.NativeError, match="sample_loop: mode "):
            _loop(h, x, rows, 0, symbol="adm_sample_loop_ex", mode=-1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_version_and_argument_checks(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    assert N.lib().adm_version() >= 123
    _, mine = _tiny()
    mine.scheduler.set_timesteps(2)
    rows = mine.scheduler.encode_rows()
    h = mine.unet._ensure_handle()
    x = _randn((1, 1, 16, 16), 5).to(dev)
    for bad in (-1, 3):
        with pytest.raises(N.NativeError, match="prediction"):
            _loop(h, x, rows, bad)
        with pytest.raises(N.NativeError, match="prediction"):
            ops.encode_step(x, x.clone(), ops.sched_coef_table(rows, dev), 0, prediction=bad)
    wide = _randn((1, 1, 16, 32), 6).to(dev)
    for window, word in (((12, False), "window_stride"), ((6, False), "window_stride"), ((12, True), "window_total_w")):
        with pytest.raises(N.NativeError, match=word):
            _loop(h, wide, rows, 0, window)
    table = ops.sched_coef_table(rows, dev)
    six = torch.zeros((6,), device=dev)
    assert N.lib().adm_encode_step(N.ptr(six), N.ptr(six), N.ptr(table), None, 0, 0, 6, N.stream_for(six)) != 0      # n % 4
    assert N.lib().adm_encode_step(N.ptr(x), None, N.ptr(table), None, 0, 0, 256, N.stream_for(x)) != 0
    assert N.lib().adm_encode_step(N.ptr(x), N.ptr(x), N.ptr(table), None, -1, 0, 256, N.stream_for(x)) != 0        # no row


# ================================================================ E. the pipeline against the oracle
def _images(B, H, W, seed):
    rng = np.random.default_rng(seed)
    return [Image.fromarray(rng.integers(0, 256, (H, W), dtype=np.uint8)) for _ in range(B)]


def _to_tensor(images):
    a = np.stack([np.asarray(i) for i in images])[:, None].astype(np.float64)
    return torch.from_numpy(a / 255 * 2 - 1).float()


def _ref_invert(forward, x, sched, level, pred, window=None):
    """The inversion on the CPU in fp32: `forward(x, timestep)` is an oracle forward; window: None or (stride, wrap) at model width 16."""
    for lv in _levels(sched, level):
        if window is None:
            o = forward(x, lv[3])
        else:
            win = torch.from_numpy(tw._np_gather(x.numpy(), 16, window[0], window[1]))
            o = torch.from_numpy(tw._np_blend(forward(win, lv[3]).numpy(), x.shape[3], window[0], window[1])[0])
        x = _table(pred, x, o, _row_of(lv), torch.float32)
    return x


def _cmp(tag, got, want):
    got = got.cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all())
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f"INVERSION pipeline {tag} max|d|={err:.3e} max|ref|={scale:.3f}")
    assert err <= 1e-3 * scale


def _round_trip(tag, mine, noise, target, steps, **call):
    """`pipe(noise=pipe.encode(...))` is accepted; its distance from the input is a record for profiles/inversion.md, not a bar."""
    images, floats = mine(batch_size=noise.shape[0], noise=noise, steps=steps, eta=0, audio=False, return_float=True, **call)
    assert len(images) == noise.shape[0] and tuple(floats.shape) == tuple(target.shape) and bool(torch.isfinite(floats).all())
    print(f"INVERSION round-trip {tag} max|image - input|={float((floats.cpu() - target).abs().max()):.3f} "
          f"rms={float((floats.cpu() - target).pow(2).mean().sqrt()):.3f}")


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("pred_name", ["sample", "v_prediction"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_of_the_other_prediction_types_matches_the_restatement(backend, pred_name, level):
    dev = select(backend)
    ref, mine = _tiny(pred_name)
    mine.to(dev)
    images = _images(2, 16, 16, 1)
    got = mine.encode(images, steps=4, level=level)
    with torch.no_grad():
        want = _ref_invert(lambda x, t: ref.unet(x, t)["sample"], _to_tensor(images), mine.scheduler, level, PRED[pred_name])
    tag = f"backend={backend} type={pred_name} level={level}"
    _cmp(tag, got, want)
    with torch.no_grad():
        other = _ref_invert(lambda x, t: ref.unet(x, t)["sample"], _to_tensor(images), mine.scheduler, "reference",
                            PRED[pred_name]) if level == "matched" else None
    assert other is None or float((other.detach() - want).abs().max()) > 1e-2 * float(want.abs().max()), "the two levels are one here"
    _round_trip(tag, mine, got, _to_tensor(images), 4)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_on_a_zero_snr_schedule(backend, level):
    """v_prediction on rescaled betas with trailing spacing: both levels are finite; "matched" matches its restatement."""
    dev = select(backend)
    ref, mine = _tiny("v_prediction", rescale_betas_zero_snr=True, timestep_spacing="trailing")
    mine.to(dev)
    images = _images(2, 16, 16, 2)
    got = mine.encode(images, steps=4, level=level)
    assert mine.scheduler.timesteps[0] == 999
    with torch.no_grad():
        want = _ref_invert(lambda x, t: ref.unet(x, t)["sample"], _to_tensor(images), mine.scheduler, level, 2)
    tag = f"backend={backend} type=v_prediction zero-snr level={level}"
    _cmp(tag, got, want)
    _round_trip(tag, mine, got, _to_tensor(images), 4)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_of_a_conditional_model_matches_the_restatement(backend, level):
    dev = select(backend)
    ref, mine = tg._build("ddim")
    mine.to(dev)
    images, enc = _images(2, 16, 16, 3), _randn((2, 1, 12), 43)
    got = mine.encode(images, steps=3, level=level, encoding=enc.to(dev))
    with torch.no_grad():
        want = _ref_invert(lambda x, t: ref.unet(x, t, enc)["sample"], _to_tensor(images), mine.scheduler, level, 0)
        none = _ref_invert(lambda x, t: ref.unet(x, t, torch.zeros_like(enc))["sample"], _to_tensor(images), mine.scheduler, level, 0)
    tag = f"backend={backend} conditional level={level}"
    _cmp(tag, got, want)
    assert float((none - want).abs().max()) > 1e-3 * float(want.abs().max()), "the encoding changes nothing here"
    if level == "matched":
        one = mine.encode(images, steps=3, level=level, encoding=enc[:1].to(dev))                # (1, S, D) is broadcast
        assert _same_bits(one, mine.encode(images, steps=3, level=level, encoding=enc[:1].expand(2, -1, -1).contiguous().to(dev)))
    _round_trip(tag, mine, got, _to_tensor(images), 3, encoding=enc.to(dev))


_LATENT = {}


def _latent(dev, pred_name="epsilon"):
    """(oracle UNet, oracle VAE, the latent pipeline): the tiny VAE of tests/test_windowed_latent.py over the 16 x 16 TINY UNet."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    from oracle.unet import UNet2DModel as OracleUNet
    if "unet" not in _LATENT:
        torch.manual_seed(0)
        _LATENT["unet"] = OracleUNet(**td.TINY).eval()
    ref_vae, vae = twl._vae()
    unet = UNet2DModel(**td.TINY).load_state_dict(_LATENT["unet"].state_dict())
    mine = AudioDiffusionPipeline(vae, unet, Mel(**td.MEL32), DDIMScheduler(prediction_type=pred_name)).to(dev)
    mine.set_progress_bar_config(disable=True)
    return _LATENT["unet"], ref_vae, mine


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("draw", ["mode", "generator"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_of_a_latent_pipeline_matches_the_restatement(backend, level, draw):
    dev = select(backend)
    ref_unet, ref_vae, mine = _latent(dev)
    images = _images(2, 32, 32, 4)
    gen = None if draw == "mode" else torch.Generator().manual_seed(5)
    got = mine.encode(images, steps=3, level=level, generator=gen)
    with torch.no_grad():
        dist = ref_vae.encode(_to_tensor(images)).latent_dist
        z = 0.18215 * (dist.mode() if gen is None else dist.sample(generator=torch.Generator().manual_seed(5)))
        want = _ref_invert(lambda x, t: ref_unet(x, t)["sample"], z, mine.scheduler, level, 0)
    assert tuple(got.shape) == (2, 1, 16, 16)
    tag = f"backend={backend} latent draw={draw} level={level}"
    _cmp(tag, got, want)
    if gen is None:
        assert _same_bits(got, mine.encode(images, steps=3, level=level)), "the mode is deterministic"
    _round_trip(tag, mine, got, _to_tensor(images), 3)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("circular", [False, True], ids=["open-3-windows", "circular-4-windows"])
@pytest.mark.parametrize("pred_name", ["epsilon", "v_prediction"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_of_a_wide_image_matches_the_restatement(backend, level, pred_name, circular):
    dev = select(backend)
    ref, mine = _tiny(pred_name)
    mine.to(dev)
    images = _images(2, 16, 32, 6)
    got = mine.encode(images, steps=3, level=level, window_stride=8, circular=circular)
    assert tuple(got.shape) == (2, 1, 16, 32) and tuple(mine.unet._hw()) == (16, 16)
    with torch.no_grad():
        want = _ref_invert(lambda x, t: ref.unet(x, t)["sample"], _to_tensor(images), mine.scheduler, level, PRED[pred_name], (8, circular))
    tag = f"backend={backend} wide type={pred_name} circular={circular} level={level}"
    _cmp(tag, got, want)
    if not circular and level == "matched":
        assert _same_bits(got, mine.encode(images, steps=3, level=level)), "the default stride is W // 2"
    _round_trip(tag, mine, got, _to_tensor(images), 3, frames=32, window_stride=8, circular=circular)


@pytest.mark.parametrize("level", LEVELS)
@pytest.mark.parametrize("circular", [False, True], ids=["open", "circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_of_a_wide_image_in_a_latent_pipeline_matches_the_restatement(backend, level, circular):
    dev = select(backend)
    ref_unet, ref_vae, mine = _latent(dev)
    images = _images(2, 32, 64, 7)
    x = _to_tensor(images)
    with torch.no_grad():
        d = ref_vae.encode(torch.from_numpy(tw._np_gather(x.numpy(), 32, 16, circular))).latent_dist
        z = 0.18215 * torch.from_numpy(twl._crossfade64(d.mean, 32, 8, circular)).float()
    got = mine.encode(images, steps=3, level=level, window_stride=8, circular=circular)
    assert tuple(got.shape) == (2, 1, 16, 32)
    with torch.no_grad():
        want = _ref_invert(lambda x_, t: ref_unet(x_, t)["sample"], z, mine.scheduler, level, 0, (8, circular))
    tag = f"backend={backend} wide latent circular={circular} level={level}"
    _cmp(tag, got, want)
    _round_trip(tag, mine, got, x, 3, frames=32, window_stride=8, circular=circular)


# ================================================================ F. the refusals of the front end
def _spy_native(monkeypatch):
    """-> a list that gains the name of every native entry point the code under test fetches (`adm_last_error` aside)."""
    from audiodiffusion import _native
    real, calls = _native.lib(), []

    class Spy:
        def __getattr__(self, name):
            if name.startswith("adm_") and name != "adm_last_error":
                calls.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_native, "lib", lambda: Spy())
    return calls


@pytest.mark.parametrize("backend", BACKENDS)
def test_every_rule_is_checked_before_any_native_call(backend, monkeypatch):
    dev = select(backend)
    import audiodiffusion as ad
    _, plain = _tiny()
    _, vpipe = _tiny("v_prediction")
    _, cond = tg._build("ddim")
    _, _, latent = _latent(dev)
    plain.to(dev), cond.to(dev)
    enc = _randn((2, 1, 12), 1).to(dev)
    img, wide, tall = _images(2, 16, 16, 1), _images(2, 16, 32, 2), _images(2, 32, 32, 3)
    calls = _spy_native(monkeypatch)
    cases = [
        (plain, img, dict(level="current"), ValueError, "level"),
        (vpipe, img, dict(level="current"), ValueError, "level"),
        (vpipe, img, dict(), NotImplementedError, "prediction_type.*level"),      # no default rule for a sample / v model
        (plain, img, dict(encoding=enc), ValueError, "encoding"),
        (cond, img, dict(), ValueError, "encoding"),
        (cond, img, dict(encoding=_randn((3, 1, 12), 2).to(dev)), ValueError, "encoding shape"),
        (cond, img, dict(encoding=_randn((2, 1, 8), 2).to(dev)), ValueError, "encoding shape"),
        (plain, img, dict(window_stride=8), ValueError, "window_stride.*frames"),
        (plain, img, dict(circular=True), ValueError, "circular.*frames"),
        (plain, wide, dict(window_stride=12), ValueError, "window_stride"),
        (plain, wide, dict(window_stride=6), ValueError, "window_stride"),
        (plain, wide, dict(window_stride=12, circular=True), ValueError, "frames"),
        (plain, tall, dict(), ValueError, "height"),
        (latent, _images(1, 32, 64, 4), dict(window_stride=12), ValueError, "window_stride"),
        (latent, _images(1, 31, 32, 4), dict(), ValueError, "latent cells"),
    ]
    for pipe, images, kw, exc, word in cases:
        pipe.unet.sample_size = (16, 16)
        with pytest.raises(exc, match=word):
            pipe.encode(images, steps=3, **kw)
    plain.scheduler = ad.DDIMScheduler(rescale_betas_zero_snr=True, timestep_spacing="trailing")
    with pytest.raises(ValueError, match="prediction_type"):
        plain.encode(img, steps=3)
    for cls in (ad.DDPMScheduler, ad.DPMSolverMultistepScheduler, ad.UniPCMultistepScheduler):
        plain.scheduler = cls()
        with pytest.raises(AssertionError):
            plain.encode(img, steps=3)
    assert calls == [], calls
    assert tuple(vpipe.encode(img, steps=2, level="reference").shape) == (2, 1, 16, 16) and "adm_encode_loop_ex" in calls
