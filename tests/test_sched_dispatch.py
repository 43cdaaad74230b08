"""The scheduler's struct-argument entry points (`adm_sched_step_ex`, `adm_sched_threshold_ex`, `adm_sample_loop_ex`; adm_version() >= 114)
against the frozen positional ones, on the emulator and, under `-m gpu`, on the MI355X. No tolerance anywhere: both sides run the same
kernels, so every comparison is of bits.

A. Each of the 26 step kernels (mode x prediction x guided x noise stream): `ops.*`, which builds `adm_sched_step_args` in Python, gives
   the bits of the positional symbol for that combination called directly: in out, u8_out, scale and hist. This pins the ctypes layout of
   the struct against the C one field by field: every field decides the result of at least one combination.
B. Every combination that is not built, and every value out of range, is refused with a message that says why.
C. `adm_sample_loop_ex` gives the bits of each of the six positional loops, alternating with them on one handle (captured-graph reuse).
"""
import ctypes as C

import pytest
import torch

import sched_kernels
import test_guidance as tg
import test_prediction_types as tp
from native_backend import BACKENDS, select

PLAIN, THRESH, MULTISTEP = 0, 1, 2
COMBOS = sorted(sched_kernels.STEP_KERNELS)          # (mode, pred, guided, philox): the 26 that are built
SHAPE = (2, 1, 4, 8)                                 # 8 float4 per sample, two samples: the scale index, the noise-stream row and the mask
                                                     # row all take two values
STEP, N_MASK = 1, 3                                  # tg.ROWS[1]: k_noise != 0 and k_hist != 0; a mask of three steps
RATIO, MAX_VALUE, GUIDANCE, SEED, ROW_OFFSET = 0.9, 4.0, 2.5, 0x1234_5678_9ABC_DEF0, 5


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _inputs(dev, combo):
    mode, pred, guided, philox = combo
    t = {k: (0.75 * _randn(SHAPE, s)).to(dev) for s, k in enumerate(("x", "eps", "uncond", "noise", "hist"))}
    t["mask"] = _randn((SHAPE[0], N_MASK, SHAPE[2], SHAPE[3]), 7).to(dev)
    t["step_dev"] = torch.tensor([STEP], dtype=torch.int32).to(dev) if guided else None   # guided: the row comes from the device scalar
    t["step"] = 0 if guided else STEP
    t["alias"] = pred == 1                                                                  # the sample-prediction kernels write out over x
    return t


def _outputs(dev, t):
    out = t["x"] if t["alias"] else torch.zeros(SHAPE, device=dev)
    return out, torch.zeros((SHAPE[0], SHAPE[2] * SHAPE[3]), dtype=torch.uint8, device=dev), torch.zeros(SHAPE[0], device=dev)


def _through_ops(dev, combo, table, khist):
    from audiodiffusion import ops
    mode, pred, guided, philox = combo
    t = _inputs(dev, combo)
    out, u8, scale = _outputs(dev, t)
    kw = dict(noise=None if philox else t["noise"], mask=t["mask"], mask_start=1, mask_end=1, out=out, u8_out=u8, step_dev=t["step_dev"],
              uncond=t["uncond"] if guided else None, guidance_scale=GUIDANCE if guided else None)
    if mode == MULTISTEP:
        ops.sched_multistep(t["x"], t["eps"], table, khist, t["hist"], t["step"], **kw)
    else:
        ops.sched_step(t["x"], t["eps"], table, t["step"], threshold=(RATIO, MAX_VALUE) if mode == THRESH else None, scale_out=scale,
                       prediction=pred, noise_seed=SEED if philox else None, noise_row_offset=ROW_OFFSET, **kw)
    return out, u8, scale, t["hist"]


def _through_the_positional_symbol(dev, combo, table, khist):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    mode, pred, guided, philox = combo
    t = _inputs(dev, combo)
    out, u8, scale = _outputs(dev, t)
    lib, p = N.lib(), N.ptr
    lo, hi, w = ops.threshold_ranks(SHAPE[1] * SHAPE[2] * SHAPE[3], RATIO)
    x, eps, noise, tab, sd = p(t["x"]), p(t["eps"]), p(t["noise"]), p(table), p(t["step_dev"])
    tail = (sd, t["step"], p(t["mask"]), N_MASK, 1, 1) + SHAPE + (N.stream_for(t["x"]),)
    th = (lo, hi, w, MAX_VALUE, p(scale) if mode == THRESH else None)
    if philox:
        rc = lib.adm_sched_step_philox(x, eps, p(t["uncond"]) if guided else None, GUIDANCE, p(out), p(u8), tab, *tail, *th, pred, SEED,
                                       ROW_OFFSET)
    elif guided:
        multi = (p(khist), p(t["hist"])) if mode == MULTISTEP else (None, None)
        rc = lib.adm_sched_step_guided(x, eps, p(t["uncond"]), GUIDANCE, noise, p(out), p(u8), tab, *multi, *tail, *th, pred)
    elif mode == MULTISTEP:
        rc = lib.adm_sched_multistep(x, eps, noise, p(out), p(u8), tab, p(khist), p(t["hist"]), *tail)
    elif pred != 0:
        rc = lib.adm_sched_step_pred(x, eps, noise, p(out), p(u8), tab, *tail, *th, pred)
    elif mode == THRESH:
        rc = lib.adm_sched_step_thresholded(x, eps, noise, p(out), p(u8), tab, *tail, *th)
    else:
        rc = lib.adm_sched_step(x, eps, noise, p(out), p(u8), tab, *tail)
    N.check(rc)
    return out, u8, scale, t["hist"]


# ================================================================ A. the 26 kernels: the struct path == the positional symbol
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "mode{}-pred{}-guided{}-stream{}".format(*c))
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_struct_entry_point_gives_the_bits_of_the_positional_symbol(backend, combo):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    assert N.lib().adm_version() >= 114
    table = ops.sched_coef_table(tg.ROWS, dev)
    khist = torch.tensor([r["k_hist"] for r in tg.ROWS], dtype=torch.float32).to(dev)
    assert tg.ROWS[STEP]["k_noise"] != 0.0 and tg.ROWS[STEP]["k_hist"] != 0.0
    x_before = _inputs(dev, combo)["x"]
    got = _through_ops(dev, combo, table, khist)
    want = _through_the_positional_symbol(dev, combo, table, khist)
    for name, g, w in zip(("out", "u8_out", "scale", "hist"), got, want):
        assert torch.equal(g, w), name
        assert bool(torch.isfinite(g.float()).all()), name
    out, u8, scale, hist = got
    mode = combo[0]
    assert not torch.equal(out, x_before) and int(u8.max()) > 0                        # the step ran and wrote both outputs
    assert torch.equal(out[..., 0], _inputs(dev, combo)["mask"][:, STEP, :, 0][:, None])    # the mask row of this step, column 0
    assert (mode == THRESH) == bool((scale >= 1.0).all()) and (mode == MULTISTEP) != torch.equal(hist, _inputs(dev, combo)["hist"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_selection_alone_gives_the_bits_of_the_positional_symbols(backend):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    table = ops.sched_coef_table(tg.ROWS, dev)
    t = _inputs(dev, (THRESH, 0, 0, 0))
    lo, hi, w = ops.threshold_ranks(SHAPE[1] * SHAPE[2] * SHAPE[3], RATIO)
    seen = []
    for max_value in (MAX_VALUE, 1.25):
        for pred, guided in sorted(sched_kernels.THRESHOLD_KERNELS):
            got = ops.sched_threshold(t["x"], t["eps"], table, STEP, RATIO, max_value, prediction=pred, uncond=t["uncond"] if guided else None,
                                      guidance_scale=GUIDANCE if guided else None)
            want = torch.zeros(SHAPE[0], device=dev)
            args = (N.ptr(table), None, STEP, lo, hi, w, max_value, N.ptr(want)) + SHAPE + (N.stream_for(want),)
            if guided:
                rc = N.lib().adm_sched_threshold_guided(N.ptr(t["x"]), N.ptr(t["eps"]), N.ptr(t["uncond"]), GUIDANCE, *args, pred)
            elif pred != 0:
                rc = N.lib().adm_sched_threshold_pred(N.ptr(t["x"]), N.ptr(t["eps"]), *args, pred)
            else:
                rc = N.lib().adm_sched_threshold(N.ptr(t["x"]), N.ptr(t["eps"]), *args)
            N.check(rc)
            assert torch.equal(got, want) and bool(((got >= 1.0) & (got <= max_value)).all()), (pred, guided)
            seen += [(max_value, v) for v in got.tolist()]
    # the ranks and the weight decide some thresholds (strictly inside the clamp) and the maximum decides others
    assert any(1.0 < v < m for m, v in seen) and any(v == 1.25 for m, v in seen)
    assert len({v for m, v in seen if m == MAX_VALUE}) > 2       # the six kernels do not all compute the same thing


# ================================================================ B. what is not built is refused, and says why
@pytest.mark.parametrize("backend", BACKENDS)
def test_combinations_that_are_not_built_are_refused_with_their_reason(backend):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    lib = N.lib()
    table = ops.sched_coef_table(tg.ROWS, dev)
    khist = torch.tensor([r["k_hist"] for r in tg.ROWS], dtype=torch.float32).to(dev)
    t = _inputs(dev, (PLAIN, 0, 0, 0))
    out, _, scale = _outputs(dev, t)

    def call(**fields):
        a = N.SchedStepArgs(x=N.ptr(t["x"]), eps=N.ptr(t["eps"]), out=N.ptr(out), coef_table=N.ptr(table), step=STEP, B=SHAPE[0], C=SHAPE[1],
                            H=SHAPE[2], W=SHAPE[3], max_value=1.0)
        for k, v in fields.items():
            setattr(a, k, v)
        return lib.adm_sched_step_ex(a, N.stream_for(out)), lib.adm_last_error().decode()
    multi = dict(mode=MULTISTEP, k_hist_table=N.ptr(khist), hist=N.ptr(t["hist"]))
    assert call()[0] == 0 and call(**multi)[0] == 0 and call(noise_source=1, seed=SEED)[0] == 0
    refused = [
        (dict(multi, prediction=1), "epsilon only"), (dict(multi, prediction=2), "epsilon only"),
        (dict(multi, scale=N.ptr(scale)), "not thresholded"),
        (dict(multi, noise_source=1), "no noise rows"),
        (dict(noise_source=1, noise=N.ptr(t["noise"])), "exclude each other"),
        (dict(mode=-1), "mode must be"), (dict(mode=3), "mode must be"),
        (dict(prediction=-1), "prediction must be"), (dict(prediction=3), "prediction must be"),
        (dict(noise_source=-1), "noise_source must be"), (dict(noise_source=2), "noise_source must be"),
        (dict(mode=THRESH), "needs scale"), (dict(mode=MULTISTEP, hist=N.ptr(t["hist"])), "k_hist_table"),
        (dict(noise_source=1, row_offset=-1), "row_offset"), (dict(W=6), "multiple of 4"),
        (dict(eps_uncond=N.ptr(t["uncond"]), guidance_scale=float("nan")), "finite"), (dict(x=None), "null argument"),
    ]
    for fields, why in refused:
        rc, msg = call(**fields)
        assert rc != 0 and why in msg, (fields, msg)
    assert lib.adm_sched_step_ex(None, N.stream_for(out)) != 0 and "null argument struct" in lib.adm_last_error().decode()
    assert lib.adm_sched_threshold_ex(None, N.stream_for(out)) != 0 and "null argument struct" in lib.adm_last_error().decode()
    assert lib.adm_sample_loop_ex(None, None, N.stream_for(out)) != 0


# ================================================================ C. the loop
def _coef(rows):
    from audiodiffusion import _native as N
    return (N.SchedCoef * len(rows))(*[N.SchedCoef(*[float(r[k]) for k in tp.FIELDS]) for r in rows])


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_loop_struct_gives_the_bits_of_each_positional_loop_on_one_handle(backend):
    """Two steps, B = 1, the conditional 16 x 16 tiny pipeline. Per positional loop: it, then the struct (which replays the graph the
    positional call captured); then the next family on the same handle, which meets the previous family's captured graph."""
    from audiodiffusion import DPMSolverMultistepScheduler
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = tg._build("ddpm")
    lib, n = N.lib(), 2
    mine.scheduler.set_timesteps(n)
    rows = mine.scheduler.coef_rows()
    assert rows[0]["k_noise"] != 0.0
    solver = DPMSolverMultistepScheduler()
    solver.set_timesteps(n + 1)             # the first two rows of a three-step run: the last row of a run is first order again
    ms_rows = solver.loop_rows(0, n)
    assert ms_rows[0]["k_hist"] == 0.0 and ms_rows[1]["k_hist"] != 0.0
    coef, ms_coef = _coef(rows), _coef(ms_rows)
    khist = (C.c_float * n)(*[float(r["k_hist"]) for r in ms_rows])
    x0, enc, neg = (1.5 * _randn((1, 1, 16, 16), 1)).to(dev), _randn((1, 1, 12), 2).to(dev), _randn((1, 1, 12), 3).to(dev)
    step_noise = _randn((n, 1, 1, 16, 16), 4).to(dev)
    mask = _randn((1, n, 16, 16), 5).to(dev)
    h = mine.unet._ensure_handle()
    mine.unet._set_encoding(h, enc, 1, dev)
    lo, hi, w = ops.threshold_ranks(16 * 16, RATIO)
    th = (lo, hi, w, MAX_VALUE)

    def run(call):
        x = x0.clone()
        u8 = torch.zeros((1, 16, 16, 1), dtype=torch.uint8, device=dev)
        N.check(call(N.ptr(x), N.ptr(u8), N.stream_for(x)))
        return x, u8

    def struct(**fields):
        def call(x, u8, st):
            a = N.SampleLoopArgs(x=x, B=1, coef_host=coef, n_steps=n, step_noise=N.ptr(step_noise), mask=N.ptr(mask), mask_start=1, mask_end=1,
                                 u8_out=u8, use_graph=1, max_value=1.0, guidance_scale=1.0)
            for k, v in fields.items():
                setattr(a, k, v)
            return lib.adm_sample_loop_ex(h, a, st)
        return call
    sn, mk = N.ptr(step_noise), N.ptr(mask)
    thresholded = dict(mode=THRESH, lo=lo, hi=hi, w=w, max_value=MAX_VALUE)
    guided = dict(encoding_uncond=N.ptr(neg), guidance_scale=GUIDANCE)
    families = {
        "adm_sample_loop": (lambda x, u8, st: lib.adm_sample_loop(h, x, 1, coef, n, sn, mk, 1, 1, u8, 1, st), struct()),
        "adm_sample_loop_multistep": (lambda x, u8, st: lib.adm_sample_loop_multistep(h, x, 1, ms_coef, khist, n, sn, mk, 1, 1, u8, 1, st),
                                      struct(mode=MULTISTEP, coef_host=ms_coef, k_hist_host=khist)),
        "adm_sample_loop_thresholded": (lambda x, u8, st: lib.adm_sample_loop_thresholded(h, x, 1, coef, n, sn, mk, 1, 1, u8, 1, st, *th),
                                        struct(**thresholded)),
        "adm_sample_loop_pred": (lambda x, u8, st: lib.adm_sample_loop_pred(h, x, 1, coef, n, sn, mk, 1, 1, u8, 1, st, *th, 1, 2),
                                 struct(prediction=2, **thresholded)),
        "adm_sample_loop_guided": (lambda x, u8, st: lib.adm_sample_loop_guided(h, x, 1, coef, None, n, sn, mk, 1, 1, u8, 1, st, *th, 0, 1,
                                                                                N.ptr(neg), GUIDANCE),
                                   struct(prediction=1, **guided)),
        "adm_sample_loop_philox": (lambda x, u8, st: lib.adm_sample_loop_philox(h, x, 1, coef, n, mk, 1, 1, u8, 1, st, *th, 1, 0, N.ptr(neg),
                                                                                GUIDANCE, SEED, ROW_OFFSET),
                                   struct(step_noise=None, noise_source=1, seed=SEED, row_offset=ROW_OFFSET, **thresholded, **guided)),
    }
    results = {}
    for name, (positional, by_struct) in families.items():
        a, b = run(positional), run(by_struct)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), name
        assert bool(torch.isfinite(a[0]).all()) and not torch.equal(a[0], x0), name
        results[name] = a[0].cpu()
    # six different computations, and the first family again, in the other order, after all the others
    keys = list(results)
    assert all(not torch.equal(results[p], results[q]) for i, p in enumerate(keys) for q in keys[i + 1:])
    for call in reversed(families["adm_sample_loop"]):
        assert torch.equal(run(call)[0].cpu(), results["adm_sample_loop"])
