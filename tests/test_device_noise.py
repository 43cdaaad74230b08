"""Device-side counter-based noise ("adm noise stream 1", include/adm.h): `adm_randn`, the noise-drawing instantiations of the fused step
kernel (`adm_sched_step_philox`), the loop that reads the seed through a device block (`adm_sample_loop_philox`), the keywords of
`ops`, the schedulers, the pipeline and the front end — on the emulator and, under `-m gpu`, on the MI355X.

A. The numpy Philox4x32-10 kept here reproduces the Random123 known answers.
B. `adm_randn` against the float64 restatement of the stream's definition. Bar, the elementwise rule of tests/test_norm_sweep.py and
   tests/test_dpmsolver.py::_judge: max|d| / max|ref| <= 8 * max(e_fp32, 4 * 2^-24), e_fp32 the same formula in numpy float32; every
   value finite and |z| < 5.77.
C. Statistics of the kernel's output: conditions at four standard errors (and the 1 % point of the Kolmogorov-Smirnov statistic),
   which the float64 restatement alone meets with margin (its figures are in the table of each test).
D. Fused == materialised, bit for bit per backend: the step that draws its noise equals the existing entry point fed `ops.randn` of the
   same counters.
E. Invariances of the loop, bit for bit per backend: shard, step chunk, starting step, captured graph, seed not frozen into the graph.
F. The device-noise pipeline against `oracle.pipeline` fed the materialised noise: max|d| <= 1e-3 on the final floats, images within
   1 LSB (the bars of tests/test_pipeline.py).
G. Refusals. I. Register check of every kernel of k_sched.hip. (H, two gloo ranks: tests/test_device_noise_distributed.py.)
"""
import functools
import math
import os
import shutil

import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_guidance as tg
import test_prediction_types as tp
import test_thresholding as tt
import sched_kernels
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import mel as omel
from oracle import pipeline as opipe
from oracle import schedulers as osched

U = 2.0 ** -24
TINY, MEL, _randn, _f32 = td.TINY, td.MEL, td._randn, td._f32
SEED, SEED_HI = 1234, 2 ** 40 + 5            # the second has a non-zero high key word
SHAPES = [(5, 1, 12, 20), (3, 4, 8, 8), (2, 1, 256, 256)]
BIG = (5, 1, 512, 1024)                      # 655 360 float4 > 2048 blocks * 256 lanes: the grid-stride loop wraps
SID = lambda s: "x".join(map(str, s))        # noqa: E731
ZMAX = 5.77                                  # sqrt(48 ln 2) = 5.768...


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ================================================================ A. the generator
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LOW, _S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays that hold 32-bit words. ctr: four arrays (broadcast together), key: two ints."""
    c = [np.asarray(v, dtype=np.uint64) for v in ctr]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LOW]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_numpy_philox_reproduces_the_random123_known_answers(ctr, key, want):
    got = tuple(int(v) for v in philox4x32_10(ctr, key))
    assert got == want, [hex(v) for v in got]


# ---- the restatement of the stream's definition (include/adm.h), in the float type asked for
@functools.lru_cache(maxsize=8)
def _words(shape, seed, row_offset, t, sid):
    B, C, H, W = shape
    assert (C * H * W) % 4 == 0
    q = np.arange(C * H * W // 4, dtype=np.uint64)[None, :]
    row = (np.uint64(row_offset) + np.arange(B, dtype=np.uint64))[:, None]
    zero = np.zeros((B, q.shape[1]), dtype=np.uint64)
    return philox4x32_10((q + zero, row + zero, zero + np.uint64(t), zero + np.uint64(sid)), (seed & 0xFFFFFFFF, seed >> 32))


def _box_muller(a, b, f):
    u1 = ((a >> np.uint64(8)) + np.uint64(1)).astype(f) * f(U)       # (0, 1], exact
    u2 = (b >> np.uint64(8)).astype(f) * f(U)                        # [0, 1), exact
    r = np.sqrt(f(-2.0) * np.log(u1))
    th = f(2.0 * math.pi) * u2
    return r * np.cos(th), r * np.sin(th)


def restate(shape, seed, row_offset=0, t=0, sid=0, f=np.float64):
    """(B, C, H, W) normals of the stream: element 4q + j of row b is normal j of the counter (q, row_offset + b, t, sid)."""
    r = _words(tuple(shape), int(seed), int(row_offset), int(t), int(sid))
    z0, z1 = _box_muller(r[0], r[1], f)
    z2, z3 = _box_muller(r[2], r[3], f)
    out = np.stack([z0, z1, z2, z3], axis=-1)
    assert out.dtype == f
    return torch.from_numpy(out.reshape(shape))


# ================================================================ B. adm_randn against the float64 restatement
def _check_randn(backend, shape, seed, sid, offsets=(0, 7), ts=(0, 500, 999)):
    from audiodiffusion import ops
    dev = select(backend)
    for off in offsets:
        for t in ts:
            got = ops.randn(shape, seed, row_offset=off, t=t, noise_stream=sid, device=dev).cpu()
            ref64, ref32 = restate(shape, seed, off, t, sid), restate(shape, seed, off, t, sid, np.float32)
            assert got.shape == tuple(shape) and got.dtype == torch.float32
            assert bool(torch.isfinite(got).all()), "randn is not finite"
            e_kernel, e_fp32 = td._g(got, ref64), td._g(ref32, ref64)
            bound = 8 * max(e_fp32, 4 * U)
            zmax = float(got.abs().max())
            print(f"DEVNOISE randn backend={backend} shape={shape} seed={seed} off={off} t={t} stream={sid} e_kernel={e_kernel:.3e} "
                  f"e_fp32={e_fp32:.3e} bound={bound:.3e} max|z|={zmax:.3f}")
            assert e_kernel <= bound, (shape, seed, off, t, sid, e_kernel, e_fp32, bound)
            assert zmax < ZMAX


@pytest.mark.parametrize("sid", [0, 1])
@pytest.mark.parametrize("seed", [SEED, SEED_HI], ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
@pytest.mark.parametrize("backend", BACKENDS)
def test_randn_against_the_float64_restatement(backend, shape, seed, sid):
    _check_randn(backend, shape, seed, sid)


@pytest.mark.parametrize("seed", [SEED, SEED_HI], ids=["seed-lo", "seed-hi"])
@pytest.mark.parametrize("t", [0, 500, 999])
@pytest.mark.parametrize("off", [0, 7])
@pytest.mark.parametrize("backend", BACKENDS)
def test_randn_against_the_float64_restatement_where_the_grid_stride_loop_wraps(backend, off, t, seed):
    """(5, 1, 512, 1024): 655 360 float4 for 524 288 lanes. (Most of a case's time is the numpy restatement of 2.6 M normals.)"""
    for sid in (0, 1):
        _check_randn(backend, BIG, seed, sid, offsets=(off,), ts=(t,))


@pytest.mark.parametrize("backend", BACKENDS)
def test_randn_counters_are_what_the_definition_says(backend):
    """Exact statements that need no transcendental function: rows, the row offset, the timestep and the stream id are counter words."""
    from audiodiffusion import ops
    dev = select(backend)
    shape = (5, 1, 12, 20)
    a = ops.randn(shape, SEED, row_offset=0, t=500, device=dev)
    assert _same_bits(ops.randn((2, 1, 12, 20), SEED, row_offset=3, t=500, device=dev), a[3:5])          # row = row_offset + b
    assert _same_bits(ops.randn((5, 2, 12, 10), SEED, t=500, device=dev).reshape(shape), a)             # q counts the flat sample
    assert _same_bits(ops.randn(shape, SEED, t=500, device=dev), a)
    for other in (ops.randn(shape, SEED + 1, t=500, device=dev), ops.randn(shape, SEED, t=499, device=dev),
                  ops.randn(shape, SEED, t=500, noise_stream=1, device=dev), ops.randn(shape, SEED + 2 ** 32, t=500, device=dev)):
        assert not bool((_bits(other) == _bits(a)).any(dim=-1).all())
    assert not torch.equal(a[0], a[1])


# ================================================================ C. statistics of the kernel's output
def _ks(z):
    """Kolmogorov-Smirnov D * sqrt(N) of z against the standard normal distribution function, in float64."""
    z = np.sort(np.asarray(z, dtype=np.float64).ravel())
    n = z.size
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(z) / math.sqrt(2.0))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - cdf).max(), (cdf - (i - 1) / n).max()) * math.sqrt(n))


@pytest.mark.parametrize("backend", BACKENDS)
def test_moments_and_distribution_of_the_kernels_output(backend):
    """seed 1234, rows 0-1, t = 500, stream 0, N = 131 072. The float64 restatement gives |mean| 0.0029, |var - 1| 0.0023,
    |E z^4 - 3| 0.0103, D sqrt(N) 1.178, max|z| 4.91."""
    from audiodiffusion import ops
    dev = select(backend)
    z = ops.randn((2, 1, 256, 256), SEED, row_offset=0, t=500, noise_stream=0, device=dev).cpu().double().numpy().ravel()
    n = z.size
    assert n == 131072
    mean, var, m4, ks, zmax = abs(z.mean()), abs(z.var() - 1.0), abs((z ** 4).mean() - 3.0), _ks(z), np.abs(z).max()
    print(f"DEVNOISE stats backend={backend} |mean|={mean:.4f} |var-1|={var:.4f} |Ez^4-3|={m4:.4f} D*sqrt(N)={ks:.3f} max|z|={zmax:.3f}")
    assert mean <= 4 / math.sqrt(n)
    assert var <= 4 * math.sqrt(2 / n)
    assert m4 <= 4 * math.sqrt(96 / n)
    assert ks <= 1.63
    assert zmax < ZMAX


@pytest.mark.parametrize("backend", BACKENDS)
def test_rows_timesteps_and_neighbours_are_uncorrelated(backend):
    """N = 65 536 per vector; |corr| <= 4 / sqrt(N) = 0.0156. The restatement, evaluated as this test evaluates the kernel, gives 0.0007 (rows), 0.0008 (timesteps), 0.0039 (lag 1)."""
    from audiodiffusion import ops
    dev = select(backend)
    two = ops.randn((2, 1, 256, 256), SEED, t=500, device=dev).cpu().double().numpy().reshape(2, -1)
    prev = ops.randn((1, 1, 256, 256), SEED, t=499, device=dev).cpu().double().numpy().ravel()
    n = two.shape[1]
    assert n == 65536
    corr = lambda a, b: abs(float(np.corrcoef(a, b)[0, 1]))  # noqa: E731
    rows, steps, lag = corr(two[0], two[1]), corr(two[0], prev), corr(two[0][:-1], two[0][1:])
    print(f"DEVNOISE corr backend={backend} rows={rows:.4f} timesteps={steps:.4f} lag1={lag:.4f}")
    for c in (rows, steps, lag):
        assert c <= 4 / math.sqrt(n)


# ================================================================ D. fused == materialised, bit for bit
ROWS = [dict(sqrt_beta=_f32(0.91), sqrt_alpha=_f32(0.41), clip=1.0, k_x0=_f32(0.23), k_x=_f32(0.76), k_eps=0.0, k_noise=_f32(0.4),
             timestep=900.0),                                                                            # a DDPM row
        dict(sqrt_beta=_f32(0.62), sqrt_alpha=_f32(0.78), clip=-1.0, k_x0=_f32(0.62), k_x=0.0, k_eps=_f32(0.31), k_noise=_f32(0.35),
             timestep=500.0),                                                                            # a DDIM row at eta = 1
        dict(sqrt_beta=_f32(0.35), sqrt_alpha=_f32(0.94), clip=1.0, k_x0=_f32(0.44), k_x=_f32(0.52), k_eps=_f32(0.3), k_noise=0.0,
             timestep=100.0)]                                                                            # a row without noise
OFF = 3


def _step(dev, shape, row, pred, thresh, guided, mask, dev_step, **noise_kw):
    """One step through ops.sched_step -> (out, u8, scale or None) on the CPU; noise_kw chooses the noise source."""
    from audiodiffusion import ops
    B, C, H, W = shape
    table = ops.sched_coef_table(ROWS, dev)
    x, e, u = (1.5 * _randn(shape, s) for s in (1, 2, 3))
    m = _randn((B, len(ROWS), H, W), 5).to(dev) if mask else None
    u8 = torch.zeros((B, H * W * C), dtype=torch.uint8, device=dev)
    scale = torch.zeros((B,), dtype=torch.float32, device=dev)
    step_dev = torch.tensor([row], dtype=torch.int32).to(dev) if dev_step else None
    kw = dict(uncond=u.to(dev), guidance_scale=3.0) if guided else {}
    out = ops.sched_step(x.to(dev), e.to(dev), table, -1 if dev_step else row, mask=m, mask_start=3 if mask else 0, mask_end=5 if mask else 0,
                         u8_out=u8, threshold=(0.9, tt.HUGE) if thresh else None, step_dev=step_dev, scale_out=scale, prediction=pred,
                         **kw, **noise_kw)
    return out.cpu(), u8.cpu(), scale.cpu() if thresh else None


DCASES = [pytest.param(s, p, th, g, id=f"{SID(s)}-pred{p}-{'thresh' if th else 'plain'}-{'guided' if g else 'unguided'}")
          for s in SHAPES for p in (0, 1, 2) for th in (False, True) for g in (False, True)]


@pytest.mark.parametrize("shape,pred,thresh,guided", DCASES)
@pytest.mark.parametrize("backend", BACKENDS)
def test_fused_step_equals_the_step_fed_the_materialised_noise(backend, shape, pred, thresh, guided):
    from audiodiffusion import ops
    dev = select(backend)
    for mask in ((False, True) if shape[1] == 1 else (False,)):
        for row in (0, 1):
            dev_step = bool(mask) != bool(row)          # both ways of naming the row, with and without a mask
            nz = ops.randn(shape, SEED_HI, row_offset=OFF, t=int(ROWS[row]["timestep"]), noise_stream=0, device=dev)
            want = _step(dev, shape, row, pred, thresh, guided, mask, dev_step, noise=nz)
            got = _step(dev, shape, row, pred, thresh, guided, mask, dev_step, noise_seed=SEED_HI, noise_row_offset=OFF)
            quiet = _step(dev, shape, row, pred, thresh, guided, mask, dev_step)
            tag = (shape, pred, thresh, guided, mask, row)
            assert _same_bits(got[0], want[0]), tag
            assert torch.equal(got[1], want[1]), tag
            assert thresh == (got[2] is not None) and (not thresh or _same_bits(got[2], want[2])), tag
            assert not torch.equal(got[0], quiet[0]), ("the noise changes nothing", tag)
            other = _step(dev, shape, row, pred, thresh, guided, mask, dev_step, noise_seed=SEED_HI, noise_row_offset=OFF + 1)
            assert not torch.equal(got[0], other[0]), ("the row offset changes nothing", tag)
        # a row with k_noise == 0 draws nothing: the step without noise
        got, quiet = _step(dev, shape, 2, pred, thresh, guided, mask, False, noise_seed=SEED_HI, noise_row_offset=OFF), \
            _step(dev, shape, 2, pred, thresh, guided, mask, False)
        assert _same_bits(got[0], quiet[0]) and torch.equal(got[1], quiet[1])


@pytest.mark.parametrize("backend", BACKENDS)
def test_fused_step_equals_the_materialised_step_where_the_grid_stride_loop_wraps(backend):
    from audiodiffusion import ops
    dev = select(backend)
    nz = ops.randn(BIG, SEED, row_offset=OFF, t=900, device=dev)
    want = _step(dev, BIG, 0, 0, False, False, False, False, noise=nz)
    got = _step(dev, BIG, 0, 0, False, False, False, False, noise_seed=SEED, noise_row_offset=OFF)
    assert _same_bits(got[0], want[0]) and torch.equal(got[1], want[1])


# ================================================================ E. invariances of the loop (TINY model, DDPM, 6 steps, B = 3)
STEPS, B3 = 6, 3


def _tiny_pipe(sched=None):
    from audiodiffusion import AudioDiffusionPipeline, DDPMScheduler, Mel, UNet2DModel
    pipe = AudioDiffusionPipeline(None, UNet2DModel(**TINY).init_random(0), Mel(**MEL), sched if sched is not None else DDPMScheduler())
    pipe.set_progress_bar_config(disable=True)
    return pipe


@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_invariances_bit_for_bit(backend):
    from audiodiffusion import ops
    dev = select(backend)
    pipe = _tiny_pipe()
    sched = pipe.scheduler
    sched.set_timesteps(STEPS)
    assert sum(r["k_noise"] != 0.0 for r in sched.coef_rows()) == STEPS - 1
    x0 = ops.randn((B3, 1, 16, 16), SEED, noise_stream=1, device=dev)
    den = lambda x, start=0, **kw: pipe._denoise(x, start, 0.0, None, None, 0, 0, **kw)  # noqa: E731
    whole, u8 = den(x0, device_noise_seed=SEED)
    # (i) rows [1:3] alone, told where they sit in the global batch
    assert _same_bits(ops.randn((2, 1, 16, 16), SEED, row_offset=1, noise_stream=1, device=dev), x0[1:3])
    part, u8p = den(x0[1:3].contiguous(), device_noise_seed=SEED, device_noise_row_offset=1)
    assert _same_bits(part, whole[1:3]) and torch.equal(u8p, u8[1:3])
    wrong, _ = den(x0[1:3].contiguous(), device_noise_seed=SEED)
    assert not torch.equal(wrong, whole[1:3])
    # (ii) one call == two halves == six eager steps
    half, _ = den(x0, device_noise_seed=SEED, stop_step=3)
    rest, u8r = den(half, 3, device_noise_seed=SEED)
    assert _same_bits(rest, whole) and torch.equal(u8r, u8)
    y = x0
    for t in sched.timesteps:
        y = sched.step(pipe.unet(y, t)["sample"], t, y, device_noise_seed=SEED).prev_sample
    assert _same_bits(y, whole)
    # (iii) captured graph on == off
    if backend != "emu":
        eager, u8e = den(x0, device_noise_seed=SEED, use_graph=False)
        assert _same_bits(eager, whole) and torch.equal(u8e, u8)
    # (iv) seeds A, B, A on the same pipeline: the seed is data behind a pointer, not a value frozen into the captured graph
    other, u8o = den(x0, device_noise_seed=SEED + 1)
    again, u8a = den(x0, device_noise_seed=SEED)
    assert _same_bits(again, whole) and torch.equal(u8a, u8)
    # (v) different seeds give different images
    assert not torch.equal(other, whole) and not torch.equal(u8o, u8)
    # and the host-noise path on the same handle is what it was
    sn = _randn((STEPS, B3, 1, 16, 16), 7).to(dev)
    h1, _ = den(x0, step_noise=sn)
    d2, _ = den(x0, device_noise_seed=SEED)
    h2, _ = den(x0, step_noise=sn)
    assert _same_bits(h1, h2) and _same_bits(d2, whole) and not torch.equal(h1, whole)


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_loop_is_one_native_call_without_a_noise_tensor(backend, monkeypatch):
    """More steps than one staging chunk holds: the host-noise path needs two calls, the device-noise path one."""
    dev = select(backend)
    pipe = _tiny_pipe()
    monkeypatch.setattr(type(pipe), "_STEP_CHUNK", 2)
    calls = spy_sample_loop(monkeypatch)
    pipe(batch_size=1, steps=4, audio=False, device_noise_seed=SEED)
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
    assert calls[0]["noise_source"] == 1 and calls[0]["step_noise"] is None and calls[0]["n_steps"] == 4 and calls[0]["seed"] == SEED
    del calls[:]
    pipe(batch_size=1, steps=4, audio=False, noise=_randn((1, 1, 16, 16), 1).to(dev), step_noise=_randn((4, 1, 1, 16, 16), 2).to(dev))
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"] * 2
    assert all(c["noise_source"] == 0 and c["step_noise"] is not None and c["n_steps"] == 2 for c in calls)


@pytest.mark.parametrize("backend", BACKENDS)
def test_schedules_without_noisy_rows_take_the_seed_for_the_latent_only(backend):
    from audiodiffusion import DDIMScheduler, DPMSolverMultistepScheduler, ops
    dev = select(backend)
    for sched in (DPMSolverMultistepScheduler(), DDIMScheduler()):
        pipe = _tiny_pipe(sched)
        kw = dict(batch_size=2, steps=4, audio=False, return_float=True)
        _, a = pipe(device_noise_seed=SEED, **kw)
        _, b = pipe(noise=ops.randn((2, 1, 16, 16), SEED, noise_stream=1, device=dev), **kw)
        _, c = pipe(device_noise_seed=SEED + 1, **kw)
        assert _same_bits(a, b) and not torch.equal(a, c)


# ================================================================ F. the pipeline against the oracle
_ORACLE = {}


def _pair(cfg):
    """(oracle pipeline, this package's pipeline, eta) over the same TINY weights for one of the unconditional configurations."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, DDPMScheduler, Mel, UNet2DModel
    if "unet" not in _ORACLE:
        torch.manual_seed(0)
        _ORACLE["unet"] = td.OracleUNet(**TINY).eval()
    ref_unet = _ORACLE["unet"]
    unet = UNet2DModel(**TINY).load_state_dict(ref_unet.state_dict())
    eta = 0.0
    if cfg == "ddpm":
        ref_sched, sched = osched.DDPMScheduler(), DDPMScheduler()
    elif cfg == "ddim-eta1":
        ref_sched, sched, eta = osched.DDIMScheduler(), DDIMScheduler(), 1.0
    elif cfg == "ddpm-thresholding":
        ref_sched, sched = tt.RefDDPM(**tt.TH), DDPMScheduler(**tt.TH)
    else:
        ref_sched, sched = tp.RefDDPM(), DDPMScheduler(prediction_type="v_prediction")
        ref_sched.kind = "v_prediction"
    ref = opipe.AudioDiffusionPipeline(None, ref_unet, omel.Mel(**MEL), ref_sched)
    mine = AudioDiffusionPipeline(None, unet, Mel(**MEL), sched)
    mine.set_progress_bar_config(disable=True)
    return ref, mine, eta


def _materialise(mine, dev, B, seed, eta):
    """The latent and the per-step noise the device-noise pipeline draws, as tensors for the oracle: ops.randn of the same counters."""
    from audiodiffusion import ops
    mine.scheduler.set_timesteps(STEPS)
    shape = (B, 1, 16, 16)
    latent = ops.randn(shape, seed, t=0, noise_stream=1, device=dev).cpu()
    step_noise = torch.stack([ops.randn(shape, seed, t=int(t), noise_stream=0, device=dev).cpu() for t in mine.scheduler.timesteps.tolist()])
    assert sum(r["k_noise"] != 0.0 for r in mine.scheduler.coef_rows(eta)) >= STEPS - 1
    return latent, step_noise


def _compare(tag, mi, mf, ri, rf):
    err = float((mf.cpu() - rf).abs().max())
    a = np.stack([np.asarray(i).astype(int) for i in mi])
    b = np.stack([np.asarray(i).astype(int) for i in ri])
    print(f"DEVNOISE pipeline {tag} max|d|={err:.3e} lsb={np.abs(a - b).max()} max|ref|={float(rf.abs().max()):.3f}")
    assert err <= 1e-3
    assert a.shape == b.shape and np.abs(a - b).max() <= 1


@pytest.mark.parametrize("cfg", ["ddpm", "ddim-eta1", "ddpm-thresholding", "ddpm-v_prediction"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_device_noise_sampling_matches_the_oracle_fed_the_materialised_noise(backend, cfg):
    dev = select(backend)
    ref, mine, eta = _pair(cfg)
    latent, step_noise = _materialise(mine, dev, B3, SEED, eta)
    kw = dict(batch_size=B3, steps=STEPS, audio=False, return_float=True, eta=eta)
    ri, rf = ref(noise=latent.clone(), step_noise=step_noise, **kw)
    mi, mf = mine(device_noise_seed=SEED, **kw)
    _compare(f"backend={backend} cfg={cfg}", mi, mf, ri, rf)
    if cfg == "ddpm-thresholding":
        tt._assert_strictly_between(ref)
    # the step noise is really in: the oracle with another step noise is far away
    _, of = ref(noise=latent.clone(), step_noise=torch.flip(step_noise, (0,)), **kw)
    assert float((of - rf).abs().max()) > 1e-2


@pytest.mark.parametrize("backend", BACKENDS)
def test_guided_device_noise_sampling_matches_the_reference_loop(backend):
    dev = select(backend)
    ref, mine = tg._build("ddpm")
    latent, step_noise = _materialise(mine, dev, B3, SEED, 0.0)
    enc = _randn((B3, 1, 12), 43)
    kw = dict(batch_size=B3, steps=STEPS, audio=False, return_float=True)
    tg._guide_reference(ref, 3.0, None)
    ri, rf = ref(noise=latent.clone(), encoding=enc, step_noise=step_noise, **kw)
    mi, mf = mine(device_noise_seed=SEED, encoding=enc.to(dev), guidance_scale=3.0, **kw)
    _compare(f"backend={backend} cfg=ddpm-guided", mi, mf, ri, rf)
    _, plain = mine(device_noise_seed=SEED, encoding=enc.to(dev), **kw)
    assert float((plain.cpu() - rf).abs().max()) > 1e-2


# ================================================================ G. refusals
@pytest.mark.parametrize("backend", BACKENDS)
def test_forbidden_keyword_combinations_raise_and_name_the_keyword(backend, tmp_path):
    from audiodiffusion import AudioDiffusion, DDIMScheduler, DDPMScheduler, ops
    dev = select(backend)
    pipe = _tiny_pipe()
    gen = torch.Generator().manual_seed(0)
    kw = dict(batch_size=1, steps=2, audio=False, device_noise_seed=SEED)
    for name, value in (("generator", gen), ("step_generator", gen), ("step_noise", _randn((2, 1, 1, 16, 16), 1).to(dev))):
        with pytest.raises(ValueError, match=name):
            pipe(**{name: value}, **kw)
    x = _randn((1, 1, 16, 16), 1).to(dev)
    for name, value in (("step_generator", gen), ("step_noise", [x, x])):
        args = dict(step_generator=None, step_noise=None)
        args[name] = value
        with pytest.raises(ValueError, match=name):
            pipe._denoise(x, 0, 0.0, args["step_generator"], None, 0, 0, step_noise=args["step_noise"], device_noise_seed=SEED)
    for bad in (-1, 2 ** 64):
        with pytest.raises(ValueError, match="device_noise_seed"):
            pipe(batch_size=1, steps=2, audio=False, device_noise_seed=bad)
    for sched in (DDPMScheduler(), DDIMScheduler()):
        sched.set_timesteps(4)
        t = sched.timesteps[0]
        for name, value in (("generator", gen), ("variance_noise", x)):
            with pytest.raises(ValueError, match=name):
                sched.step(x, t, x, device_noise_seed=SEED, **{name: value})
        with pytest.raises(TypeError):
            sched.step(x, t, x, *([None] * 7), SEED)       # keyword-only
    table = ops.sched_coef_table(ROWS, dev)
    with pytest.raises(ValueError, match="noise"):
        ops.sched_step(x, x, table, 0, noise=x, noise_seed=SEED)
    # the front end passes the keyword through
    pipe.save_pretrained(str(tmp_path / "pipe"))
    front = AudioDiffusion(str(tmp_path / "pipe"), cuda=backend != "emu", progress_bar=None)
    front.pipe.set_progress_bar_config(disable=True)
    seen = {}
    real = front.pipe._denoise

    def spy(*a, **k):
        seen.update(k)
        return real(*a, **k)
    front.pipe._denoise = spy
    one, _ = front.generate_spectrogram_and_audio(steps=2, device_noise_seed=SEED)
    assert seen["device_noise_seed"] == SEED
    two, _ = front.generate_spectrogram_and_audio(steps=2, device_noise_seed=SEED)
    three, _ = front.generate_spectrogram_and_audio(steps=2, device_noise_seed=SEED + 1)
    assert np.array_equal(np.asarray(one), np.asarray(two)) and not np.array_equal(np.asarray(one), np.asarray(three))
    with pytest.raises(ValueError, match="generator"):
        front.generate_spectrogram_and_audio(steps=2, device_noise_seed=SEED, generator=gen)


@pytest.mark.parametrize("backend", BACKENDS)
def test_abi_version_and_argument_checks(backend):
    from audiodiffusion import UNet2DModel
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    lib = N.lib()
    assert lib.adm_version() >= 113
    for sym in ("adm_randn", "adm_sched_step_philox", "adm_sample_loop_philox"):
        assert hasattr(lib, sym), sym
    out = torch.zeros((2, 16), dtype=torch.float32, device=dev)

    def randn(B=2, per=16, off=0, t=0, sid=0, o=out):
        return lib.adm_randn(N.ptr(o), B, per, SEED, off, t, sid, N.stream_for(out))
    assert randn() == 0 and randn(sid=1) == 0 and randn(off=2 ** 31 - 3, t=2 ** 31 - 1) == 0
    assert randn(per=14) != 0 and "multiple of 4" in lib.adm_last_error().decode()
    assert randn(off=-1) != 0 and "row_offset" in lib.adm_last_error().decode()
    assert randn(t=-1) != 0 and "timestep" in lib.adm_last_error().decode()
    assert randn(sid=2) != 0 and "reserved" in lib.adm_last_error().decode()
    assert randn(B=0) != 0 and randn(o=None) != 0 and randn(per=0) != 0

    shape = (1, 1, 4, 4)
    x, e, o = (_randn(shape, s).to(dev) for s in (1, 2, 3))
    table, scale = ops.sched_coef_table(ROWS, dev), torch.zeros(1).to(dev)

    def step(u=None, g=3.0, off=0, pred=0, scale_=None, W=4, x_=x):
        return lib.adm_sched_step_philox(N.ptr(x_), N.ptr(e), N.ptr(u), g, N.ptr(o), None, N.ptr(table), None, 0, None, 0, 0, 0, 1, 1,
                                         16 // W, W, N.stream_for(x), 3, 4, 0.5, 2.0, N.ptr(scale_), pred, SEED, off)
    assert step() == 0 and step(u=e) == 0 and step(scale_=scale, pred=2) == 0
    assert step(off=-1) != 0 and "row_offset" in lib.adm_last_error().decode()
    assert step(W=2) != 0 and step(pred=3) != 0 and step(x_=None) != 0
    assert step(u=e, g=float("nan")) != 0 and "finite" in lib.adm_last_error().decode()

    pipe = _tiny_pipe()
    pipe.scheduler.set_timesteps(2)
    rows = pipe.scheduler.coef_rows()
    h = pipe.unet._ensure_handle()
    xs = _randn((1, 1, 16, 16), 5).to(dev)

    def loop(off=0, pred=0, neg=None, t0=None, n=2):
        rr = [dict(r) for r in rows]
        if t0 is not None:
            rr[0]["timestep"] = t0
        coef = (N.SchedCoef * 2)(*[N.SchedCoef(*[float(r[k]) for k in tp.FIELDS]) for r in rr])
        return lib.adm_sample_loop_philox(h, N.ptr(xs), 1, coef, n, None, 0, 0, None, 1, N.stream_for(xs), 0, 0, 0.0, 1.0, 0, pred, N.ptr(neg),
                                          3.0, SEED, off)
    assert loop() == 0
    assert loop(off=-1) != 0 and "row_offset" in lib.adm_last_error().decode()
    assert loop(t0=-1.0) != 0 and "timestep" in lib.adm_last_error().decode()
    assert loop(t0=2.0 ** 31) != 0 and "timestep" in lib.adm_last_error().decode()
    assert loop(pred=5) != 0 and loop(n=0) != 0
    assert loop(neg=xs) != 0 and "no cross-attention" in lib.adm_last_error().decode()
    assert isinstance(pipe.unet, UNet2DModel)


# ================================================================ I. register check
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_every_kernel_of_k_sched_compiles_without_scratch():
    """The static check of tests/test_no_spill.py on k_sched.hip: the twelve noise-drawing step kernels and the fill kernel exist, the
    kernel set is exactly the dispatch tables', and no kernel of the file uses scratch on gfx950."""
    sched_kernels.assert_kernel_set_and_no_scratch()
