"""Region in-painting (include/adm.h "Region in-painting"; adm_version() >= 118): the known-region overwrite inside the fused step kernels
(csrc/k_sched_common.h `sched_known4`), the six fields of `adm_sched_step_args` / `adm_sample_loop_args`, and the `keep_mask` /
`known_level` / `known` keywords of the pipeline with `longform.inpaint` / `longform.continue_track`.

A. the step kernel through `adm_sched_step_ex`: the definition bit for bit (A1), identity with the staged `mask=` path (A2), refusals (A3)
B. the loop and the pipeline: composed identity, identity with `mask_start_secs`, exactness of the kept region, the oracle, windowed,
   device noise, four channels, the Python refusals, the long-form helpers

The fused multiply-add of the definition, fma(ka, known, fl32(kb * noise)), is restated in numpy exactly: the product ka*known is exact
in float64, its sum with the fp32 product is rounded to ODD in float64 (TwoSum gives the error term), and 53 >= 24 + 2 bits make the
final rounding to fp32 the single rounding of the fused operation.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_windowed as tw
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import schedulers as osched


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _fma32(a, x, c):
    """fp32 fma(a, x, c), correctly rounded, on numpy float32 operands."""
    p = np.asarray(a, np.float64) * np.asarray(x, np.float64)      # exact: 24 x 24 bits
    c = np.asarray(c, np.float64) + np.zeros_like(p)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                                 # TwoSum: p + c == s + err exactly
    b = s.view(np.int64)
    fix = (err != 0) & ((b & 1) == 0)                               # inexact and even: take the odd neighbour on err's side
    b = np.where(fix, np.where((err > 0) == (s > 0), b + 1, b - 1), b)
    return b.view(np.float64).astype(np.float32)


def _noisy_np(ka, known, kb, noise):
    """noisy_of of csrc/k_sched_common.h: the product kb*noise rounded on its own, then one fused multiply-add."""
    return _fma32(np.float32(ka), known.astype(np.float32), (np.float32(kb) * noise.astype(np.float32)).astype(np.float32))


def test_the_fma_restatement_is_a_single_rounding():
    rng = np.random.default_rng(0)
    a, x, c = (rng.standard_normal(20000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    got = _fma32(a, x, c)
    for i in range(0, 20000, 97):
        exact = Fraction(float(a[i])) * Fraction(float(x[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], np.float32(-np.inf)), np.nextafter(got[i], np.float32(np.inf))
        assert abs(Fraction(float(got[i])) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    # a case where rounding the float64 sum twice goes wrong: 1 + 2^-24 + 2^-60 must round UP in fp32
    assert _fma32(np.float32(1), np.float32(1), np.float32(0)) == np.float32(1)
    assert _fma32(np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)


# ================================================================ A. the step kernel
def _f(v):
    return float(np.float32(v))


ROWS = [dict(sqrt_beta=_f(0.91), sqrt_alpha=_f(0.41), clip=1.0, k_x0=_f(0.23), k_x=_f(0.87), k_eps=_f(0.35), k_noise=0.0, timestep=900.0),
        dict(sqrt_beta=_f(0.62), sqrt_alpha=_f(0.78), clip=1.0, k_x0=_f(0.57), k_x=_f(0.49), k_eps=_f(0.21), k_noise=0.0, timestep=500.0),
        dict(sqrt_beta=_f(0.31), sqrt_alpha=_f(0.95), clip=1.0, k_x0=_f(0.81), k_x=_f(0.17), k_eps=_f(0.11), k_noise=_f(0.27), timestep=100.0)]
K_HIST = [0.0, _f(-0.31), _f(-0.13)]
UROWS = [dict(c_x=0.0, c_m1=0.0, c_m2=0.0, c_t=0.0, p_m1=0.0),
         dict(c_x=_f(0.9), c_m1=_f(0.1), c_m2=0.0, c_t=_f(0.2), p_m1=_f(-0.1)),
         dict(c_x=_f(0.8), c_m1=_f(0.1), c_m2=_f(0.05), c_t=_f(0.2), p_m1=_f(-0.1))]
KNOWN_TABLE = [(_f(0.3), _f(0.95)), (_f(0.7), _f(0.71)), (_f(0.99), _f(0.14))]    # a row taken from the wrong step shows
KINDS = ["plain-eps", "sample-noise", "v", "thresholded", "multistep", "unipc", "unipc-v-thresholded-guided", "guided", "guided-rescaled",
         "philox", "philox-thresholded-guided"]
TH = (0.9, 4.0)


def _inputs(shape, dev, seed=1):
    names = ("x", "e", "u", "nz", "hist", "last", "known", "known_noise")
    t = {n: _randn(shape, seed + i).to(dev) for i, n in enumerate(names)}
    t["hist2"] = _randn((2,) + tuple(shape), seed + 20).to(dev)
    t["known"] = t["known"].clamp(-1, 1)
    return t


def _run(kind, dev, shape, t, known):
    """One step of `kind` -> dict(out, u8, and the solver state the step writes). The state tensors are fresh copies each time."""
    from audiodiffusion import ops
    table = ops.sched_coef_table(ROWS, dev)
    u8 = torch.zeros(shape, dtype=torch.uint8, device=dev)       # (the kernel packs at the float's flat index)
    x, e, u, st = t["x"], t["e"], t["u"], {}
    kw = dict(u8_out=u8, known=known)
    if kind == "plain-eps":
        out = ops.sched_step(x, e, table, 1, **kw)
    elif kind == "sample-noise":
        out = ops.sched_step(x, e, table, 2, noise=t["nz"], prediction=1, **kw)
    elif kind == "v":
        out = ops.sched_step(x, e, table, 1, prediction=2, **kw)
    elif kind == "thresholded":
        out = ops.sched_step(x, e, table, 1, threshold=TH, **kw)
    elif kind == "multistep":
        st["hist"] = t["hist"].clone()
        out = ops.sched_multistep(x, e, table, torch.tensor(K_HIST).to(dev), st["hist"], 1, **kw)
    elif kind.startswith("unipc"):
        st["hist2"], st["last"] = t["hist2"].clone(), t["last"].clone()
        extra = dict(prediction=2, threshold=TH, uncond=u, guidance_scale=3.0) if kind != "unipc" else {}
        out = ops.sched_unipc(x, e, table, ops.sched_unipc_table(UROWS, dev), st["hist2"], st["last"], 2, **extra, **kw)
    elif kind == "guided":
        out = ops.sched_step(x, e, table, 1, uncond=u, guidance_scale=3.0, **kw)
    elif kind == "guided-rescaled":
        out = ops.sched_step(x, e, table, 1, uncond=u, guidance_scale=3.0, guidance_rescale=0.7, **kw)
    elif kind == "philox":
        out = ops.sched_step(x, e, table, 2, noise_seed=77, noise_row_offset=3, **kw)
    else:
        assert kind == "philox-thresholded-guided"
        out = ops.sched_step(x, e, table, 2, noise_seed=77, threshold=TH, uncond=u, guidance_scale=2.0, prediction=2, **kw)
    return dict(out=out, u8=u8, **st)


def _step_of(kind):
    return 2 if kind.startswith("unipc") or kind in ("sample-noise", "philox", "philox-thresholded-guided") else 1


def _masks(shape):
    """name -> (Bm, H, W) uint8. Columns whose edges fall inside a float4, one pixel, a frequency band, nothing, everything, and one
    mask per sample."""
    B, _, H, W = shape
    m = {n: np.zeros((1, H, W), np.uint8) for n in ("columns", "pixel", "band", "zeros")}
    m["columns"][:, :, 3:9] = 1
    m["pixel"][0, H // 2, 5] = 1
    m["band"][:, 2:6, :] = 1
    m["ones"] = np.ones((1, H, W), np.uint8)
    m["per-sample"] = (np.random.default_rng(5).random((B, H, W)) < 0.3).astype(np.uint8)
    m["per-sample"][:, :, 3:9] ^= 1
    m["per-sample"][0, 0, :4] = (0, 7, 0, 255)          # any non-zero byte keeps
    return m


def _check_definition(kind, dev, shape, t, base, keep, known_batched):
    from audiodiffusion import ops
    B = shape[0]
    table = torch.tensor(KNOWN_TABLE, dtype=torch.float32).to(dev)
    known = t["known"] if known_batched else t["known"][:1].contiguous()
    got = _run(kind, dev, shape, t, (known, t["known_noise"], torch.from_numpy(keep).to(dev), table))
    ka, kb = KNOWN_TABLE[_step_of(kind)]
    noisy = _noisy_np(ka, np.broadcast_to(known.cpu().numpy(), shape), kb, t["known_noise"].cpu().numpy())
    k = np.broadcast_to(keep[:, None] != 0, (keep.shape[0],) + tuple(shape[1:]))
    k = np.broadcast_to(k, shape)
    want = np.where(k, noisy, base["out"].cpu().numpy())
    assert np.array_equal(_bits(got["out"].cpu().numpy()), _bits(want)), (kind, shape)
    want_u8 = ops.dequant_u8(torch.from_numpy(want).to(dev))
    assert torch.equal(got["u8"], want_u8) and torch.equal(ops.dequant_u8(base["out"]), base["u8"]), (kind, shape)
    for name in ("hist", "hist2", "last"):               # the solver's state is written before the overwrite and never sees it
        if name in base:
            assert torch.equal(got[name], base[name]), (kind, name)
    if not k.any():
        assert torch.equal(got["out"], base["out"]) and torch.equal(got["u8"], base["u8"])
    return got


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(3, 1, 8, 16), (2, 4, 4, 12)], ids=["3x1x8x16", "2x4x4x12"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_overwrite_is_the_definition_bit_for_bit(backend, shape, kind):
    """A1. (3,1,8,16): fewer float4 than one workgroup; (2,4,4,12): C > 1, the keep index wraps over the channels."""
    dev = select(backend)
    t = _inputs(shape, dev)
    base = _run(kind, dev, shape, t, None)
    assert float((base["out"] - t["x"]).abs().max()) > 1e-2
    masks = _masks(shape)
    outs = {}
    for name, keep in masks.items():
        outs[name] = _check_definition(kind, dev, shape, t, base, keep, known_batched=True)
    # the broadcast mask against the same mask given per sample; `known` broadcast against per sample (with equal rows)
    B = shape[0]
    rep = _check_definition(kind, dev, shape, t, base, np.repeat(masks["columns"], B, 0), known_batched=True)
    assert torch.equal(rep["out"], outs["columns"]["out"])
    one = _check_definition(kind, dev, shape, t, base, masks["per-sample"], known_batched=False)
    t2 = dict(t, known=t["known"][:1].expand(shape).contiguous())
    many = _check_definition(kind, dev, shape, t2, base, masks["per-sample"], known_batched=True)
    assert torch.equal(one["out"], many["out"]) and not torch.equal(one["out"], outs["per-sample"]["out"])


@pytest.mark.parametrize("kind", ["plain-eps", "unipc"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_overwrite_above_the_grid_cap(backend, kind):
    """A1 at (9,1,256,1024): 589824 float4 against 2048 blocks of 256 lanes, so the grid-stride loop runs twice."""
    dev = select(backend)
    shape = (9, 1, 256, 1024)
    t = _inputs(shape, dev, seed=3)
    base = _run(kind, dev, shape, t, None)
    keep = _masks(shape)["per-sample"]
    assert 0.2 < keep.mean() < 0.4 and keep[8].any()
    _check_definition(kind, dev, shape, t, base, keep, known_batched=True)


@pytest.mark.parametrize("ms,me", [(5, 0), (0, 6), (3, 3)])
@pytest.mark.parametrize("kind", ["plain-eps", "multistep", "unipc"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_edge_columns_at_the_current_level_are_the_staged_mask_path(backend, kind, ms, me):
    """A2. C == 1, keep = columns [0, ms) u [W - me, W), known (1, H, W): `out` and u8 equal those of the existing `mask=` path with
    the mask that `ops.add_noise(..., per_sample=False)` builds: add_noise_kernel's arithmetic is sched_known4's, bit for bit."""
    from audiodiffusion import ops
    dev = select(backend)
    shape = (2, 1, 8, 16)
    B, _, H, W = shape
    t = _inputs(shape, dev, seed=7)
    acp = torch.tensor([0.0413, 0.3371, 0.8912], dtype=torch.float32)
    sa, sb = (acp ** 0.5).to(dev), ((1 - acp) ** 0.5).to(dev)
    known = t["known"][0].contiguous()                                              # (1, H, W)
    mask = ops.add_noise(known, t["known_noise"], sa, sb, per_sample=False)         # (B, 3, H, W)
    keep = np.zeros((1, H, W), np.uint8)
    keep[:, :, :ms] = 1
    keep[:, :, W - me:] = 1
    table = torch.stack([sa, sb], 1).contiguous()
    step = _step_of(kind)

    def run(**kw):
        u8 = torch.zeros(shape, dtype=torch.uint8, device=dev)
        if kind == "plain-eps":
            out = ops.sched_step(t["x"], t["e"], ops.sched_coef_table(ROWS, dev), step, u8_out=u8, **kw)
        elif kind == "multistep":
            out = ops.sched_multistep(t["x"], t["e"], ops.sched_coef_table(ROWS, dev), torch.tensor(K_HIST).to(dev), t["hist"].clone(),
                                      step, u8_out=u8, **kw)
        else:
            out = ops.sched_unipc(t["x"], t["e"], ops.sched_coef_table(ROWS, dev), ops.sched_unipc_table(UROWS, dev), t["hist2"].clone(),
                                  t["last"].clone(), step, u8_out=u8, **kw)
        return out, u8
    staged = run(mask=mask, mask_start=ms, mask_end=me)
    fused = run(known=(known[None].contiguous(), t["known_noise"], torch.from_numpy(keep).to(dev), table))
    plain = run()
    assert torch.equal(staged[0], fused[0]) and torch.equal(staged[1], fused[1])
    assert not torch.equal(plain[0], fused[0])


@pytest.mark.parametrize("backend", BACKENDS)
def test_step_refusals_name_the_field(backend):
    """A3."""
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    lib = N.lib()
    assert lib.adm_version() >= 118
    shape = (2, 1, 8, 16)
    t = _inputs(shape, dev)
    out = torch.empty(shape, device=dev)
    table, ktable = ops.sched_coef_table(ROWS, dev), torch.tensor(KNOWN_TABLE, dtype=torch.float32).to(dev)
    keep = torch.ones((1, 8, 16), dtype=torch.uint8, device=dev)
    mask = torch.zeros((2, 3, 8, 16), device=dev)
    full = dict(known=N.ptr(t["known"]), known_noise=N.ptr(t["known_noise"]), keep=N.ptr(keep), known_table=N.ptr(ktable), known_batched=1)

    def call(**f):
        a = N.SchedStepArgs(x=N.ptr(t["x"]), eps=N.ptr(t["e"]), out=N.ptr(out), coef_table=N.ptr(table), step=1, B=2, C=1, H=8, W=16, **f)
        return lib.adm_sched_step_ex(a, N.stream_for(out)), lib.adm_last_error().decode()
    utab, hist2, last = ops.sched_unipc_table(UROWS, dev), t["hist2"].clone(), t["last"].clone()
    for extra in ({}, dict(unipc_table=N.ptr(utab), hist=N.ptr(hist2), last=N.ptr(last))):    # both launchers
        for drop, word in (("known", "known"), ("known_noise", "known_noise"), ("known_table", "known_table")):
            rc, msg = call(**{k: v for k, v in full.items() if k != drop}, **extra)
            assert rc != 0 and "keep" in msg and word in msg, msg
        rc, msg = call(mask=N.ptr(mask), n_mask_steps=3, mask_start=2, **full, **extra)
        assert rc != 0 and "keep" in msg and "mask" in msg, msg
        rc, msg = call(**full, **extra)
        assert rc == 0, msg
        rc, msg = call(**{k: v for k, v in full.items() if k != "keep"}, **extra)     # without keep the other fields are ignored
        assert rc == 0, msg


# ================================================================ B. the loop and the pipeline
KINDS_B = ["ddim", "ddpm", "dpm", "unipc"]


def _coef(sched, level):
    """The (ka, kb) rows restated: add_noise's coefficients at timesteps[i] ("current") or timesteps[i + 1] and (1, 0) ("previous")."""
    acp, ts = sched.alphas_cumprod, sched.timesteps.tolist()
    cur = [(float(acp[t] ** 0.5), float((1 - acp[t]) ** 0.5)) for t in ts]
    return cur if level == "current" else cur[1:] + [(1.0, 0.0)]


def _den(mine, x, **kw):
    return mine._denoise(x, 0, 0.0, None, None, 0, 0, **kw)


def _composed(mine, x0, keep, known, noise, level, window=None, **step_kw):
    """The loop, step by step: the forward (windowed: gather, forward, blend) and `scheduler.step` (adm_sched_step_ex) with the overwrite."""
    from audiodiffusion import ops
    sched, y = mine.scheduler, x0
    coef = _coef(sched, level)
    for k, t in enumerate(sched.timesteps):
        if window is None:
            o = mine.unet(y, t)["sample"]
        else:
            s, wrap = window
            o = ops.window_blend(mine.unet(ops.window_gather(y, 16, s, wrap), t)["sample"], y.shape[3], s, wrap)
        y = sched.step(o, t, y, known=(known, noise, keep, *coef[k]), **step_kw).prev_sample
    return y


def _keep_cols(H, W, lo, hi, dev):
    k = torch.zeros((H, W), dtype=torch.uint8)
    k[:, lo:hi] = 1
    return k.to(dev)


@pytest.mark.parametrize("kind", KINDS_B)
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_native_loop_is_the_steps_composed_from_the_public_pieces(backend, kind):
    """B1. The emulator has no graph (use_graph 0 and 1, a first call and a replay are the same code there), so what only a captured
    graph can get wrong runs on the device alone."""
    dev = select(backend)
    hip = backend != "emu"
    n, B = 2, 2
    _, mine = tw._pipe(tw._scheduler(kind))
    sched = mine.scheduler
    x0, known, noise = (_randn((B, 1, 16, 16), 21 + i).to(dev) for i in range(3))
    known = known.clamp(-1, 1)
    keep = _keep_cols(16, 16, 5, 11, dev)
    keep[3, 0] = 1
    den_kw = step_kw = dict(device_noise_seed=77, device_noise_row_offset=2) if kind == "ddpm" else {}

    def both(keep, known, level):
        """-> the native loop's result, after checking it against the composed steps."""
        sched.set_timesteps(n)
        whole, u8 = _den(mine, x0, keep_mask=keep, known=known, known_noise=noise, known_level=level, **den_kw)
        sched.set_timesteps(n)
        y = _composed(mine, x0, keep, known, noise, level, **step_kw)
        sched.set_timesteps(n)
        assert torch.equal(whole, y), (kind, level)
        return whole, u8
    first, u8 = both(keep, known, "previous")
    kw = dict(keep_mask=keep, known=known, known_noise=noise, known_level="previous", **den_kw)
    if hip:
        eager, u8e = _den(mine, x0, use_graph=False, **kw)
        again, u8a = _den(mine, x0, **kw)                                  # replays the captured graph
        assert torch.equal(first, eager) and torch.equal(first, again) and torch.equal(u8, u8e) and torch.equal(u8, u8a)
    if hip or kind == "ddim":
        assert not torch.equal(both(keep, known, "current")[0], first)
    plain1 = _den(mine, x0, **den_kw)[0]                                   # an ordinary loop on the same handle, in between
    keep.zero_()[:, 2:7] = 1                                               # new contents in the same buffer
    second, _ = both(keep, known, "previous")
    assert not torch.equal(second, first) and not torch.equal(plain1, second)
    if hip:
        keep2, known2 = keep.clone(), (0.5 * known).contiguous()           # new buffers
        third, _ = both(keep2, known2, "previous")
        plain2 = _den(mine, x0, **den_kw)[0]
        assert torch.equal(plain1, plain2) and not torch.equal(plain1, third)
        assert torch.equal(_den(mine, x0, **dict(kw, keep_mask=keep2, known=known2))[0], third)
        assert torch.equal(_den(mine, x0, **kw)[0], second)


def _audio(n=2000, seed=0):
    return (0.2 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _bytes(images):
    return np.stack([np.asarray(i) for i in images])


@pytest.mark.parametrize("backend", BACKENDS)
def test_edge_columns_at_the_current_level_give_the_images_of_mask_secs(backend):
    """B2. pixels_per_second = 16 * 4000 / 16 / 64 = 62.5: mask_start_secs = 0.1 keeps 6 columns, mask_end_secs = 0.05 keeps 3."""
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    a, n = _audio(), _randn((2, 1, 16, 16), 31)
    kw = dict(raw_audio=a, batch_size=2, steps=2, audio=False, return_float=True)
    for ms, me, lo, hi in ((0.1, 0.05, 6, 13), (0.1, 0, 6, 16), (0, 0.05, 0, 13)):
        keep = np.ones((16, 16), bool)
        keep[:, lo:hi] = False
        old_i, old_f = mine(mask_start_secs=ms, mask_end_secs=me, noise=n.clone().to(dev), **kw)
        new_i, new_f = mine(keep_mask=keep, known_level="current", noise=n.clone().to(dev), **kw)
        assert np.array_equal(_bytes(old_i), _bytes(new_i)) and torch.equal(old_f, new_f)
    free_i, _ = mine(noise=n.clone().to(dev), batch_size=2, steps=2, audio=False, return_float=True)
    assert not np.array_equal(_bytes(free_i), _bytes(new_i))


@pytest.mark.parametrize("kind", KINDS_B)
@pytest.mark.parametrize("backend", BACKENDS)
def test_at_the_previous_level_the_kept_pixels_are_the_input_bytes(backend, kind):
    """B3. A middle span and a frequency band; everything outside is generated (and is not the input)."""
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler(kind))
    a = _audio()
    mine.mel.load_audio(raw_audio=a)
    src = np.asarray(mine.mel.audio_slice_to_image(0))
    span, band = np.ones((16, 16), np.uint8), np.zeros((1, 16, 16), np.uint8)
    span[:, 5:11] = 0                    # regenerate a span in the middle
    band[:, 2:6, :] = 1                  # keep a frequency band
    for keep in (span, band):
        images = mine(raw_audio=a, keep_mask=keep, batch_size=2, steps=3, audio=False, generator=torch.Generator().manual_seed(3)).images
        got, k = _bytes(images), np.broadcast_to(keep.reshape(1, 16, 16) != 0, (2, 16, 16))
        assert np.array_equal(got[k], np.broadcast_to(src, (2, 16, 16))[k])
        assert (got[~k] != np.broadcast_to(src, (2, 16, 16))[~k]).mean() > 0.5
    assert dev is not None


def _u8(x):
    return ((x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")


@pytest.mark.parametrize("level", ["previous", "current"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_sampling_matches_the_oracle(backend, level):
    """B4. A torch restatement on the oracle UNet and the oracle DDIM scheduler: sched.step, then where(keep, ka*known + kb*noise, x).
    The bars of tests/test_pipeline.py, test_dpmsolver.py and test_windowed.py for this model and length: max|d| <= 1e-3 on the floats,
    images within 1 LSB."""
    dev = select(backend)
    ref_unet, mine = tw._pipe(tw._scheduler("ddim"))
    noise, known = _randn((2, 1, 16, 16), 42), _randn((2, 1, 16, 16), 43).clamp(-1, 1)
    keep = torch.zeros(16, 16, dtype=torch.bool)
    keep[:, 4:10] = True
    keep[12:, :] = True
    sched = osched.DDIMScheduler()
    sched.set_timesteps(4)
    ts = sched.timesteps.tolist()
    acp = sched.alphas_cumprod.double()
    cur = [(float(acp[t] ** 0.5), float((1 - acp[t]) ** 0.5)) for t in ts]
    coef = cur if level == "current" else cur[1:] + [(1.0, 0.0)]
    x = noise.clone()
    with torch.no_grad():
        for (ka, kb), t in zip(coef, sched.timesteps):
            x = sched.step(ref_unet(x, t)["sample"], t, x)["prev_sample"]
            x = torch.where(keep, ka * known + kb * noise, x)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), keep_mask=keep, known=known.to(dev), known_level=level, audio=False,
                  return_float=True)
    err = float((mf.cpu() - x).abs().max())
    a, b = _bytes(mi).astype(int), _u8(x)[..., 0].astype(int)
    print(f"INPAINT oracle level={level} max|d|={err:.3e} lsb={np.abs(a - b).max()}")
    assert err <= 1e-3
    assert a.shape == b.shape == (2, 16, 16) and np.abs(a - b).max() <= 1


@pytest.mark.parametrize("wrap", [False, True], ids=["open", "circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_windowed_inpainting(backend, wrap, monkeypatch):
    """B5. frames = 32, window_stride = 8, columns 0..11 kept."""
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    sched = mine.scheduler
    x0, known, noise = (_randn((2, 1, 16, 32), 51 + i).to(dev) for i in range(3))
    known = known.clamp(-1, 1)
    keep = _keep_cols(16, 32, 0, 12, dev)
    sched.set_timesteps(2)
    whole, _ = _den(mine, x0, window_stride=8, circular=wrap, keep_mask=keep, known=known, known_noise=noise)
    sched.set_timesteps(2)
    y = _composed(mine, x0, keep, known, noise, "previous", window=(8, wrap))
    assert torch.equal(whole, y)
    assert torch.equal(whole[..., :12], known[..., :12]) and not torch.equal(whole[..., 12:], known[..., 12:])
    if backend != "emu":
        free, _ = _den(mine, x0, window_stride=8, circular=wrap)
        assert not torch.equal(free[..., 12:], whole[..., 12:])      # the generated columns see the kept ones through the windows
    calls = spy_sample_loop(monkeypatch)
    images, mf = mine(batch_size=2, steps=2, noise=x0.clone(), frames=32, window_stride=8, circular=wrap, keep_mask=keep, known=known,
                      audio=False, return_float=True)
    monkeypatch.undo()
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
    c = calls[0]
    assert c["mask"] is None and (c["window_total_w"], c["window_stride"], c["window_wrap"]) == (32, 8, int(wrap))
    assert c["keep"] is not None and c["known"] is not None and c["known_noise"] is not None and c["known_coef_host"] is not None
    assert images[0].size == (32, 16) and torch.equal(mf[..., :12], known[..., :12])
    # an audio input as the source, through the Mel of width `frames`
    a = _audio(3000)
    wide = mine._wide_mel(32)
    wide.load_audio(raw_audio=a)
    src = np.asarray(wide.audio_slice_to_image(0))
    images = mine(batch_size=1, steps=2, raw_audio=a, frames=32, window_stride=8, circular=wrap, keep_mask=keep, audio=False).images
    assert np.array_equal(_bytes(images)[:, :, :12], src[None, :, :12])


@pytest.mark.parametrize("backend", BACKENDS)
def test_ddpm_with_device_noise_and_a_keep_mask_is_one_native_call(backend, monkeypatch):
    """B6. The staged paths run in chunks of _STEP_CHUNK steps; this one does not, and has no tensor with a step axis."""
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddpm"))
    mine._STEP_CHUNK = 2
    keep = np.zeros((16, 16), np.uint8)
    keep[:, 4:9] = 1
    calls = spy_sample_loop(monkeypatch)
    out = mine(batch_size=2, steps=5, raw_audio=_audio(), keep_mask=keep, device_noise_seed=9, audio=False)
    monkeypatch.undo()
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
    c = calls[0]
    assert c["mask"] is None and c["step_noise"] is None and c["noise_source"] == 1 and c["n_steps"] == 5 and c["keep"] is not None
    assert len(out.images) == 2 and dev is not None


@pytest.mark.parametrize("backend", BACKENDS)
def test_four_channels(backend):
    """B7 (the model): a 4-channel model, `known` a latent, a (H, W) mask broadcast over the channels."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel, UNet2DModel
    from oracle.unet import UNet2DModel as OracleUNet
    dev = select(backend)
    cfg = dict(td.TINY, in_channels=4, out_channels=4)
    torch.manual_seed(0)
    unet = UNet2DModel(**cfg).load_state_dict(OracleUNet(**cfg).eval().state_dict())
    mine = AudioDiffusionPipeline(None, unet, Mel(**td.MEL), DDIMScheduler())
    mine.set_progress_bar_config(disable=True)
    x0, known, noise = (_randn((2, 4, 16, 16), 61 + i).to(dev) for i in range(3))
    known = known[:1].contiguous()                                         # one latent for both samples
    keep = _keep_cols(16, 16, 6, 13, dev)
    mine.scheduler.set_timesteps(3)
    whole, _ = _den(mine, x0, keep_mask=keep, known=known, known_noise=noise, want_u8=False)
    mine.scheduler.set_timesteps(3)
    y = _composed(mine, x0, keep, known, noise, "previous")
    assert torch.equal(whole, y)
    assert torch.equal(whole[..., 6:13], known.expand(2, -1, -1, -1)[..., 6:13])           # every channel
    for ch in range(4):
        assert not torch.equal(whole[:, ch, :, :6], known.expand(2, -1, -1, -1)[:, ch, :, :6])


@pytest.mark.parametrize("backend", BACKENDS)
def test_latent_pipeline(backend, monkeypatch):
    """B7 (the pipeline): with a `vqvae` the audio input is encoded and scaled, and the mask has the latent's resolution."""
    from audiodiffusion import AudioDiffusionPipeline, AutoencoderKL, DDIMScheduler, Mel, UNet2DModel
    from oracle.unet import UNet2DModel as OracleUNet
    from oracle.vae import AutoencoderKL as OracleVAE
    dev = select(backend)
    torch.manual_seed(0)
    ref_unet, ref_vae = OracleUNet(**td.TINY).eval(), OracleVAE(**td.VAE_TINY).eval()
    unet = UNet2DModel(**td.TINY).load_state_dict(ref_unet.state_dict())
    vae = AutoencoderKL(**td.VAE_TINY).load_state_dict(ref_vae.state_dict())
    mine = AudioDiffusionPipeline(vae, unet, Mel(**td.MEL32), DDIMScheduler()).to(dev)
    mine.set_progress_bar_config(disable=True)
    keep = np.zeros((16, 16), np.uint8)
    keep[:, :7] = 1
    seen, real = {}, mine._denoise

    def spy(*a, **kw):
        seen.update(kw)
        seen["out"] = real(*a, **kw)
        return seen["out"]
    monkeypatch.setattr(mine, "_denoise", spy)
    a = _audio(4000)
    out = mine(raw_audio=a, keep_mask=keep, batch_size=2, steps=3, audio=False, generator=torch.Generator().manual_seed(1))
    assert [i.size for i in out.images] == [(32, 32)] * 2
    assert tuple(seen["known"].shape) == (1, 1, 16, 16) and tuple(seen["keep_mask"].shape) == (1, 16, 16)
    latent = seen["out"][0]
    assert torch.equal(latent[..., :7], seen["known"].expand(2, -1, -1, -1)[..., :7])       # the kept latent cells are the encoded input's
    with pytest.raises(ValueError, match="keep_mask"):
        mine(raw_audio=a, keep_mask=np.zeros((32, 32), np.uint8), steps=2, audio=False)     # image resolution is not the latent's


@pytest.mark.parametrize("backend", BACKENDS)
def test_every_python_refusal_names_its_keyword(backend, monkeypatch):
    """B8."""
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    calls = spy_sample_loop(monkeypatch)
    a, keep = _audio(), np.ones((16, 16), np.uint8)
    kw = dict(steps=2, audio=False)
    for bad, word in [(dict(keep_mask=keep), "keep_mask"),                                                     # no source
                      (dict(keep_mask=keep, raw_audio=a, mask_start_secs=0.1), "keep_mask"),
                      (dict(keep_mask=keep, raw_audio=a, mask_end_secs=0.1), "keep_mask"),
                      (dict(keep_mask=np.ones((16, 12), np.uint8), raw_audio=a), "keep_mask"),
                      (dict(keep_mask=np.ones((3, 16, 16), np.uint8), raw_audio=a, batch_size=2), "keep_mask"),
                      (dict(keep_mask=np.ones((1, 1, 16, 16), np.uint8), raw_audio=a), "keep_mask"),
                      (dict(keep_mask=keep, raw_audio=a, known_level="next"), "known_level"),
                      (dict(known_level="next"), "known_level"),
                      (dict(keep_mask=keep, known=torch.zeros(1, 1, 16, 12)), "known"),
                      (dict(keep_mask=keep, known=torch.zeros(3, 1, 16, 16), batch_size=2), "known"),
                      (dict(keep_mask=keep, known=torch.zeros(16, 16)), "known"),
                      (dict(keep_mask=keep, known=torch.zeros(1, 1, 16, 16), raw_audio=a), "known"),
                      (dict(known=torch.zeros(1, 1, 16, 16)), "keep_mask"),
                      (dict(frames=32, raw_audio=a), "raw_audio"),                                             # without a mask: as before
                      (dict(frames=32, keep_mask=keep, raw_audio=a), "keep_mask")]:                             # the mask is `frames` wide
        with pytest.raises(ValueError, match=word):
            mine(**kw, **bad)
    mine.vqvae = object()
    with pytest.raises(NotImplementedError, match="vqvae"):
        mine(frames=32, keep_mask=np.ones((16, 32), np.uint8), raw_audio=a, **kw)
    assert calls == [] and dev is not None


@pytest.mark.parametrize("backend", BACKENDS)
def test_loop_refusals_name_the_field(backend):
    """The C-ABI's own refusals of adm_sample_loop_ex, and the refusal of the old mask with window_total_w, word for word."""
    from audiodiffusion import _native as N
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    mine(batch_size=1, steps=2, audio=False)         # a finalized handle
    lib, h = N.lib(), mine.unet._handle
    x = torch.zeros(1, 1, 16, 16, device=dev)
    keep = torch.ones(1, 16, 16, dtype=torch.uint8, device=dev)
    coef = (N.SchedCoef * 1)(N.SchedCoef(0.5, 0.5, 1.0, 1.0, 0.0, 0.0, 0.0, 10.0))
    kc = (ctypes.c_float * 2)(1.0, 0.0)
    full = dict(known=N.ptr(x), known_noise=N.ptr(x), keep=N.ptr(keep), known_coef_host=kc)

    def call(**f):
        a = N.SampleLoopArgs(x=N.ptr(x), B=1, coef_host=coef, n_steps=1, use_graph=0, max_value=1.0, guidance_scale=1.0, **f)
        return lib.adm_sample_loop_ex(h, a, None), lib.adm_last_error().decode()
    for drop, word in (("known", "known"), ("known_noise", "known_noise"), ("known_coef_host", "known_coef_host")):
        rc, msg = call(**{k: v for k, v in full.items() if k != drop})
        assert rc != 0 and "keep" in msg and word in msg, msg
    rc, msg = call(mask=N.ptr(x), **full)
    assert rc != 0 and "keep" in msg and "mask" in msg, msg
    xw = torch.zeros(1, 1, 16, 32, device=dev)
    a = N.SampleLoopArgs(x=N.ptr(xw), B=1, coef_host=coef, n_steps=1, use_graph=0, max_value=1.0, guidance_scale=1.0, window_total_w=32,
                         window_stride=8, mask=N.ptr(xw))
    assert lib.adm_sample_loop_ex(h, a, None) != 0
    assert lib.adm_last_error().decode().endswith("sample_loop: mask must be NULL with window_total_w (the mask's layout assumes the model's width)")
    rc, msg = call(**full)
    assert rc == 0, msg


@pytest.mark.parametrize("backend", BACKENDS)
def test_longform_inpaint_and_continue_track(backend, monkeypatch):
    """B9. One column is hop_length / sample_rate = 0.016 s; pixels_per_second = 62.5."""
    from audiodiffusion import longform
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    a = _audio()
    keep = longform.span_keep_mask(mine, [(0.1, 0.15), (0.2, 0.21)])
    want = np.ones((16, 16), np.uint8)
    want[:, 6:9] = 0                     # int(6.25) .. int(9.375)
    want[:, 12:13] = 0                   # int(12.5) .. int(13.125)
    assert np.array_equal(keep, want)
    (images, _), keep2 = longform.inpaint(mine, a, [(0.1, 0.15), (0.2, 0.21)], steps=3, batch_size=2, audio=False, return_dict=False)
    mine.mel.load_audio(raw_audio=a)
    src = np.broadcast_to(np.asarray(mine.mel.audio_slice_to_image(0)), (2, 16, 16))
    k = np.broadcast_to(want != 0, (2, 16, 16))
    assert np.array_equal(keep2, want) and np.array_equal(_bytes(images)[k], src[k]) and not np.array_equal(_bytes(images)[~k], src[~k])
    # continue_track: 1100 samples cover 17 columns; 0.5 s with 0.128 s overlap is frames = 32, stride = 8 (tests/test_windowed.py)
    calls = spy_sample_loop(monkeypatch)
    (images, (sr, audios)), used = longform.continue_track(mine, a[:1100], 0.5, 0.128, steps=3, return_dict=False)
    monkeypatch.undo()
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
    assert (calls[0]["window_total_w"], calls[0]["window_stride"], calls[0]["B"]) == (32, 8, 1) and calls[0]["keep"] is not None
    assert (used["frames"], used["window_stride"], used["kept_columns"]) == (32, 8, 17) and abs(used["seconds"] - 0.512) < 1e-9
    wide = mine._wide_mel(32)
    wide.load_audio(raw_audio=a[:1100])
    src = np.asarray(wide.audio_slice_to_image(0))
    got = np.asarray(images[0])
    assert got.shape == (16, 32) and np.array_equal(got[:, :17], src[:, :17]) and not np.array_equal(got[:, 17:], src[:, 17:])
    assert audios[0].shape == (64 * 31,) and dev is not None


@pytest.mark.parametrize("backend", BACKENDS)
def test_start_step_noises_every_sample_and_the_noise_is_the_latent(backend, monkeypatch):
    """With `start_step > 0` every row of the batch starts from add_noise(known, noise, timesteps[start_step - 1]), and the noise of the
    overwrite is a copy of the initial latent taken before that write."""
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    seen, real = {}, mine._denoise

    def spy(images, start_step, *a, **kw):
        seen.update(kw, images=images.clone(), start_step=start_step)
        return real(images, start_step, *a, **kw)
    monkeypatch.setattr(mine, "_denoise", spy)
    n, known = _randn((2, 1, 16, 16), 71).to(dev), _randn((1, 1, 16, 16), 72).clamp(-1, 1).to(dev)
    keep = np.zeros((16, 16), np.uint8)
    keep[:, 9:] = 1
    images, mf = mine(batch_size=2, steps=5, start_step=2, noise=n.clone(), keep_mask=keep, known=known, audio=False, return_float=True)
    sched = mine.scheduler
    t = sched.timesteps[1]
    sa, sb = (sched.alphas_cumprod[t] ** 0.5).reshape(1).repeat(2).to(dev), ((1 - sched.alphas_cumprod[t]) ** 0.5).reshape(1).repeat(2).to(dev)
    want = ops.add_noise(known.expand(2, -1, -1, -1).contiguous(), n, sa, sb, per_sample=True)
    assert seen["start_step"] == 2 and torch.equal(seen["images"], want) and torch.equal(seen["known_noise"], n)
    assert seen["known_noise"].data_ptr() != seen["images"].data_ptr()
    assert torch.equal(mf[..., 9:], known.expand(2, -1, -1, -1)[..., 9:]) and len(images) == 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_front_end_passes_the_keywords_through(backend, tmp_path):
    from audiodiffusion import AudioDiffusion
    dev = select(backend)
    _, mine = tw._pipe(tw._scheduler("ddim"))
    mine.save_pretrained(str(tmp_path / "pipe"))
    front = AudioDiffusion(str(tmp_path / "pipe"), cuda=backend != "emu", progress_bar=None)
    front.pipe.set_progress_bar_config(disable=True)
    seen, real = {}, front.pipe._denoise

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)
    front.pipe._denoise = spy
    a = _audio(3000)
    keep = np.zeros((16, 32), np.uint8)
    keep[:, :10] = 1
    img, (sr, audio) = front.generate_spectrogram_and_audio_from_audio(raw_audio=a, steps=2, keep_mask=keep, known_level="current", frames=32)
    assert img.size == (32, 16) and audio.shape == (64 * 31,) and seen["known_level"] == "current" and seen["window_stride"] == 8
    assert tuple(seen["keep_mask"].shape) == (1, 16, 32) and tuple(seen["known"].shape) == (1, 1, 16, 32) and dev is not None
    img, _ = front.generate_spectrogram_and_audio_from_audio(raw_audio=a, steps=2)
    assert img.size == (16, 16) and seen["keep_mask"] is None and seen["known"] is None
