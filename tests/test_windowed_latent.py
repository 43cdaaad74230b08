"""Windowed sampling for latent models (include/adm.h "Tiled codec"; adm_version() >= 121): the cross-fade kernel `adm_window_crossfade`
(csrc/k_window.hip), `AutoencoderKL.decode_tiled` / `encode_tiled`, `frames` with a `vqvae` in the pipeline, and the long-form helpers.

A. the kernel against a numpy fp32 restatement of the definition kept here, bit for bit, with its properties and refusals
B. decode_tiled: identities bit for bit (one window, the composition of the public pieces, the circle, batch independence), the oracle
C. encode_tiled: the same
D. the pipeline: these raise NotImplementedError without the feature
E. longform on a latent pipeline

Shapes: the tiny VAE of tests/test_vae.py (f = 2, 32x32 image, 16x16 latent), the tiny W = 16 UNet of tests/test_dpmsolver.py, every
placement of tests/test_windowed.py::PLACEMENTS in latent cells (x f in pixels), B in {1, 2}, C in {1, 2}, H in {1, 4}.
"""
import ctypes

import numpy as np
import pytest
import torch

import test_dpmsolver as td
import test_vae as tv
import test_windowed as tw
from native_backend import BACKENDS, select, spy_sample_loop

PLACEMENTS, PIDS, W = tw.PLACEMENTS, tw.PIDS, tw.W
U = 2.0 ** -24
COVERS = {(16, 16, False): {1}, (48, 16, False): {1}, (32, 8, False): {1, 2}, (28, 12, False): {1, 2}, (24, 4, False): {1, 2, 3},
          (32, 8, True): {2}, (24, 12, True): {1, 2}, (32, 4, True): {4}, (20, 4, True): {4}}


def _weights(Wt, Wm, s, wrap):
    """(nW, Wm) integer weights m_w(j) of the definition."""
    nW = Wt // s if wrap else (Wt - Wm) // s + 1
    r = Wm - s
    m = np.ones((nW, Wm), np.int64)
    if r == 0:
        return m
    j = np.arange(Wm)
    for w in range(nW):
        left = nW > 1 if wrap else w > 0
        right = nW > 1 if wrap else w < nW - 1
        a = np.minimum(2 * j + 1, 2 * r) if left else np.full(Wm, 2 * r)
        b = np.minimum(2 * (Wm - 1 - j) + 1, 2 * r) if right else np.full(Wm, 2 * r)
        m[w] = np.minimum(a, b)
    assert m.min() >= 1 and m.max() <= 2 * r
    return m


def _np_crossfade(win, Wt, s, wrap, dtype=np.float32):
    """The definition, sequentially: ascending window index (a wrapping window of a column always has a higher index than its
    non-wrapping ones, so this IS "non-wrapping first, then wrapping"), the sum starts from the first product, every product and every
    addition rounded to `dtype` on its own, integer weight sum, one division; a column one window covers is a copy.
    -> (out, cover count per column, weight sum per column)"""
    BW, Cc, H, Wm = win.shape
    cols, m = tw._cols(Wt, Wm, s, wrap), _weights(Wt, Wm, s, wrap)
    nW = len(cols)
    win = win.reshape(BW // nW, nW, Cc, H, Wm).astype(dtype)
    acc = np.zeros((BW // nW, Cc, H, Wt), dtype)
    only = np.zeros_like(acc)
    count, den = np.zeros(Wt, np.int64), np.zeros(Wt, np.int64)
    for w in range(nW):
        first = count[cols[w]] == 0
        p = (m[w].astype(dtype) * win[:, w]).astype(dtype)
        only[..., cols[w][first]] = win[:, w][..., first]
        acc[..., cols[w][first]] = p[..., first]
        acc[..., cols[w][~first]] = (acc[..., cols[w][~first]] + p[..., ~first]).astype(dtype)
        count[cols[w]] += 1
        den[cols[w]] += m[w]
    assert count.min() >= 1
    out = (acc / den.astype(dtype)).astype(dtype)
    out[..., count == 1] = only[..., count == 1]
    return out, count, den


def _bits(a):
    return tw._bits(a.cpu().numpy() if torch.is_tensor(a) else a)


# ================================================================ A. the kernel
def _check_kernel(dev, shape, Wm, s, wrap, seed):
    from audiodiffusion import ops
    Wt = shape[3]
    x = tw._randn(shape, seed)
    win = ops.window_gather(x.to(dev), Wm, s, wrap)
    o = tw._randn(tuple(win.shape), seed + 1)                       # independent window values, as a codec's outputs are
    got, u8 = ops.window_crossfade(o.to(dev), Wt, s, wrap, want_u8=True)
    ref, count, den = _np_crossfade(o.numpy(), Wt, s, wrap)
    assert tuple(got.shape) == tuple(shape) == ref.shape and np.array_equal(_bits(got), _bits(ref)), (shape, s, wrap)
    assert u8.dtype == torch.uint8 and torch.equal(u8, ops.dequant_u8(got)), (shape, s, wrap)
    plain = ops.window_crossfade(o.to(dev), Wt, s, wrap)            # u8_out NULL
    assert torch.equal(plain, got)
    # cover-1 columns are copies: of whichever window covers them
    one = count == 1
    if one.any():
        blend = ops.window_blend(o.to(dev), Wt, s, wrap)            # (o / 1.0f is o)
        assert np.array_equal(_bits(got[..., one]), _bits(blend[..., one]))
    if s == Wm:
        assert torch.equal(got, ops.window_blend(o.to(dev), Wt, s, wrap))
    # crossfade(gather(x)): exact on cover-1 columns, elsewhere `cover` products, cover - 1 additions, one division on same-sign terms
    back = ops.window_crossfade(win, Wt, s, wrap).cpu().numpy()
    xn = x.numpy()
    assert np.array_equal(_bits(back[..., one]), _bits(xn[..., one]))
    assert np.all(np.abs(back.astype(np.float64) - xn) <= (count + 2) * U * np.abs(xn).astype(np.float64)), (shape, s, wrap)
    if 2 * s == Wm:
        inner = count == 2
        assert np.all(den[inner] == 2 * (Wm - s))                   # the linear cross-fade of two windows
    return count, den


@pytest.mark.parametrize("Wt,s,wrap", PLACEMENTS, ids=PIDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_crossfade_is_the_definition_bit_for_bit(backend, Wt, s, wrap):
    dev = select(backend)
    covers, varies = set(), False
    for f in (1, 2):
        for B in (1, 2):
            for Cc in (1, 2):
                for H in (1, 4):
                    count, den = _check_kernel(dev, (B, Cc, H, f * Wt), f * W, f * s, wrap, 11 + B + 2 * Cc + H + f)
                    covers |= set(count.tolist())
                    varies |= len(set(den[count > 1].tolist())) > 1
    assert covers == COVERS[(Wt, s, wrap)]
    # the weight sum is the constant 2r wherever the windows are evenly spread over a column (stride W/2; the cover-4 circles, 32);
    # the open cover-3 placement has edge windows without a ramp, and there it varies: the normalisation is needed
    assert varies == ((Wt, s, wrap) == (24, 4, False))


@pytest.mark.parametrize("backend", BACKENDS)
def test_crossfade_at_size(backend):
    """The grid-stride loop: more float4 in the wide tensor (589824) than the capped grid has lanes (2048 blocks of 256)."""
    dev = select(backend)
    _check_kernel(dev, (3, 1, 256, 3072), 256, 128, True, 3)


@pytest.mark.parametrize("backend", BACKENDS)
def test_crossfade_refusals_carry_the_name_of_the_argument(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    lib = N.lib()
    assert lib.adm_version() >= 121
    a, b = torch.zeros(4096, device=dev), torch.zeros(4096, device=dev)
    c = torch.zeros(4096, dtype=torch.uint8, device=dev)
    ok = dict(B=1, C=1, H=1, total_w=32, W=16, stride=8, wrap=0)
    order = ("B", "C", "H", "total_w", "W", "stride", "wrap")
    cases = [(dict(total_w=34), "total_w"), (dict(total_w=12), "total_w"), (dict(total_w=36), "total_w"),
             (dict(total_w=40, stride=16, wrap=1), "total_w"),
             (dict(stride=6), "stride"), (dict(stride=0), "stride"), (dict(stride=-8), "stride"), (dict(stride=20, total_w=36), "stride"),
             (dict(wrap=2), "wrap"), (dict(wrap=-1), "wrap"), (dict(W=18), "W"), (dict(B=0), "B"), (dict(C=0), "C"),
             (dict(B=1 << 30, total_w=48), "int")]
    for bad, word in cases:
        k = dict(ok, **bad)
        rc = lib.adm_window_crossfade(N.ptr(a), N.ptr(b), N.ptr(c), *[k[n] for n in order], None)
        assert rc != 0 and word in lib.adm_last_error().decode(), (bad, lib.adm_last_error())
    for pa, pb in ((None, N.ptr(b)), (N.ptr(a), None)):
        assert lib.adm_window_crossfade(pa, pb, None, *[ok[n] for n in order], None) != 0
        assert "null" in lib.adm_last_error().decode()
    assert lib.adm_window_crossfade(N.ptr(a), N.ptr(b), None, *[ok[n] for n in order], None) == 0
    assert lib.adm_window_crossfade(N.ptr(a), N.ptr(b), N.ptr(c), *[ok[n] for n in order], None) == 0
    for bad, word in [(dict(total_w=36), "total_w"), (dict(stride=6), "stride"), (dict(wrap=2), "wrap")]:
        k = dict(dict(total_w=32, stride=8, wrap=False), **bad)
        with pytest.raises(ValueError, match=word):
            ops.window_crossfade(torch.zeros(3, 1, 1, 16, device=dev), k["total_w"], k["stride"], k["wrap"])


# ================================================================ B. decode
_PAIRS = {}


def _vae(name="TINY"):
    """(oracle VAE, this package's VAE with its weights): built once per configuration, never modified."""
    if name not in _PAIRS:
        _PAIRS[name] = tv._pair(getattr(tv, name))
    return _PAIRS[name]


def _crossfade64(win, Wt, s, wrap):
    return _np_crossfade(win.double().numpy(), Wt, s, wrap, np.float64)[0]


@pytest.mark.parametrize("backend", BACKENDS)
def test_decode_tiled_of_one_window_is_decode(backend):
    dev = select(backend)
    _, mine = _vae()
    z = tw._randn((2, 1, 16, 16), 1).to(dev)
    for circular in (False, True):
        out = mine.decode_tiled(z, 16, 16, circular, _in_scale=1 / 0.18215, want_u8=True)
        assert torch.equal(out["sample"], mine.decode(z, _in_scale=1 / 0.18215)["sample"])
        assert torch.equal(out.sample, out["sample"]) and tuple(out.u8.shape) == (2, 1, 32, 32)
    assert set(mine.decode_tiled(z, 16, 8)) == {"sample"}


@pytest.mark.parametrize("Wt,s,wrap", PLACEMENTS, ids=PIDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_decode_tiled_is_the_composition_of_the_public_pieces(backend, Wt, s, wrap):
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = _vae()
    z = tw._randn((2, 1, 16, Wt), 2).to(dev)
    got = mine.decode_tiled(z, W, s, wrap, _in_scale=0.5, want_u8=True)
    windows = ops.window_gather(z, W, s, wrap)
    pixels = mine.decode(windows, _in_scale=0.5)["sample"]
    assert tuple(pixels.shape) == (windows.shape[0], 1, 32, 32)
    want, u8 = ops.window_crossfade(pixels, 2 * Wt, 2 * s, wrap, want_u8=True)
    assert tuple(got.sample.shape) == (2, 1, 32, 2 * Wt) and torch.equal(got.sample, want) and torch.equal(got.u8, u8)


@pytest.mark.parametrize("backend", BACKENDS)
def test_sample_b_of_a_batch_has_the_bits_of_its_own_call(backend):
    dev = select(backend)
    _, mine = _vae()
    z = tw._randn((2, 1, 16, 28), 2).to(dev)
    both = mine.decode_tiled(z, 16, 12, False, _in_scale=0.5).sample
    for b in range(2):
        assert torch.equal(mine.decode_tiled(z[b:b + 1].contiguous(), 16, 12, False, _in_scale=0.5).sample[0], both[b])


@pytest.mark.parametrize("cfg,Wt,s,wrap", [("TINY", 32, 8, False), ("TINY", 24, 4, False), ("TINY", 32, 8, True), ("TINY", 20, 4, True),
                                           ("TINY_GEMM_ATTN", 32, 8, False)],
                         ids=["32-8-open", "24-4-open", "32-8-circular", "20-4-circular", "gemmattn-32-8-open"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_decode_tiled_matches_the_oracle(backend, cfg, Wt, s, wrap):
    """The oracle VAE on each window and a float64 cross-fade; the bar of tests/test_vae.py. TINY_GEMM_ATTN: the attention with
    per-sample weights at batch B*nW."""
    dev = select(backend)
    ref, mine = _vae(cfg)
    z = tw._randn((2, 1, 16, Wt), 3)
    with torch.no_grad():
        pixels = ref.decode(torch.from_numpy(tw._np_gather(z.numpy(), W, s, wrap)))["sample"]
    want = _crossfade64(pixels, 2 * Wt, 2 * s, wrap)
    got = mine.decode_tiled(z.to(dev), W, s, wrap).sample.cpu().double().numpy()
    err = float(np.abs(got - want).max())
    print(f"decode_tiled {cfg} {Wt}-{s}-{wrap}: max error {err:.3e}, max |ref| {np.abs(want).max():.3e}")
    assert err <= 1e-3 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_on_the_circle_a_roll_of_the_latent_is_a_roll_of_the_image(backend):
    """stride = W/2 on the circle: every column is a two-term sum, and a two-term fp32 sum commutes."""
    dev = select(backend)
    _, mine = _vae()
    z = tw._randn((1, 1, 16, 32), 4)
    a = mine.decode_tiled(z.to(dev), 16, 8, True).sample
    for k in (1, 3):
        b = mine.decode_tiled(torch.roll(z, 8 * k, dims=3).contiguous().to(dev), 16, 8, True).sample
        assert torch.equal(b, torch.roll(a, 16 * k, dims=3))


# ================================================================ C. encode
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_tiled_of_one_window_is_encode(backend):
    dev = select(backend)
    _, mine = _vae()
    x, noise = tw._randn((2, 1, 32, 32), 5).to(dev), tw._randn((2, 1, 16, 16), 6).to(dev)
    for circular in (False, True):
        dist, one = mine.encode_tiled(x, 32, 32, circular).latent_dist, mine.encode(x).latent_dist
        assert torch.equal(dist.sample(noise=noise), one.sample(noise=noise)) and torch.equal(dist.mode(), one.mode())
        g1, g2 = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
        assert torch.equal(dist.sample(generator=g1), one.sample(generator=g2))


def _moments(mine, windows):
    """quant_conv(encoder(windows)) through the C-ABI's public entry point."""
    from audiodiffusion import _native as N
    h = mine._ensure_handle(windows.shape[2:])
    BW = windows.shape[0]
    z = torch.empty((BW, 1, 16, 16), device=windows.device)
    mom = torch.empty((BW, 2, 16, 16), device=windows.device)
    N.check(N.lib().adm_vae_encode(h, N.ptr(windows), None, ctypes.c_float(1.0), N.ptr(z), N.ptr(mom), BW, N.stream_for(windows)))
    return mom


@pytest.mark.parametrize("Wt,s,wrap", PLACEMENTS, ids=PIDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_tiled_is_the_composition_of_the_public_pieces(backend, Wt, s, wrap):
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = _vae()
    x, noise = tw._randn((2, 1, 32, 2 * Wt), 7).to(dev), tw._randn((2, 1, 16, Wt), 8).to(dev)
    dist = mine.encode_tiled(x, 2 * W, 2 * s, wrap).latent_dist
    wide = ops.window_crossfade(_moments(mine, ops.window_gather(x, 2 * W, 2 * s, wrap)), Wt, s, wrap)
    assert tuple(wide.shape) == (2, 2, 16, Wt) and torch.equal(dist.moments, wide)
    for nz in (noise, None):
        want = torch.empty((2, 1, 16, Wt), device=dev)
        N.check(N.lib().adm_vae_sample_moments(N.ptr(wide), N.ptr(nz), ctypes.c_float(1.0), N.ptr(want), 2, 1, 16 * Wt, N.stream_for(wide)))
        assert torch.equal(dist.sample(noise=nz) if nz is not None else dist.mode(), want)
    # the tail kernel's expression on the cross-faded moments, first order: exp and two roundings
    mean, logvar = wide[:, :1].cpu().double(), wide[:, 1:].cpu().double().clamp(-30, 20)
    ref = mean + torch.exp(0.5 * logvar) * noise.cpu().double()
    assert float((dist.sample(noise=noise).cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("Wt,s,wrap", [(32, 8, False), (24, 4, False), (32, 8, True)], ids=["32-8-open", "24-4-open", "32-8-circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_tiled_matches_the_oracle(backend, Wt, s, wrap):
    dev = select(backend)
    ref, mine = _vae()
    x, noise = tw._randn((2, 1, 32, 2 * Wt), 9), tw._randn((2, 1, 16, Wt), 10)
    with torch.no_grad():
        d = ref.encode(torch.from_numpy(tw._np_gather(x.numpy(), 2 * W, 2 * s, wrap))).latent_dist
    mean = torch.from_numpy(_crossfade64(d.mean, Wt, s, wrap))
    logvar = torch.from_numpy(_crossfade64(d.logvar, Wt, s, wrap)).clamp(-30.0, 20.0)
    want = mean + torch.exp(0.5 * logvar) * noise.double()
    dist = mine.encode_tiled(x.to(dev), 2 * W, 2 * s, wrap).latent_dist
    got = dist.sample(noise=noise.to(dev)).cpu().double()
    assert tuple(got.shape) == (2, 1, 16, Wt)
    print(f"encode_tiled {Wt}-{s}-{wrap}: max error {float((got - want).abs().max()):.3e}")
    assert float((got - want).abs().max()) <= 1e-3 * max(1.0, float(want.abs().max()))
    assert float((dist.mode().cpu().double() - mean).abs().max()) <= 1e-3 * max(1.0, float(mean.abs().max()))


@pytest.mark.parametrize("backend", BACKENDS)
def test_encode_tiled_refuses_by_name(backend):
    dev = select(backend)
    _, mine = _vae()
    x = torch.zeros(1, 1, 32, 64, device=dev)
    for kw, word in [(dict(tile_w=32, stride=12), "stride"), (dict(tile_w=32, stride=4), "stride"), (dict(tile_w=32, stride=0), "stride"),
                     (dict(tile_w=36, stride=8), "tile_w"), (dict(tile_w=32, stride=24), "width"), (dict(tile_w=32, stride=40), "stride")]:
        with pytest.raises(ValueError, match=word):
            mine.encode_tiled(x, **kw)
    with pytest.raises(ValueError, match="noise"):
        mine.encode_tiled(x, 32, 16).latent_dist.sample(noise=torch.zeros(1, 1, 16, 16, device=dev))
    with pytest.raises(ValueError, match="stride"):
        mine.decode_tiled(torch.zeros(1, 1, 16, 32, device=dev), 16, 6)


# ================================================================ D. the pipeline
def _pipes(dev, kind="ddim"):
    """(the latent pipeline: tiny VAE + tiny W = 16 UNet, the same UNet and scheduler kind without a VAE)."""
    from audiodiffusion import AudioDiffusionPipeline, Mel, UNet2DModel
    from oracle.unet import UNet2DModel as OracleUNet
    torch.manual_seed(0)
    unet = UNet2DModel(**td.TINY).load_state_dict(OracleUNet(**td.TINY).eval().state_dict())
    _, vae = _vae()
    latent = AudioDiffusionPipeline(vae, unet, Mel(**td.MEL32), tw._scheduler(kind)).to(dev)
    bare = AudioDiffusionPipeline(None, unet, Mel(**td.MEL), tw._scheduler(kind)).to(dev)
    latent.set_progress_bar_config(disable=True), bare.set_progress_bar_config(disable=True)
    return latent, bare


def _image_bytes(images):
    return np.stack([np.asarray(i) for i in images])


@pytest.mark.parametrize("kind,circular", [("ddim", False), ("ddim", True), ("ddpm", False), ("unipc", True)],
                         ids=["ddim-open", "ddim-circular", "ddpm-open", "unipc-circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_frames_with_a_vqvae_decodes_the_loops_latents_in_tiles(backend, kind, circular):
    from audiodiffusion import ops
    dev = select(backend)
    latent, bare = _pipes(dev, kind)
    noise = tw._randn((2, 1, 16, 32), 21).to(dev)
    kw = dict(batch_size=2, frames=32, steps=2, audio=False, return_float=True, circular=circular)
    images, floats = latent(noise=noise.clone(), generator=torch.Generator().manual_seed(1), **kw)
    assert [i.size for i in images] == [(64, 32)] * 2 and tuple(floats.shape) == (2, 1, 32, 64)
    _, z = bare(noise=noise.clone(), generator=torch.Generator().manual_seed(1), **kw)
    assert tuple(z.shape) == (2, 1, 16, 32)
    want = latent.vqvae.decode_tiled(z, 16, 8, circular, _in_scale=1 / 0.18215)["sample"]
    assert torch.equal(floats, want)
    assert np.array_equal(_image_bytes(images), ops.dequant_u8(want)[:, 0].cpu().numpy())
    if kind == "ddim" and not circular:     # an explicit stride, and the default noise draw at the wide latent shape
        kw = dict(kw, batch_size=1, steps=1, frames=24, window_stride=4)
        _, f2 = latent(generator=torch.Generator().manual_seed(2), **kw)
        _, z2 = bare(generator=torch.Generator().manual_seed(2), **kw)
        assert tuple(z2.shape) == (1, 1, 16, 24) and torch.equal(f2, latent.vqvae.decode_tiled(z2, 16, 4, False, _in_scale=1 / 0.18215)["sample"])


@pytest.mark.parametrize("backend", BACKENDS)
def test_keep_mask_with_known_latents_keeps_them_exactly(backend, monkeypatch):
    dev = select(backend)
    latent, _ = _pipes(dev)
    keep = np.zeros((16, 32), np.uint8)
    keep[:, 5:19] = 1
    keep[3:9, 25:] = 1
    known = tw._randn((1, 1, 16, 32), 22).to(dev)
    seen, real = {}, latent._denoise

    def spy(*a, **kw):
        seen["out"] = real(*a, **kw)
        return seen["out"]
    monkeypatch.setattr(latent, "_denoise", spy)
    images, floats = latent(batch_size=2, frames=32, steps=3, audio=False, return_float=True, keep_mask=keep, known=known,
                            generator=torch.Generator().manual_seed(1))
    z = seen["out"][0]
    k = torch.from_numpy(keep != 0).to(dev).expand(2, 1, 16, 32)
    assert torch.equal(z[k], known.expand(2, -1, -1, -1)[k]) and not torch.equal(z[~k], known.expand(2, -1, -1, -1)[~k])
    assert torch.equal(floats, latent.vqvae.decode_tiled(z, 16, 8, False, _in_scale=1 / 0.18215)["sample"])
    assert [i.size for i in images] == [(64, 32)] * 2


@pytest.mark.parametrize("backend", BACKENDS)
def test_keep_mask_with_audio_encodes_the_wide_mel_image_in_tiles(backend, monkeypatch):
    dev = select(backend)
    latent, _ = _pipes(dev)
    keep = np.zeros((16, 32), np.uint8)
    keep[:, :11] = 1
    audio = (0.2 * np.random.default_rng(0).standard_normal(6000)).astype(np.float32)
    seen, real = {}, latent._denoise

    def spy(*a, **kw):
        seen.update(kw)
        seen["out"] = real(*a, **kw)
        return seen["out"]
    monkeypatch.setattr(latent, "_denoise", spy)
    noise = tw._randn((2, 1, 16, 32), 23).to(dev)
    out = latent(batch_size=2, frames=32, steps=2, raw_audio=audio, keep_mask=keep, noise=noise.clone(),
                 generator=torch.Generator().manual_seed(4))
    assert [i.size for i in out.images] == [(64, 32)] * 2 and out.audios.shape == (2, 1, td.MEL32["hop_length"] * 63)
    mel = latent._wide_mel(64)
    mel.load_audio(raw_audio=audio)
    img = np.asarray(mel.audio_slice_to_image(0))
    assert img.shape == (32, 64)
    x = torch.tensor((img / 255) * 2 - 1, dtype=torch.float)[None, None].to(dev)
    want = 0.18215 * latent.vqvae.encode_tiled(x, 32, 16).latent_dist.sample(generator=torch.Generator().manual_seed(4))
    assert tuple(seen["known"].shape) == (1, 1, 16, 32) and torch.equal(seen["known"], want)
    assert torch.equal(seen["out"][0][..., :11], want.expand(2, -1, -1, -1)[..., :11])


@pytest.mark.parametrize("backend", BACKENDS)
def test_audio_of_a_wide_latent_run_has_the_wide_images_length(backend):
    dev = select(backend)
    latent, _ = _pipes(dev)
    out = latent(batch_size=1, frames=32, steps=2, circular=True, generator=torch.Generator().manual_seed(1))
    assert out.images[0].size == (64, 32) and out.audios.shape == (1, 1, td.MEL32["hop_length"] * (2 * 32 - 1))


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_vqvae_that_cannot_decode_tiles_is_refused_before_any_work(backend, monkeypatch):
    dev = select(backend)
    latent, _ = _pipes(dev)
    calls = spy_sample_loop(monkeypatch)

    class Foreign:
        config = latent.vqvae.config

        def decode(self, *a, **k):
            raise AssertionError("no work before the refusal")
        encode = decode
    latent.vqvae = Foreign()
    with pytest.raises(NotImplementedError, match="vqvae"):
        latent(frames=32, steps=2, audio=False)
    with pytest.raises(NotImplementedError, match="vqvae"):
        latent(frames=32, steps=2, audio=False, keep_mask=np.ones((16, 32), np.uint8), raw_audio=np.zeros(3000, np.float32))
    assert calls == []


@pytest.mark.parametrize("backend", BACKENDS)
def test_without_frames_the_vqvae_path_is_the_one_it_was(backend, monkeypatch):
    from audiodiffusion import ops
    dev = select(backend)
    latent, bare = _pipes(dev)

    def never(*a, **k):
        raise AssertionError("decode_tiled / encode_tiled without `frames`")
    monkeypatch.setattr(latent.vqvae, "decode_tiled", never)
    monkeypatch.setattr(latent.vqvae, "encode_tiled", never)
    noise = tw._randn((2, 1, 16, 16), 24).to(dev)
    kw = dict(batch_size=2, steps=2, audio=False, return_float=True)
    images, floats = latent(noise=noise.clone(), **kw)
    _, z = bare(noise=noise.clone(), **kw)
    want = latent.vqvae.decode(z, _in_scale=1 / 0.18215)["sample"]
    assert torch.equal(floats, want) and np.array_equal(_image_bytes(images), ops.dequant_u8(want)[:, 0].cpu().numpy())
    audio = (0.2 * np.random.default_rng(0).standard_normal(4000)).astype(np.float32)
    out = latent(raw_audio=audio, keep_mask=np.ones((16, 16), np.uint8), steps=2, audio=False)   # the in-painting path's plain encode
    assert out.images[0].size == (32, 32)


# ================================================================ E. long-form
@pytest.mark.parametrize("backend", BACKENDS)
def test_longform_on_a_latent_pipeline(backend, monkeypatch):
    """One latent column is f * hop_length / sample_rate = 0.032 s; W = 16 latent columns = 0.512 s."""
    from audiodiffusion import longform
    dev = select(backend)
    latent, bare = _pipes(dev)
    assert longform.long_placement(latent, 1.0, 0.256) == (32, 8)                   # 31.25 columns -> 16 + 2*8; overlap 8 columns
    assert longform.long_placement(latent, 1.0, 0.256, circular=True) == (32, 8)
    assert longform.long_placement(latent, 1.2, 0.14) == (40, 12)                   # 37.5 columns; overlap 4.375 -> stride 12
    assert longform.long_placement(bare, 0.5, 0.128) == (32, 8)                     # image space: as it was
    (images, _), used = longform.generate_long(latent, 1.0, 0.256, steps=2, batch_size=2, audio=False, return_dict=False,
                                               generator=torch.Generator().manual_seed(1))
    assert (used["frames"], used["window_stride"]) == (32, 8) and abs(used["seconds"] - 1.024) < 1e-9
    assert abs(used["overlap_secs"] - 0.256) < 1e-9 and [i.size for i in images] == [(2 * used["frames"], 32)] * 2
    # spans: image columns at 62.5 per second, [int(6.25), int(17.5)) = [6, 17); latent column 8 = image columns 16, 17 is half
    # regenerated, so it is not kept
    keep = longform.span_keep_mask(latent, [(0.1, 0.28)])
    want = np.ones((16, 16), np.uint8)
    want[:, 3:9] = 0
    assert keep.dtype == np.uint8 and np.array_equal(keep, want)
    assert longform.span_keep_mask(latent, [(0.1, 0.28)], width=32).shape == (16, 32)
    assert np.array_equal(longform.span_keep_mask(bare, [(0.1, 0.15)])[0], np.array([1] * 6 + [0] * 3 + [1] * 7, np.uint8))
    # continue_track: 3000 samples cover 23 latent columns of 128 samples whole
    audio = (0.2 * np.random.default_rng(1).standard_normal(3000)).astype(np.float32)
    seen, real = {}, latent._denoise

    def spy(*a, **kw):
        seen.update(kw)
        seen["out"] = real(*a, **kw)
        return seen["out"]
    monkeypatch.setattr(latent, "_denoise", spy)
    calls = spy_sample_loop(monkeypatch)
    (images, floats), used = longform.continue_track(latent, audio, 1.0, 0.256, steps=2, audio=False, return_float=True,
                                                     generator=torch.Generator().manual_seed(5))
    assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
    assert (calls[0]["window_total_w"], calls[0]["window_stride"], calls[0]["B"]) == (32, 8, 1) and calls[0]["keep"] is not None
    assert (used["frames"], used["window_stride"], used["kept_columns"]) == (32, 8, 23) and abs(used["seconds"] - 1.024) < 1e-9
    z = seen["out"][0]
    assert torch.equal(z[..., :23], seen["known"][..., :23]) and not torch.equal(z[..., 23:], seen["known"][..., 23:])
    assert torch.equal(floats, latent.vqvae.decode_tiled(z, 16, 8, False, _in_scale=1 / 0.18215)["sample"])
    assert images[0].size == (64, 32)
