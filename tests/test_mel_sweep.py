"""Float64 sweep over the mel codec kernels (csrc/k_mel.hip) and both of their FFT engines, on both builds.

Five families, each driven through the C ABI (`adm_mel_forward_power`, `adm_mel_forward`, `adm_mel_inverse` with `stft_mag_out`):
  A. forward power: mel_stft_power_kernel<T> (radix-2 in LDS, any n_fft) and mel_stft2048_kernel<T, 1|2> (wave per frame, persistent groups)
  B. dB + quantisation: mel_db_u8_kernel<T> (one workgroup per spectrogram) and mel_db_u8_grid_kernel<T> (maximum from the STFT kernel)
  C. u8 -> power -> pinv GEMM (mel_u8_to_power_kernel, mel_pinv_gemm_kernel), and the known-block path of the NNLS kernels
  D. Griffin-Lim audio: gl_init / gl_istft_frames[2048] / gl_overlap_add / gl_stft_update[2048], n_iter 0..3
  E. the settings read once per process (ADM_MEL_FAST=0, ADM_MEL_OCC=1), one child process each

Every case names the branch it is meant to reach, recomputed here from the launcher's own rules, and `test_case_lists_reach_every_branch`
pins case -> branch, so an edit of a list cannot silently drop one. `adm_mel_last_variant()` (engine * 100 + element size * 10 + waves per
SIMD) must report the instantiation those rules give.

Truth. fp32 audio: float64 numpy (np.fft.rfft of the windowed, centre-padded frames, |.|^2, the fp32 filterbank weights widened). fp64 audio:
a radix-2 FFT written here in np.longdouble (eps < 2e-19 is asserted) and the float64 filterbank. The magnitude: the longdouble product of
the pinv matrix the Python layer uploads with the longdouble power, clipped at 0, compared as power (the rows no filter touches hold
pseudo-inverse rounding noise around 0, see tests/test_golden.py). Audio: oracle.mel.griffinlim(dtype=np.float64) from the kernel's own
magnitude and the injected phase.

Reference = the oracle's dtype-faithful path: oracle.mel.melspectrogram (fp32 audio), |oracle.mel.stft|^2 projected with the float64
filterbank (fp64 audio: the kernel documents fp64 weights there; oracle.mel.melspectrogram keeps float32 weights for float64 audio and sits
3e-8 from the truth, which would make the bar 1e8 u - its figure is printed as e_melspectrogram, not used), the float64 einsum of
oracle.mel.nnls(lbfgs=False) with the uploaded pinv, oracle.mel.griffinlim(dtype=np.float32).

Bars (the rule of tests/test_norm_sweep.py): e_kernel <= M * max(e_oracle, 4u); u = 2^-24 for fp32 audio and the fp32 audio output, 2^-53 for
fp64 spectrograms and the magnitude; M = 8 (the FFT runs in fp64 on both sides and is rounded once where librosa rounds; the mel taps and the
overlap-add have at most 65 and 4 terms), for the GEMM M = max(8, sqrt(n / log2 n)), n = n_mels. Two figures per tensor: g = max|d| / max|ref|
over the tensor, h = the same ratio per (clip, frame) column (spectrograms, magnitude) or per clip (audio), maximised, so a quiet clip or
a mostly padded frame cannot hide behind a loud one; a column that is exactly zero in the truth must be exactly zero. The ceilings of the
older tests stay as ceilings everywhere (2e-5 / 1e-10 forward, 1e-12 magnitude power, 1e-3 audio). Figures are printed (`MEL_SWEEP ...`)
before they are asserted; measured ratios: profiles/mel_accuracy.md.

Slices. Every forward case runs twice more with `slice_stride = n_samples + 37` inside a buffer whose gaps hold NaN (one read outside a
slice makes the output non-finite) and must come back bit-identical; every output sits between canaries that must come back intact.

No case is hip-only: the emulator runs every list in full (the largest case takes it half a second). The persistent case has B = CU count
+ 1 clips: 257 on the MI355X, 4 on the emulator (whose launcher reports 3 CUs), where every fast case already makes several trips.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                  # the child process of family E: no conftest has set the path up
    sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-diffusion_amd")]

import numpy as np
import pytest
import torch

from native_backend import BACKENDS, select
from oracle import mel as omel

LD = np.longdouble
U32, U64 = 2.0 ** -24, 2.0 ** -53
SR = 22050
TOP_DB = 80
GUARD = 64                                  # elements of canary on either side of a guarded output
CANARY, CANARY_U8 = -12345.5, 0xA5
CEIL_FWD = {np.float32: 2e-5, np.float64: 1e-10}    # tests/test_independent.py::test_kernel_melspectrogram_agrees_with_the_torch_stft_route
CEIL_MAG, CEIL_AUDIO = 1e-12, 1e-3                  # tests/test_mel.py
DTYPES = [np.float32, np.float64]
EMU_CUS = 3                                 # mel_cu_count() of the emulation build


# ---------------------------------------------------------------- figures and bars
def _margin(n):
    return max(8.0, math.sqrt(n / math.log2(n))) if n > 2 else 8.0


def _gh(got, ref, axis):
    """-> (g, h, zero_ok): g over the tensor, h per column (maximum over `axis` inside a column); zero_ok: every column that is exactly zero
    in `ref` is exactly zero in `got`."""
    d, r = np.abs(got.astype(ref.dtype) - ref), np.abs(ref)
    g = float(d.max() / r.max())
    cd, cr = d.max(axis=axis), r.max(axis=axis)
    live = cr > 0
    h = float((cd[live] / cr[live]).max())
    return g, h, bool((cd[~live] == 0).all())


def _figures(tag, what, got, truth, ref, axis, u, n=None, ceiling=None):
    """One record per compared tensor (a plain dict: family E sends them through JSON)."""
    assert got.shape == truth.shape == ref.shape, (tag, what, got.shape, truth.shape, ref.shape)
    assert np.isfinite(got).all(), (tag, what, "kernel output is not finite")
    assert np.isfinite(np.asarray(ref, np.float64)).all() and np.isfinite(np.asarray(truth, np.float64)).all(), (tag, what)
    gk, hk, zk = _gh(got, truth, axis)
    gr, hr, _ = _gh(ref, truth, axis)
    return dict(tag=tag, what=what, g_kernel=gk, h_kernel=hk, g_ref=gr, h_ref=hr, zero_ok=zk, u=u, margin=_margin(n) if n else 8.0,
                ceiling=ceiling)


def _judge(rec):
    fg, fh = max(rec["g_ref"], 4 * rec["u"]), max(rec["h_ref"], 4 * rec["u"])
    print(f"MEL_SWEEP {rec['tag']} out={rec['what']} g_kernel={rec['g_kernel']:.3e} g_oracle={rec['g_ref']:.3e} "
          f"g_ratio={rec['g_kernel'] / fg:.2f} h_kernel={rec['h_kernel']:.3e} h_oracle={rec['h_ref']:.3e} h_ratio={rec['h_kernel'] / fh:.2f} "
          f"bound={rec['margin']:.2f}" + (f" ceiling={rec['ceiling']:g}" if rec["ceiling"] else "") +
          "".join(f" {k}={v:.3e}" for k, v in rec.get("extra", {}).items()))
    assert rec["zero_ok"], (rec["tag"], rec["what"], "a column that is exactly zero in the truth is not zero")
    assert rec["g_kernel"] <= rec["margin"] * fg, (rec["tag"], rec["what"], "g", rec["g_kernel"], rec["margin"] * fg)
    assert rec["h_kernel"] <= rec["margin"] * fh, (rec["tag"], rec["what"], "h", rec["h_kernel"], rec["margin"] * fh)
    if rec["ceiling"]:
        assert rec["g_kernel"] <= rec["ceiling"], (rec["tag"], rec["what"], rec["g_kernel"], rec["ceiling"])


def _tag(backend, case, branch):
    return f"backend={backend} case={case} branch={branch}"


# ---------------------------------------------------------------- longdouble FFT (truth for fp64 audio)
def _fft_ld(x):
    """Radix-2 decimation-in-time FFT over the last axis in np.clongdouble; twiddles from cosl / sinl of a longdouble pi."""
    n = x.shape[-1]
    lg = n.bit_length() - 1
    assert 1 << lg == n
    rev = np.zeros(n, np.int64)
    for i in range(lg):
        rev |= ((np.arange(n) >> i) & 1) << (lg - 1 - i)
    x = x[..., rev].astype(np.clongdouble)
    pi = 4 * np.arctan(LD(1))
    s = 1
    while s < n:
        ang = -pi * np.arange(s, dtype=LD) / LD(s)
        w = np.cos(ang) + 1j * np.sin(ang)
        x = x.reshape(x.shape[:-1] + (n // (2 * s), 2, s))
        a, b = x[..., 0, :], x[..., 1, :] * w
        x = np.stack([a + b, a - b], axis=-2).reshape(x.shape[:-3] + (n,))
        s *= 2
    return x


def test_longdouble_is_wider_than_float64_and_the_fft_is_an_fft():
    assert np.finfo(LD).eps < 2e-19
    x = np.random.default_rng(0).standard_normal((3, 256))
    got, want = _fft_ld(x.astype(LD)), np.fft.fft(x, axis=-1)
    assert got.dtype == np.clongdouble
    assert np.abs(got.astype(np.complex128) - want).max() <= 1e-13 * np.abs(want).max()
    k = 5                                                                # a pure tone lands in one bin to longdouble precision
    pi = 4 * np.arctan(LD(1))
    tone = np.cos(2 * pi * k * np.arange(64, dtype=LD) / 64)
    T = _fft_ld(tone)
    T[k] -= 32
    T[64 - k] -= 32
    assert float(np.abs(T).max()) <= 64 * 8 * float(np.finfo(LD).eps)


# ---------------------------------------------------------------- inputs
def _batch(B, n, seed, dtype):
    """The tone-plus-noise signal of tests/test_mel.py, one seed per clip: clip 3k at amplitude 1, clip 3k+1 at 1e-3 (a quiet clip next to a
    loud one), clip 3k+2 silent in its second half."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050
    y = 0.1 * rng.standard_normal((B, n)) + 0.5 * np.sin(2 * np.pi * 440 * t) + 0.3 * np.sin(2 * np.pi * 3000 * t)
    y[1::3] *= 1e-3
    y[2::3, n // 2:] = 0.0
    return y.astype(dtype)


def _frames(y, n_fft, hop):
    yp = np.pad(y, ((0, 0), (n_fft // 2, n_fft // 2)))
    n_frames = 1 + (yp.shape[1] - n_fft) // hop
    idx = np.arange(n_fft)[None, :] + hop * np.arange(n_frames)[:, None]
    return yp[:, idx]                                                    # (B, n_frames, n_fft)


_TRUTH = {}


def _forward_truth(key, y, n_fft, hop, n_mels):
    """-> (truth, reference, melspectrogram-as-librosa) of shape (B, n_mels, n_frames); computed once per (case, precision, B)."""
    if key in _TRUTH:
        return _TRUTH[key]
    win = omel._hann(n_fft)
    B = y.shape[0]
    if y.dtype == np.float32:
        D = np.fft.rfft(win * _frames(y.astype(np.float64), n_fft, hop), axis=-1)
        fb = omel.mel_filterbank(SR, n_fft, n_mels, np.float32).astype(np.float64)
        truth = np.einsum("btf,mf->bmt", D.real ** 2 + D.imag ** 2, fb)
        ref = np.stack([omel.melspectrogram(y[b], SR, n_fft, hop, n_mels) for b in range(B)])
        assert ref.dtype == np.float32
        lib = ref
    else:
        fb64 = omel.mel_filterbank(SR, n_fft, n_mels, np.float64)
        fb = fb64.astype(LD)
        truth = np.empty((B, n_mels, 1 + y.shape[1] // hop), LD)
        for b0 in range(0, B, 8):                                        # chunks: a clongdouble is 32 bytes
            Dl = _fft_ld(win.astype(LD) * _frames(y[b0:b0 + 8].astype(LD), n_fft, hop))[..., :n_fft // 2 + 1]
            P = Dl.real ** 2 + Dl.imag ** 2
            truth[b0:b0 + 8] = np.matmul(fb[None], P.transpose(0, 2, 1))
        ref = np.stack([np.einsum("ft,mf->mt", np.abs(omel.stft(y[b], n_fft, hop)) ** 2.0, fb64) for b in range(B)])
        lib = np.stack([omel.melspectrogram(y[b], SR, n_fft, hop, n_mels) for b in range(B)])
        assert ref.dtype == lib.dtype == np.float64
    _TRUTH[key] = (truth, ref, lib)
    return _TRUTH[key]


# ---------------------------------------------------------------- driving the C ABI
def _native():
    from audiodiffusion import _native
    return _native, _native.lib()


_MELS = {}
_LOADED = [None]


def _drop_handles():
    for m in _MELS.values():
        m._free()
    _MELS.clear()


def _select(backend):
    """select(), after the cached handles of the other build have been destroyed by the library that made them."""
    if _LOADED[0] != backend:
        _drop_handles()
        _LOADED[0] = backend
    return select(backend)


@pytest.fixture(scope="module", autouse=True)
def _handles_die_with_the_module():
    yield
    _drop_handles()
    _LOADED[0] = None


def _mel(backend, fresh=False, dense_pinv=False, **cfg):
    """A `Mel` with its native handle, shared between the tests of one build unless `fresh`. dense_pinv: the `pinv` table handed to
    adm_mel_create is a dense positive matrix in place of the filterbank's pseudo-inverse, so that every bin gets a real magnitude. (No
    Slaney filter touches DC or Nyquist: with the true pseudo-inverse their magnitude is rounding noise, and what the inverse FFT does with
    their imaginary parts would never reach the audio.) The NNLS solver is off for such a handle: its start point is the magnitude."""
    from audiodiffusion.mel import Mel
    key = (backend, dense_pinv) + tuple(sorted(cfg.items()))
    if fresh or key not in _MELS:
        m = Mel(sample_rate=SR, top_db=TOP_DB, **cfg)
        if dense_pinv:
            true_pinv = np.linalg.pinv
            np.linalg.pinv = lambda a: np.random.default_rng(a.shape[0]).random(a.T.shape) + 0.25
            try:
                m._ensure_handle()
            finally:
                np.linalg.pinv = true_pinv
            m.nnls_max_iter = 0
        m._ensure_handle()
        if fresh:
            return m
        _MELS[key] = m
    return _MELS[key]


def _forward(dev, mel, y, image, stride_extra=0):
    """adm_mel_forward (image) / adm_mel_forward_power on y (B, n): clips `n + stride_extra` apart in a NaN-filled buffer, the output
    between canaries. -> (output (B, n_mels, n_frames) as numpy, adm_mel_last_variant())."""
    N, lib = _native()
    B, n = y.shape
    T = torch.float64 if y.dtype == np.float64 else torch.float32
    stride = n + stride_extra
    buf = torch.full((B * stride + 8,), float("nan"), dtype=T)
    buf[:B * stride].view(B, stride)[:, :n] = torch.from_numpy(y)
    buf = buf.to(dev)
    n_frames = 1 + n // mel.hop_length
    numel = B * mel.n_mels * n_frames
    whole = (torch.full((numel + 2 * GUARD,), CANARY_U8, dtype=torch.uint8) if image else
             torch.full((numel + 2 * GUARD,), CANARY, dtype=T)).to(dev)
    out = whole[GUARD:GUARD + numel]
    fn = lib.adm_mel_forward if image else lib.adm_mel_forward_power
    N.check(fn(mel._handle, C.c_void_p(buf.data_ptr()), int(y.dtype == np.float64), B, stride, n, C.c_void_p(out.data_ptr()),
               N.stream_for(buf)))
    variant = int(lib.adm_mel_last_variant())
    w = whole.cpu()
    can = CANARY_U8 if image else CANARY
    assert bool((w[:GUARD] == can).all()) and bool((w[-GUARD:] == can).all()), "the kernel wrote outside its output"
    return w[GUARD:GUARD + numel].view(B, mel.n_mels, n_frames).numpy().copy(), variant


def _cus(backend):
    return EMU_CUS if backend == "emu" else int(torch.cuda.get_device_properties(0).multi_processor_count)


# ================================================================ A. forward power
# (id, n_fft, hop, n_mels, n_frames, B, n_samples or None = hop * (n_frames - 1) + hop // 3); B = 0: CU count + 1
FWD_CASES = [
    ("g64-h16-m8", 64, 16, 8, 9, 3, None),                       # generic, the smallest n_fft adm_mel_create accepts, hop = n_fft / 4
    ("g64-h48-m8", 64, 48, 8, 9, 3, None),                       # a hop that does not divide n_fft
    ("g256-h64-m40", 256, 64, 40, 9, 3, None),                   # one bin per thread
    ("g1024-h256-m40", 1024, 256, 40, 9, 3, None),               # several bins per thread
    ("g1024-h48-short", 1024, 48, 40, 9, 3, 389),                 # n_samples < n_fft / 2: every frame is mostly padding
    ("g4096-h1024-m300", 4096, 1024, 300, 9, 3, None),           # the largest n_fft (81 952 B of LDS), a second pass over the mels
    ("f-h512-fr11-m256", 2048, 512, 256, 11, 3, None),           # fast: a ragged last group; <float, 2> / <double, 1>
    ("f-h512-fr16-m32", 2048, 512, 32, 16, 3, None),             # one full group of 16; <float, 2> / <double, 2>
    ("f-h128-fr17-m32", 2048, 128, 32, 17, 3, None),             # a full group plus one live frame
    ("f-h128-fr16-m256", 2048, 128, 256, 16, 3, None),           # <double, 1>: two full groups of 8
    ("f-h512-fr17-m256", 2048, 512, 256, 17, 3, None),           # <double, 1>: two full groups of 8 plus one live frame
    ("f-persist-fr17-m32", 2048, 128, 32, 17, 0, None),          # more groups than CUs: the second trip, a prefetch into another clip
]
FWD_IDS = [c[0] for c in FWD_CASES]


def _fast_lds_bytes(nw, tsz, n_mels, nnz):
    """lds_bytes() of mel_forward_power_impl."""
    return 16 * nw * 16 * 65 + tsz * n_mels * 2 * nw + 4 * (3 * n_mels + 2) + tsz * nnz


def _nnz(n_fft, n_mels):
    from audiodiffusion.mel import slaney_filter_taps
    return int(slaney_filter_taps(SR, n_fft, n_mels)[1].sum())


def _fwd_variant(n_fft, n_mels, dtype, nnz, fast_env=1, occ_env=2):
    """What adm_mel_last_variant() must report: the rules of mel_fast_path() and mel_forward_power_impl()."""
    tsz = 8 if dtype == np.float64 else 4
    if not (n_fft == 2048 and fast_env):
        return 100 + tsz * 10 + 1
    occ = 2 if (occ_env == 2 and _fast_lds_bytes(8, tsz, n_mels, nnz) <= 160 * 1024) else 1
    return 200 + tsz * 10 + occ


def _lds_class(n_fft):
    """fft_smem() of the generic kernels against 64 KiB: "under", "over" with the complex frame alone "at" 64 KiB (n_fft = 4096)."""
    smem = 16 * n_fft + 8 * (n_fft // 2 + 1 + 3)
    return "under" if smem <= 64 * 1024 else ("frame-at-total-over" if 16 * n_fft == 64 * 1024 else "over")


def _fwd_branch(case, dtype, cus=256):
    cid, n_fft, hop, n_mels, n_frames, B, n_samples = case
    B = B or cus + 1
    v = _fwd_variant(n_fft, n_mels, dtype, _nnz(n_fft, n_mels))
    t = "f32" if dtype == np.float32 else "f64"
    if v < 200:
        return (f"generic-{t}-n{n_fft}-lds-{_lds_class(n_fft)}-hop{'div' if n_fft % hop == 0 else 'nodiv'}-melpass{-(-n_mels // 256)}"
                + ("-padded" if n_samples is not None and n_samples < n_fft // 2 else ""))
    fr = 8 * (v % 10)
    gpc = -(-n_frames // fr)
    trips = -(-(gpc * B) // min(gpc * B, cus))
    last = n_frames - (gpc - 1) * fr
    return f"fast-{t}-w{v % 10}-groups{gpc}-last{'full' if last == fr else last}-trips{trips}"


FWD_BRANCHES = {    # case -> (fp32 branch, fp64 branch) on the MI355X's 256 CUs
    "g64-h16-m8": ("generic-f32-n64-lds-under-hopdiv-melpass1", "generic-f64-n64-lds-under-hopdiv-melpass1"),
    "g64-h48-m8": ("generic-f32-n64-lds-under-hopnodiv-melpass1", "generic-f64-n64-lds-under-hopnodiv-melpass1"),
    "g256-h64-m40": ("generic-f32-n256-lds-under-hopdiv-melpass1", "generic-f64-n256-lds-under-hopdiv-melpass1"),
    "g1024-h256-m40": ("generic-f32-n1024-lds-under-hopdiv-melpass1", "generic-f64-n1024-lds-under-hopdiv-melpass1"),
    "g1024-h48-short": ("generic-f32-n1024-lds-under-hopnodiv-melpass1-padded", "generic-f64-n1024-lds-under-hopnodiv-melpass1-padded"),
    "g4096-h1024-m300": ("generic-f32-n4096-lds-frame-at-total-over-hopdiv-melpass2",
                         "generic-f64-n4096-lds-frame-at-total-over-hopdiv-melpass2"),
    "f-h512-fr11-m256": ("fast-f32-w2-groups1-last11-trips1", "fast-f64-w1-groups2-last3-trips1"),
    "f-h512-fr16-m32": ("fast-f32-w2-groups1-lastfull-trips1", "fast-f64-w2-groups1-lastfull-trips1"),
    "f-h128-fr17-m32": ("fast-f32-w2-groups2-last1-trips1", "fast-f64-w2-groups2-last1-trips1"),
    "f-h128-fr16-m256": ("fast-f32-w2-groups1-lastfull-trips1", "fast-f64-w1-groups2-lastfull-trips1"),
    "f-h512-fr17-m256": ("fast-f32-w2-groups2-last1-trips1", "fast-f64-w1-groups3-last1-trips1"),
    "f-persist-fr17-m32": ("fast-f32-w2-groups2-last1-trips3", "fast-f64-w2-groups2-last1-trips3"),
}


def _fwd_case(cid):
    return FWD_CASES[FWD_IDS.index(cid)]


def _fwd_audio(case, dtype, backend):
    cid, n_fft, hop, n_mels, n_frames, B, n_samples = case
    B = B or _cus(backend) + 1
    n = n_samples if n_samples is not None else hop * (n_frames - 1) + hop // 3
    assert 1 + n // hop == n_frames
    return _batch(B, n, 1000 + FWD_IDS.index(cid), dtype)


def _forward_records(backend, dev, case, dtype, fast_env=1, occ_env=2):
    """Runs one case of A and -> (its figure record, the power spectrogram, the audio); structural properties are asserted here."""
    cid, n_fft, hop, n_mels, n_frames, B, _ = case
    y = _fwd_audio(case, dtype, backend)
    mel = _mel(backend, x_res=n_frames, y_res=n_mels, n_fft=n_fft, hop_length=hop)
    want_v = _fwd_variant(n_fft, n_mels, dtype, int(mel.filter_taps[1].sum()), fast_env, occ_env)
    got, v = _forward(dev, mel, y, image=False)
    assert v == want_v, (cid, v, want_v)
    if v >= 200 and B == 0:                                              # the case that is about the persistent loop really loops
        fr = 8 * (v % 10)
        assert -(-n_frames // fr) * y.shape[0] > _cus(backend)
    again, _ = _forward(dev, mel, y, image=False)
    assert np.array_equal(got, again), (cid, "two runs differ")
    strided, _ = _forward(dev, mel, y, image=False, stride_extra=37)
    assert np.isfinite(strided).all(), (cid, "a read outside a slice (the gaps hold NaN)")
    assert np.array_equal(got, strided), (cid, "slice_stride != n_samples changes the result")
    truth, ref, lib = _forward_truth((cid, np.dtype(dtype).name, y.shape[0]), y, n_fft, hop, n_mels)
    branch = _fwd_branch(case, dtype, _cus(backend)) if (fast_env, occ_env) == (1, 2) else f"variant{v}"
    rec = _figures(_tag(backend, f"{cid}-{'f32' if dtype == np.float32 else 'f64'}", branch), "melspec", got, truth, ref, 1,
                   U32 if dtype == np.float32 else U64, ceiling=CEIL_FWD[dtype])
    if dtype == np.float64:
        rec["extra"] = {"e_melspectrogram": _gh(lib, truth, 1)[0]}
    rec["variant"] = v
    return rec, got, y


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("cid", FWD_IDS)
def test_forward_power(backend, dtype, cid):
    case = _fwd_case(cid)
    dev = _select(backend)
    rec, got, y = _forward_records(backend, dev, case, dtype)
    assert (got >= 0).all()
    _judge(rec)


# ================================================================ B. dB and quantisation
def _quantise(S, dtype):
    """Mel.audio_slice_to_image's dB conversion and quantisation of one power spectrogram, in `dtype`: -> (u8 image, q + 0.5 before the cast)."""
    log_S = omel.power_to_db(S.astype(dtype), top_db=TOP_DB)
    q = ((log_S + TOP_DB) * 255 / TOP_DB).clip(0, 255) + 0.5
    assert q.dtype == dtype
    return q.astype(np.uint8), q


def _check_image(backend, cid, img, S, dtype):
    """img (B, m, t) from adm_mel_forward against the quantisation of the kernel's own power S: equal except within 1e-3 of a rounding edge."""
    assert img.shape[1] * img.shape[2] * img.shape[0] >= 100
    near_total = 0
    for b in range(img.shape[0]):
        want, _ = _quantise(S[b], dtype)
        _, q64 = _quantise(S[b], np.float64)
        near = np.abs(q64 - np.rint(q64)) < 1e-3
        near_total += int(near.sum())
        diff = img[b].astype(int) - want.astype(int)
        assert (diff[~near] == 0).all(), (cid, b, "pixels away from a rounding edge differ", np.argwhere((diff != 0) & ~near)[:4])
        assert np.abs(diff).max() <= 1, (cid, b)
    share = near_total / img.size
    print(f"MEL_SWEEP backend={backend} case={cid} dtype={np.dtype(dtype).name} out=image pixels={img.size} near_edge_share={share:.4f}")
    assert share <= 0.02, (cid, share)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("cid", FWD_IDS)
def test_db_and_quantisation(backend, dtype, cid):
    case = _fwd_case(cid)
    dev = _select(backend)
    _, n_fft, hop, n_mels, n_frames, _, _ = case
    y = _fwd_audio(case, dtype, backend)
    mel = _mel(backend, x_res=n_frames, y_res=n_mels, n_fft=n_fft, hop_length=hop)
    S, _ = _forward(dev, mel, y, image=False)
    img, v = _forward(dev, mel, y, image=True)
    assert v == _fwd_variant(n_fft, n_mels, dtype, int(mel.filter_taps[1].sum()))
    strided, _ = _forward(dev, mel, y, image=True, stride_extra=37)
    assert np.array_equal(img, strided)
    _check_image(backend, cid, img, S, dtype)
    # each clip is normalised by its OWN maximum: the loud clip, the quiet one (1e-3) and the half-silent one all reach 255 ...
    assert all((img[b] == 255).any() for b in range(min(3, img.shape[0])))
    # ... and the frames of clip 2 that lie wholly in its silent half sit on the top_db floor: pixels that are exactly 0
    t_silent = -(-(y.shape[1] // 2 + n_fft // 2) // hop)                 # first frame that starts inside the silent half
    if t_silent < n_frames:
        assert (img[2][:, t_silent:] == 0).all()
    assert t_silent < n_frames or hop in (48, 128), "only the short case and the hop-128 cases have no such frame"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n_fft", [256, 2048], ids=["generic", "fast"])
def test_silence_gives_white_and_a_reused_handle_gives_what_a_fresh_one_gives(backend, dtype, n_fft):
    dev = _select(backend)
    cfg = dict(x_res=17, y_res=32, n_fft=n_fft, hop_length=n_fft // 4)
    n = (n_fft // 4) * 16 + 5
    used = _mel(backend, fresh=True, **cfg)
    img, _ = _forward(dev, used, np.zeros((1, n), dtype), image=True)
    assert (img == 255).all()
    # a loud batch of 1, then a quieter batch of 3 on the same handle: the per-spectrogram maxima are reset and their buffer grows
    y = _batch(3, n, 77, dtype)
    _forward(dev, used, (8 * y[:1]).astype(dtype), image=True)
    got, _ = _forward(dev, used, (0.05 * y).astype(dtype), image=True)
    fresh = _mel(backend, fresh=True, **cfg)
    want, _ = _forward(dev, fresh, (0.05 * y).astype(dtype), image=True)
    assert np.array_equal(got, want)
    S, _ = _forward(dev, used, (0.05 * y).astype(dtype), image=False)
    _check_image(backend, f"reuse-{n_fft}", got, S, dtype)
    # ... and a still quieter batch of the same size: no growth now, the maxima of the run before must not survive
    got, _ = _forward(dev, used, (1e-3 * y).astype(dtype), image=True)
    want, _ = _forward(dev, _mel(backend, fresh=True, **cfg), (1e-3 * y).astype(dtype), image=True)
    assert np.array_equal(got, want)


# ================================================================ C. u8 -> power -> pinv GEMM
# (id, n_fft, n_frames, n_mels): n_bins = n_fft / 2 + 1 in {33, 1025, 2049} (1 / 17 / 33 row tiles of 64, the last one ragged: 33, 1, 1 rows),
# n_frames on both sides of the 64-wide column tile, n_mels = K in chunks of 16 with a ragged last chunk (8, 40 = 2 * 16 + 8, 100 = 6 * 16 + 4)
GEMM_CASES = [
    ("b33-f5-m8", 64, 5, 8),
    ("b33-f65-m40", 64, 65, 40),
    ("b1025-f64-m100", 2048, 64, 100),
    ("b1025-f65-m8", 2048, 65, 8),
    ("b2049-f5-m100", 4096, 5, 100),
    ("b2049-f64-m40", 4096, 64, 40),
]
GEMM_IDS = [c[0] for c in GEMM_CASES]
GEMM_BRANCHES = {
    "b33-f5-m8": "rowtiles1-last33-coltiles1-last5-kchunks1-last8",
    "b33-f65-m40": "rowtiles1-last33-coltiles2-last1-kchunks3-last8",
    "b1025-f64-m100": "rowtiles17-last1-coltiles1-last64-kchunks7-last4",
    "b1025-f65-m8": "rowtiles17-last1-coltiles2-last1-kchunks1-last8",
    "b2049-f5-m100": "rowtiles33-last1-coltiles1-last5-kchunks7-last4",
    "b2049-f64-m40": "rowtiles33-last1-coltiles1-last64-kchunks3-last8",
}


def _gemm_branch(case):
    _, n_fft, n_frames, n_mels = case
    nb = n_fft // 2 + 1
    t = lambda n, w: f"{-(-n // w)}-last{n - (-(-n // w) - 1) * w}"      # noqa: E731
    return f"rowtiles{t(nb, 64)}-coltiles{t(n_frames, 64)}-kchunks{t(n_mels, 16)}"


def _gemm_images(n_mels, n_frames, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 256, (n_mels, n_frames), dtype=np.uint8), np.zeros((n_mels, n_frames), np.uint8),
                     np.full((n_mels, n_frames), 255, np.uint8)])


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("cid", GEMM_IDS)
def test_magnitude_gemm(backend, cid):
    _select(backend)
    case = GEMM_CASES[GEMM_IDS.index(cid)]
    _, n_fft, n_frames, n_mels = case
    mel = _mel(backend, x_res=n_frames, y_res=n_mels, n_fft=n_fft, hop_length=n_fft // 4, n_iter=0)
    mel.nnls_max_iter = 0                                                # the start point everywhere: the GEMM alone
    imgs = _gemm_images(n_mels, n_frames, 500 + GEMM_IDS.index(cid))
    phase = np.random.default_rng(9).random((3, n_fft // 2 + 1, n_frames))
    _, mag = mel.images_to_audios(imgs, init_phase=phase, return_magnitude=True)      # (B, n_bins, n_frames)
    _, mag2 = mel.images_to_audios(imgs, init_phase=phase, return_magnitude=True)
    assert np.array_equal(mag, mag2) and (mag >= 0).all() and mel.last_nnls_iterations == 0
    S_ld = LD(10) ** (LD(1) / LD(10) * (imgs.astype(LD) * TOP_DB / 255 - TOP_DB))
    truth = np.clip(np.matmul(mel.pinv.astype(LD)[None], S_ld), 0, None)
    assert (truth[0] == 0).any(), "the random image must leave bins clipped to exactly 0"
    S64 = omel.db_to_power(imgs.astype("float") * TOP_DB / 255 - TOP_DB)
    ref = np.stack([np.clip(np.einsum("fm,mt->ft", mel.pinv, S64[b], optimize=True), 0, None) for b in range(3)])
    rec = _figures(_tag(backend, cid, _gemm_branch(case)), "mag^2", mag ** 2, truth, ref, 1, U64, n=n_mels, ceiling=CEIL_MAG)
    rec["zero_ok"] = True                                                # (no column of a magnitude is all zero)
    _judge(rec)
    # where the truth is clipped with room (the unclipped product is below -1e3 u of the column's maximum) the kernel clips too
    raw = np.matmul(mel.pinv.astype(LD)[None], S_ld)
    deep = raw < -1e3 * U64 * truth.max(axis=1, keepdims=True)
    assert deep.any() and (mag[deep] == 0).all()


@pytest.mark.parametrize("backend", BACKENDS)
def test_nnls_converged_block_next_to_an_iterating_one(backend):
    """Two NNLS column blocks (librosa's blocking: 32768 / n_mels = 512 columns) of which scipy's L-BFGS-B returns the first as it is
    (nit = 0: an all-zero image, S = 1e-8) and iterates on the second (nit = 5 on the oracle; found by a search over sample rates and
    filterbank sizes around NNLS_ITERATING of tests/test_mel.py): the `known_blk` path of mel_nnls_diff_kernel / mel_nnls_pg_kernel."""
    from PIL import Image

    from audiodiffusion.mel import Mel
    _select(backend)
    sr, cols = 200, 512
    cfg = dict(sample_rate=sr, x_res=cols + 6, y_res=64, n_fft=128, hop_length=32, n_iter=0)
    rng = np.random.default_rng(sr + 64)
    img = np.zeros((64, cols + 6), np.uint8)
    img[:, cols:] = rng.integers(0, 256, (64, 6), dtype=np.uint8)
    info = []
    ref_mag = omel.Mel(**cfg).image_to_stft_magnitude(Image.fromarray(img), info)
    assert [d["nit"] == 0 for d in info] == [True, False], info          # the regime this test is about
    mine = Mel(**cfg)
    assert mine.n_mels * 8 * cols == 2 ** 18
    phase = rng.random((1, 65, cols + 6))
    mine.nnls_max_iter = 0
    with pytest.warns(UserWarning, match="projected gradient"):          # the start point alone does not satisfy the rule here
        _, start = mine.images_to_audios(img[None], init_phase=phase, return_magnitude=True)
    assert mine.last_nnls_iterations == 0
    mine.nnls_max_iter = 4000
    _, mag = mine.images_to_audios(img[None], init_phase=phase, return_magnitude=True)
    assert np.array_equal(mag[0][:, :cols], start[0][:, :cols]), "the converged block must come back as the start point, bit for bit"
    assert not np.array_equal(mag[0][:, cols:], start[0][:, cols:])
    assert np.abs(mag[0][:, :cols] ** 2 - ref_mag[:, :cols] ** 2).max() <= CEIL_MAG * max(1.0, np.abs(ref_mag ** 2).max())
    # the other block: the bars of tests/test_mel.py::test_nnls_solver_where_lbfgsb_iterates
    S = omel.db_to_power(img[:, cols:].astype(float) * TOP_DB / 255 - TOP_DB)
    A = omel.mel_filterbank(sr, 128, 64, np.float64)
    f = lambda X: 0.5 * np.sum((A @ X - S) ** 2) / S.size  # noqa: E731
    f_hip, f_ref, f_start = f(mag[0][:, cols:] ** 2), f(ref_mag[:, cols:] ** 2), f(start[0][:, cols:] ** 2)
    print(f"MEL_SWEEP backend={backend} case=nnls-two-blocks pg_start={mine.last_nnls_pg_start:.3e} pg={mine.last_nnls_pg:.3e} "
          f"iterations={mine.last_nnls_iterations} f_kernel={f_hip:.6e} f_scipy={f_ref:.6e} f_start={f_start:.6e}")
    assert mine.last_nnls_pg_start > 1e-5 and mine.last_nnls_iterations > 0
    assert mine.last_nnls_pg <= 1e-5
    assert (mag[0] >= 0).all()
    assert f_hip <= f_ref * (1 + 1e-3), (f_hip, f_ref)
    assert f_hip < f_start


# ================================================================ D. Griffin-Lim audio
# (id, n_fft, n_frames, n_mels, dense): hop = n_fft / 4; B = 2 images with different injected phases; every case runs n_iter = 0 (irfft and
# overlap-add alone), 1 (the update without momentum), 2 (the momentum term), 3 (the whole reb / tprev / spare rotation). dense = 0: the
# magnitude of the filterbank's pseudo-inverse, with bins clipped to exactly 0 (`0 / tiny`, `s2 > 0`) and DC / Nyquist at rounding noise;
# dense = 1: a dense positive `pinv` table (see _mel), so DC and Nyquist carry a real magnitude and an injected imaginary part
GL_CASES = [
    ("gl-g64-f9", 64, 9, 8, 0),              # generic engine, the smallest n_fft
    ("gl-g256-f9", 256, 9, 40, 0),
    ("gl-g256-f9-dense", 256, 9, 40, 1),
    ("gl-g4096-f5", 4096, 5, 40, 0),         # the largest n_fft (81 952 B of LDS)
    ("gl-f2048-f4", 2048, 4, 32, 0),         # fast engine: one full workgroup of 4 frames
    ("gl-f2048-f5", 2048, 5, 32, 0),         # a second workgroup with 1 live wave
    ("gl-f2048-f5-dense", 2048, 5, 32, 1),
    ("gl-f2048-f6", 2048, 6, 32, 0),         # ... with 2
]
GL_IDS = [c[0] for c in GL_CASES]
GL_BRANCHES = {
    "gl-g64-f9": "generic-n64-lds-under-zeros", "gl-g256-f9": "generic-n256-lds-under-zeros",
    "gl-g256-f9-dense": "generic-n256-lds-under-dc-nyquist", "gl-g4096-f5": "generic-n4096-lds-frame-at-total-over-zeros",
    "gl-f2048-f4": "fast-wg1-live4-zeros", "gl-f2048-f5": "fast-wg2-live1-zeros", "gl-f2048-f5-dense": "fast-wg2-live1-dc-nyquist",
    "gl-f2048-f6": "fast-wg2-live2-zeros",
}
N_ITERS = [0, 1, 2, 3]


def _gl_branch(case, fast_env=1):
    _, n_fft, n_frames, _, dense = case
    kind = "-dc-nyquist" if dense else "-zeros"
    if n_fft == 2048 and fast_env:
        return f"fast-wg{-(-n_frames // 4)}-live{n_frames - (-(-n_frames // 4) - 1) * 4}" + kind
    return f"generic-n{n_fft}-lds-{_lds_class(n_fft)}" + kind


def _gl_inputs(case):
    cid, n_fft, n_frames, n_mels, _ = case
    rng = np.random.default_rng(700 + GL_IDS.index(cid))
    imgs = rng.integers(0, 256, (2, n_mels, n_frames), dtype=np.uint8)
    imgs[1] = (imgs[1] // 4 + 150).astype(np.uint8)                      # a second image of another character
    return imgs, rng.random((2, n_fft // 2 + 1, n_frames))


def _gl_records(backend, case, n_iter, fast_env=1):
    cid, n_fft, n_frames, n_mels, dense = case
    hop = n_fft // 4
    mel = _mel(backend, dense_pinv=bool(dense), x_res=n_frames, y_res=n_mels, n_fft=n_fft, hop_length=hop, n_iter=n_iter)
    imgs, phase = _gl_inputs(case)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", UserWarning)                     # (a dense table is no NNLS solution, and the wrapper says so)
        audio, mag = mel.images_to_audios(imgs, init_phase=phase, return_magnitude=True)
        audio2 = mel.images_to_audios(imgs, init_phase=phase)
    assert np.array_equal(audio, audio2), (cid, "two runs differ")
    assert audio.dtype == np.float32 and audio.shape == (2, hop * (n_frames - 1))
    if dense:
        assert (mag[:, 0] > 1e-3 * mag.max()).all() and (mag[:, -1] > 1e-3 * mag.max()).all(), "DC and Nyquist must carry a real magnitude"
    else:
        assert (mag[0] == 0).any(), "the random image must give a magnitude with exactly-zero bins (0 / tiny, s2 > 0)"
    truth = np.stack([omel.griffinlim(mag[b], n_iter, hop, n_fft, init_phase=phase[b], dtype=np.float64) for b in range(2)])
    ref = np.stack([omel.griffinlim(mag[b], n_iter, hop, n_fft, init_phase=phase[b], dtype=np.float32) for b in range(2)])
    assert truth.dtype == np.float64 and ref.dtype == np.float32
    return _figures(_tag(backend, f"{cid}-it{n_iter}", _gl_branch(case, fast_env)), "audio", audio, truth, ref, 1, U32, ceiling=CEIL_AUDIO)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_iter", N_ITERS)
@pytest.mark.parametrize("cid", GL_IDS)
def test_griffin_lim_audio(backend, cid, n_iter):
    _select(backend)
    _judge(_gl_records(backend, GL_CASES[GL_IDS.index(cid)], n_iter))


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n_fft", [256, 2048], ids=["generic", "fast"])
def test_inverse_scratch_grows_with_the_batch(backend, n_fft):
    """B = 1 and then B = 3 on one handle (the cap_inv growth path) give what a fresh handle gives."""
    _select(backend)
    cfg = dict(x_res=6, y_res=32, n_fft=n_fft, hop_length=n_fft // 4, n_iter=2)
    rng = np.random.default_rng(31)
    imgs, phase = rng.integers(0, 256, (3, 32, 6), dtype=np.uint8), rng.random((3, n_fft // 2 + 1, 6))
    used = _mel(backend, fresh=True, **cfg)
    first = used.images_to_audios(imgs[:1], init_phase=phase[:1])
    got, gmag = used.images_to_audios(imgs, init_phase=phase, return_magnitude=True)
    want, wmag = _mel(backend, fresh=True, **cfg).images_to_audios(imgs, init_phase=phase, return_magnitude=True)
    assert np.array_equal(got, want) and np.array_equal(gmag, wmag) and np.array_equal(got[:1], first)


# ================================================================ E. settings that are read once per process
# ADM_MEL_FAST and ADM_MEL_OCC are function-local statics of the launcher: a fresh process each. The child (this file run as a program) runs
# the 2048 cases of A and D under the setting, checks adm_mel_last_variant() and prints its figure records as JSON; the bars are applied here.
CHILD_MODES = {"fast0": {"ADM_MEL_FAST": "0"}, "occ1": {"ADM_MEL_OCC": "1"}}
CHILD_MARK = "MEL_SWEEP_CHILD_JSON "


def _child_settings(mode):
    return (0, 2) if mode == "fast0" else (1, 1)


def _child_variant(mode, dtype):
    tsz = 8 if dtype == np.float64 else 4
    return 100 + tsz * 10 + 1 if mode == "fast0" else 200 + tsz * 10 + 1


def _child_main(backend, mode):
    dev = _select(backend)
    fast_env, occ_env = _child_settings(mode)
    recs = []
    for case in FWD_CASES:
        if case[1] != 2048:
            continue
        for dtype in DTYPES:
            rec, _, _ = _forward_records(backend, dev, case, dtype, fast_env, occ_env)
            assert rec["variant"] == _child_variant(mode, dtype), (case[0], rec["variant"])
            recs.append(rec)
    for case in GL_CASES:
        if case[1] != 2048:
            continue
        for n_iter in (N_ITERS if mode == "fast0" else [2]):             # ADM_MEL_OCC does not reach the Griffin-Lim kernels: one pass
            recs.append(_gl_records(backend, case, n_iter, fast_env))
    print(CHILD_MARK + json.dumps(recs), flush=True)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", sorted(CHILD_MODES))
def test_settings_read_once_per_process(backend, mode):
    _select(backend)                                                     # (builds the emulation library before the child needs it)
    env = dict(os.environ, **CHILD_MODES[mode])
    run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", backend, mode], env=env, capture_output=True, text=True,
                         timeout=600)
    assert run.returncode == 0, (run.returncode, run.stdout[-3000:], run.stderr[-3000:])
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith(CHILD_MARK)]
    assert len(lines) == 1
    recs = json.loads(lines[0][len(CHILD_MARK):])
    fwd = [r for r in recs if r["what"] == "melspec"]
    assert len(fwd) == 2 * sum(1 for c in FWD_CASES if c[1] == 2048)
    assert {r["variant"] for r in fwd} == {_child_variant(mode, d) for d in DTYPES}
    assert len(recs) - len(fwd) == sum(1 for c in GL_CASES if c[1] == 2048) * (len(N_ITERS) if mode == "fast0" else 1)
    for r in recs:
        r["tag"] = f"setting={mode} " + r["tag"]
        _judge(r)


# ================================================================ the lists reach every branch
def test_case_lists_reach_every_branch():
    """Recomputes the launcher's rules for every case and pins case -> branch: a case deleted from a list, or edited onto another branch,
    fails here. Then the branches every family must reach."""
    assert {c[0]: (_fwd_branch(c, np.float32), _fwd_branch(c, np.float64)) for c in FWD_CASES} == FWD_BRANCHES
    assert {c[0]: _gemm_branch(c) for c in GEMM_CASES} == GEMM_BRANCHES
    assert {c[0]: _gl_branch(c) for c in GL_CASES} == GL_BRANCHES
    for cus in (EMU_CUS, 256):
        f = [_fwd_branch(c, d, cus) for c in FWD_CASES for d in DTYPES]
        for need in ("generic-f32", "generic-f64", "fast-f32-w2", "fast-f64-w2", "fast-f64-w1",      # engine, T, 4 or 8 waves
                     "-n64-lds-under", "-n1024-lds-under", "-n4096-lds-frame-at-total-over",         # LDS under / at / over 64 KiB
                     "hopnodiv", "melpass2", "-padded", "lastfull-", "last1-", "last11-", "last3-"): # ragged, full, full + 1
            assert any(need in b for b in f), (cus, need)
        assert any(int(b.rsplit("trips", 1)[1]) > 1 for b in f if b.startswith("fast")), cus  # more than one persistent trip
    # <float, 1> needs ADM_MEL_OCC=1 (family E); with it, and with ADM_MEL_FAST=0, the remaining instantiations
    nnz = _nnz(2048, 32)
    assert {_fwd_variant(2048, 32, d, nnz, 1, 1) for d in DTYPES} == {241, 281}
    assert {_fwd_variant(2048, 32, d, nnz, 0, 2) for d in DTYPES} == {141, 181}
    assert {_fwd_variant(c[1], c[3], d, _nnz(c[1], c[3])) for c in FWD_CASES for d in DTYPES} == {141, 181, 242, 281, 282}
    # the 8-wave image of fp64 audio at 256 mels is what exceeds the LDS, with the handle's real tap count
    nnz = _nnz(2048, 256)
    assert nnz == 2032 and _fast_lds_bytes(8, 4, 256, nnz) <= 160 * 1024 < _fast_lds_bytes(8, 8, 256, nnz)
    g = "".join(GEMM_BRANCHES.values())
    for need in ("coltiles1-last5", "coltiles1-last64", "coltiles2-last1", "rowtiles1-", "rowtiles17-", "rowtiles33-", "kchunks1-last8",
                 "kchunks3-last8", "kchunks7-last4"):
        assert need in g, need
    assert set(GL_BRANCHES.values()) >= {"fast-wg1-live4-zeros", "fast-wg2-live1-zeros", "fast-wg2-live2-zeros", "fast-wg2-live1-dc-nyquist",
                                         "generic-n64-lds-under-zeros", "generic-n256-lds-under-dc-nyquist",
                                         "generic-n4096-lds-frame-at-total-over-zeros"}


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child_main(sys.argv[2], sys.argv[3])
