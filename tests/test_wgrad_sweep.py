"""Float64 sweep over the fp32 convolution weight-gradient kernels (k_conv_wgrad.hip: nine kernels, two reduce kernels) and the small-channel
convolution backward kernels (k_backward.hip: conv_small_cin_wgrad_kernel<1..4>, conv_small_cout_dgrad_kernel, conv_small_cout_wgrad_kernel<1..4>),
on both builds.

Reference. The same operation in float64 torch on the CPU, from the SAME fp32 inputs. The GroupNorm scale / shift handed to a kernel are computed
here in float64 and rounded to fp32 once; the reference applies those fp32 values in float64, a = silu(x * sc + sh), so no statistics error enters
a comparison. The fp32 torch result of the same graph supplies e_torch_fp32.

Bars (the rule of tests/test_norm_sweep.py). g = max|d| / max|ref| against float64, and g_kernel <= M(n) * max(g_torch_fp32, 4u), u = 2^-24,
M(n) = max(8, sqrt(n / log2 n)), n = the length of the output's reduction: N * Ho * Wo for every dW, `split` for the reduce kernels driven
directly, 9 * Cout for da of the small-cout kernel. The 1e-4 of tests/test_backward.py::test_conv_wgrad stays as a ceiling on every dW. Where the
reference is structurally zero (a tap that only ever meets padding: every non-centre tap of a 3x3 filter on a 1x1 image) the kernel's value must
be exactly 0. Figures are printed (`WGRAD_SWEEP ...`) before they are asserted; measured ratios: profiles/wgrad_accuracy.md.

Dispatch. Every case asserts what `adm_last_wgrad_variant` reports — kernel, reduce kernel, split, tiles_per_block — against `_predict`, the
launcher's rule restated here; option "wgrad_path" reaches the kernels the heuristic never picks (conv_wgrad_sp_kernel, conv_wgrad_kernel<1,1>,
conv_wgrad_kernel<3,1> at a pipelined shape). `test_case_lists_reach_every_branch` asserts that the lists reach every kernel, reduce branch and
tiles_per_block class, so an edit of a list cannot silently drop one. The sweep runs with "conv_bf16" at its default (fp32).

Slices. A destination is a view into a canary-filled buffer that must come back untouched around the view; a batch-strided source is a channel
slice of a wider NaN-filled buffer, so one read outside the slice makes dW non-finite.

The small kernels add into dW with fp32 atomics over n: no run-to-run bit identity is asserted for them.

Not covered: the `n_ptiles >= 65536` division branch of the pipelined kernels (gigabytes of input); the bf16 routes (tests/test_conv_bf16*.py).
`conv_wgrad: patch too large for LDS` cannot be reached: the patch of a 64-pixel tile is largest for a 1x1 output (64 images x 3x3, PS = 577
floats per channel, 107 KiB with the dy tile) and every output dim below 16 / 4 must be a power of two, which is checked first.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from native_backend import BACKENDS, select

U = 2.0 ** -24
CANARY = -12345.5
GUARD = 64                                  # floats of canary in front of and behind a guarded buffer (keeps its alignment)
GROUPS, EPS = 8, 1e-5

GEN31, GEN32, GEN11, PF3, PF3F, PF1, PF1F, SP, SP8 = 310, 320, 110, 1300, 1301, 1100, 1101, 2304, 2308
FP32_KERNELS = {GEN31, GEN32, GEN11, PF3, PF3F, PF1, PF1F, SP, SP8}
FAMILY = {SP8: "sp8", SP: "sp", PF3: "pf3", PF3F: "pf3", PF1: "pf1", PF1F: "pf1", GEN31: "gen", GEN32: "gen", GEN11: "gen"}


# ---------------------------------------------------------------- figures and bars
def _margin(n):
    return max(8.0, math.sqrt(n / math.log2(n))) if n > 2 else 8.0


def _judge(entry, what, got, ref64, ref32, n, tag, ceiling=None):
    """got (kernel, fp32) against ref64 under M(n) * max(error of ref32, 4u); the figures are printed before they are asserted."""
    got = got.detach().cpu()
    ref64, ref32 = ref64.detach(), ref32.detach()
    assert got.shape == ref64.shape == ref32.shape, (entry, what, tag, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), (entry, what, tag, "kernel output is not finite")
    assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(ref64).all()), (entry, what, tag, "reference is not finite")
    den = float(ref64.abs().max()) + 1e-300
    e_kernel, e_torch = float((got.double() - ref64).abs().max()) / den, float((ref32.double() - ref64).abs().max()) / den
    floor = max(e_torch, 4 * U)
    bound = _margin(n) * floor
    print(f"WGRAD_SWEEP {tag} entry={entry} out={what} n={n} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} "
          f"ratio={e_kernel / floor:.2f} bound={_margin(n):.2f}")
    assert e_kernel <= bound, (entry, what, tag, e_kernel, e_torch, bound)
    if ceiling is not None:
        assert e_kernel <= ceiling, (entry, what, tag, e_kernel, ceiling)


def _tag(backend, case, branch):
    return f"backend={backend} case={case} branch={branch}"


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _guarded(init, dev, off=0):
    """-> (view, whole): `init` copied to float offset GUARD + off of a canary-filled device buffer; the view is what the kernel is given."""
    n = init.numel()
    whole = torch.full((n + 2 * GUARD + 4,), CANARY, dtype=torch.float32)
    whole[GUARD + off:GUARD + off + n] = init.reshape(-1)
    whole = whole.to(dev)
    view = whole[GUARD + off:GUARD + off + n]
    assert (view.data_ptr() - whole.data_ptr()) == 4 * (GUARD + off) and whole.data_ptr() % 64 == 0
    return view, whole


def _guard_intact(whole, n, off=0):
    w = whole.cpu()
    return bool((w[:GUARD + off] == CANARY).all()) and bool((w[GUARD + off + n:] == CANARY).all())


def _ops():
    from audiodiffusion import _native, ops
    return _native, ops


class _Options:
    """Sets process-wide options for one case and puts the defaults back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        N, _ = _ops()
        for k, v in self.kv.items():
            N.check(N.lib().adm_set_option(k.encode(), v))

    def __exit__(self, *exc):
        N, _ = _ops()
        for k in self.kv:
            N.check(N.lib().adm_set_option(k.encode(), 0))


# ================================================================ the launcher's rule, restated
def _cdiv(a, b):
    return -(-a // b)


def _out_dims(H, W, ks, stride, up, pad_lo):
    Hi, Wi = (2 * H, 2 * W) if up else (H, W)
    if stride == 1:
        return Hi, Wi, Hi, Wi
    return Hi, Wi, (Hi + (2 if pad_lo else 1) - ks) // stride + 1, (Wi + (2 if pad_lo else 1) - ks) // stride + 1


def _predict(c):
    """-> dict(kernel, reduce, split, tpb, n_ptiles, NI, n): launch_conv_wgrad's choices for case c (conv_bf16 off)."""
    Ct = c["C1"] + c["C2"]
    _, _, Ho, Wo = _out_dims(c["H"], c["W"], c["ks"], c["stride"], c["up"], c["pad_lo"])
    TW, TH = min(Wo, 16), min(Ho, 4)
    NI = 64 // (TW * TH)
    n_ptiles = _cdiv(Wo, TW) * _cdiv(Ho, TH) * _cdiv(c["N"], NI)
    CB = 32 if c["ks"] == 3 else 128
    pairs = _cdiv(c["Cout"], 128) * _cdiv(Ct, CB)
    split = _cdiv(768, pairs)
    if c["cap"] > 0:
        split = min(split, c["cap"])
    split = max(1, min(split, n_ptiles))
    tpb = _cdiv(n_ptiles, split)
    split = _cdiv(n_ptiles, tpb)
    fast = c["up"] == 0 and c["C1"] % CB == 0 and Ct % CB == 0 and c["Cout"] % 128 == 0
    PE = NI * ((TH - 1) * c["stride"] + c["ks"]) * ((TW - 1) * c["stride"] + c["ks"])
    use_pf, use_sp, use_sp8 = c["path"] < 3, c["path"] < 2, c["path"] < 1
    if use_pf and use_sp and fast and c["stride"] == 1 and c["ks"] == 3 and TW == 16 and TH == 4:
        kernel = SP8 if use_sp8 else SP
    elif use_pf and c["stride"] == 1 and c["ks"] == 3 and PE <= 128:
        kernel = PF3F if fast else PF3
    elif use_pf and c["ks"] == 1:
        kernel = PF1F if fast else PF1
    elif c["ks"] == 3:
        kernel = GEN31 if c["stride"] == 1 else GEN32
    else:
        kernel = GEN11
    return dict(kernel=kernel, reduce=9 if c["ks"] == 3 else 1, split=split, tpb=tpb, n_ptiles=n_ptiles, NI=NI, n=c["N"] * Ho * Wo,
                pairs=pairs, Ho=Ho, Wo=Wo, ragged_last=n_ptiles % tpb != 0)


def _branch(c):
    p = _predict(c)
    return f"k{p['kernel']}-r{p['reduce']}-split{p['split']}-tpb{p['tpb']}"


def wc(id, N, C1, C2, H, W, Cout, ks=3, stride=1, up=0, pad_lo=1, gn=0, act=0, path=0, cap=0, **extra):
    """One weight-gradient case. extra: xscale (input scale), bs=(extra channels of the wide x1 buffer, of x2's), acc (accumulate onto a prefilled
    dW), dw_off (float offset of the dW view in its guarded buffer)."""
    if ks == 1:
        pad_lo = 0
    return dict(id=id, N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, ks=ks, stride=stride, up=up, pad_lo=pad_lo, gn=gn, act=act, path=path, cap=cap,
                xscale=extra.pop("xscale", 1.0), bs=extra.pop("bs", None), acc=extra.pop("acc", 0), dw_off=extra.pop("dw_off", 0), **extra)


# ---- A. kernel selection
SEL_CASES = [
    wc("sp8-4x16", 2, 32, 0, 4, 16, 128, gn=1, act=1),
    wc("sp-4x16", 2, 32, 0, 4, 16, 128, gn=1, act=1, path=1),
    wc("sp8-8x32-nogn", 1, 32, 0, 8, 32, 128),
    wc("sp-8x32-nogn", 1, 32, 0, 8, 32, 128, path=1),
    wc("pf3f-4x8-two-images", 4, 32, 0, 4, 8, 128, gn=1, act=1),
    wc("pf3f-by-option-4x16", 2, 32, 0, 4, 16, 128, gn=1, act=1, path=2),
    wc("pf3-upfold", 2, 32, 0, 2, 4, 128, up=1, gn=1, act=1),
    wc("pf3-upfold-8x8", 2, 32, 0, 4, 4, 128, up=1),
    wc("pf3-cout32", 2, 32, 0, 4, 8, 32, gn=1, act=1),
    wc("pf3-cout160", 2, 32, 0, 4, 16, 160, gn=1, act=1),
    wc("pf3-seam-c40+24", 2, 40, 24, 4, 16, 128),
    wc("pf3-ct40-ragged-chunk", 2, 40, 0, 4, 8, 128, gn=1, act=1),
    wc("gen31-4x4", 5, 32, 0, 4, 4, 64, gn=1, act=1),
    wc("gen31-2x2", 5, 32, 0, 2, 2, 32, gn=1, act=1),
    wc("gen31-1x1", 70, 32, 0, 1, 1, 32, gn=1, act=1),
    wc("gen31-2x16", 3, 32, 0, 2, 16, 32, gn=1),
    wc("gen31-8x4", 2, 32, 0, 8, 4, 32, act=1),
    wc("gen31-by-option-4x16", 2, 32, 0, 4, 16, 128, gn=1, act=1, path=3),
    wc("gen31-by-option-4x8-concat", 3, 32, 32, 4, 8, 128, gn=1, act=1, path=3),
] + [
    wc(f"gen32-{h}x{h}-pad{pad}", n, 32, 0, h, h, 32, stride=2, pad_lo=pad, gn=g, act=g)
    for (h, n, g) in ((16, 2, 1), (4, 5, 0), (2, 70, 1)) for pad in (1, 0)
] + [
    wc(f"{name}-{h}x{w}", n, c1, c2, h, w, 128, ks=1, gn=g, act=g, path=path)
    for (name, c1, c2, g, path) in (("pf1f", 128, 0, 1, 0), ("pf1-gn", 64, 32, 1, 0), ("gen11", 64, 32, 1, 3))
    for (h, w, n) in ((1, 1, 70), (2, 2, 5), (8, 8, 3), (16, 32, 1))
]

# ---- B. pipeline depth and tiling: five pixel tiles, max_split 0 / 3 / 2 / 1 -> 1 / 2 / 3 / 5 tiles per workgroup (cap 2: 3 + 2, a short last
# workgroup); one image (sp8, sp) or two (prefetch) per tile, GroupNorm on: the per-image scale row switches between a workgroup's tiles
_DEPTH = [("sp8", dict(N=5, C1=32, C2=0, H=4, W=16, Cout=128), 0), ("sp", dict(N=5, C1=32, C2=0, H=4, W=16, Cout=128), 1),
          ("pf3f", dict(N=10, C1=32, C2=0, H=4, W=8, Cout=128), 0), ("pf3", dict(N=10, C1=32, C2=0, H=4, W=8, Cout=160), 0),
          ("pf1f", dict(N=10, C1=128, C2=0, H=4, W=8, Cout=128, ks=1), 0), ("pf1", dict(N=10, C1=64, C2=32, H=4, W=8, Cout=128, ks=1), 0)]
DEPTH_CASES = [wc(f"{name}-5tiles-cap{cap}", gn=1, act=1, path=path, cap=cap, **shape) for (name, shape, path) in _DEPTH for cap in (0, 3, 2, 1)] + [
    wc("sp8-ho6", 2, 32, 0, 6, 16, 128, gn=1, act=1, cap=2),
    wc("sp-ho6", 2, 32, 0, 6, 16, 128, gn=1, act=1, cap=2, path=1),
    wc("sp8-wo24", 2, 32, 0, 4, 24, 128, gn=1, act=1, cap=1),
    wc("sp-wo24", 2, 32, 0, 4, 24, 128, gn=1, act=1, cap=3, path=1),
    wc("pf3f-wo24-ho6", 1, 32, 0, 6, 24, 128, gn=1, act=1, cap=2, path=2),
    wc("pf3f-n3-two-per-tile", 3, 32, 0, 4, 8, 128, gn=1, act=1, cap=1),
    wc("pf3-n3-two-per-tile", 3, 32, 0, 4, 8, 96, gn=1, act=1),
    wc("gen31-n5-four-per-tile", 5, 32, 0, 4, 4, 32, gn=1, act=1, cap=1),
    wc("pf1f-n5-four-per-tile", 5, 128, 0, 4, 4, 128, ks=1, gn=1, act=1, cap=1),
    wc("pf1-n5-sixteen-per-tile", 5, 64, 0, 2, 2, 128, ks=1, gn=1, act=1),
    wc("gen32-n5-sixteen-per-tile", 5, 32, 0, 4, 4, 32, stride=2, gn=1, act=1),
    wc("sp8-cout256", 2, 32, 0, 4, 16, 256, gn=1, act=1, cap=1),
    wc("sp-cout256", 2, 32, 0, 4, 16, 256, gn=1, act=1, path=1),
    wc("sp8-chunks-in-x2", 2, 64, 32, 4, 16, 128, gn=1, act=1, cap=1),
    wc("sp-chunks-in-x2", 2, 64, 32, 4, 16, 128, gn=1, act=1, cap=1, path=1),
    wc("pf3f-chunks-in-x2", 3, 64, 32, 4, 8, 128, gn=1, act=1, cap=1),
    # the longest serial chain the size limit allows: one workgroup adds all 64 tiles of four 32x32 images (n = 4096) into its accumulators
    wc("sp8-32x32-one-workgroup", 4, 32, 0, 32, 32, 128, gn=1, act=1, cap=1),
    wc("sp-32x32-one-workgroup", 4, 32, 0, 32, 32, 128, gn=1, act=1, cap=1, path=1),
    wc("pf3f-32x32-one-workgroup", 4, 32, 0, 32, 32, 128, gn=1, act=1, cap=1, path=2),
    wc("gen31-32x32-one-workgroup", 4, 32, 0, 32, 32, 128, gn=1, act=1, cap=1, path=3),
    wc("gen32-32x32-one-workgroup", 4, 32, 0, 32, 32, 32, stride=2, gn=1, act=1, cap=1),
    wc("pf1f-32x32-one-workgroup", 4, 128, 0, 32, 32, 128, ks=1, gn=1, act=1, cap=1),
]

# ---- C. arguments no other test passes
ARG_CASES = [
    wc("bstride-sp8", 3, 32, 32, 4, 16, 128, gn=1, act=1, cap=2, bs=(5, 9)),
    wc("bstride-sp", 3, 32, 32, 4, 16, 128, gn=1, act=1, cap=2, bs=(5, 9), path=1),
    wc("bstride-pf3f", 4, 32, 32, 4, 8, 128, gn=1, act=1, cap=1, bs=(3, 8)),
    wc("bstride-pf3", 4, 32, 32, 4, 8, 96, gn=1, act=1, cap=1, bs=(3, 8)),
    wc("bstride-pf1f", 4, 128, 128, 4, 8, 128, ks=1, cap=1, bs=(2, 7)),
    wc("bstride-gen31", 5, 32, 32, 4, 4, 32, gn=1, act=1, bs=(1, 6)),
    wc("bstride-gen32", 2, 32, 32, 8, 8, 32, stride=2, pad_lo=0, bs=(4, 2)),
    wc("accumulate-reduce9", 2, 32, 0, 4, 16, 128, gn=1, act=1, acc=1),
    wc("accumulate-reduce9-unaligned", 2, 32, 0, 4, 8, 32, acc=1, dw_off=3),
    wc("accumulate-reduce", 3, 128, 0, 8, 8, 128, ks=1, gn=1, act=1, acc=1),
    wc("accumulate-reduce-unaligned", 3, 64, 32, 8, 8, 128, ks=1, acc=1, dw_off=2),
] + [wc(f"dw-offset{o}-reduce9", 2, 32, 0, 4, 8, 32, gn=1, act=1, dw_off=o) for o in (1, 2, 3)] + [
    wc(f"dw-offset{o}-reduce", 2, 64, 32, 4, 8, 128, ks=1, gn=1, act=1, dw_off=o) for o in (1, 2, 3)
] + [
    wc("gn-without-act-sp8", 2, 32, 0, 4, 16, 128, gn=1),
    wc("gn-without-act-pf3f", 2, 32, 0, 4, 8, 128, gn=1),
    wc("gn-without-act-gen32", 2, 32, 0, 8, 8, 32, stride=2, gn=1),
    wc("gn-without-act-pf1", 2, 64, 0, 4, 8, 128, ks=1, gn=1),
    wc("preact-120-sp8", 2, 32, 0, 4, 16, 128, act=1, xscale=40.0),
    wc("preact-120-sp", 2, 32, 0, 4, 16, 128, act=1, xscale=40.0, path=1),
    wc("preact-120-pf3f", 2, 32, 0, 4, 8, 128, act=1, xscale=40.0),
    wc("preact-120-pf1", 2, 64, 0, 4, 8, 128, ks=1, act=1, xscale=40.0),
    wc("preact-120-gen31", 2, 32, 0, 4, 4, 32, act=1, xscale=40.0),
]

WG_CASES = SEL_CASES + DEPTH_CASES + ARG_CASES


@functools.lru_cache(maxsize=8)
def _wg_reference(N, C1, C2, H, W, Cout, ks, stride, up, pad_lo, gn, act, xscale):
    """Inputs (fp32) and references of one shape, computed once and shared by every kernel path / split that runs it.
    -> x (N, Ct, H, W), dy, (sc, sh) fp32 or None, dW in float64, dW by fp32 torch, structural-zero mask."""
    Ct = C1 + C2
    x = _randn((N, Ct, H, W), 11, xscale).clamp_(-120.0, 120.0)
    _, _, Ho, Wo = _out_dims(H, W, ks, stride, up, pad_lo)
    dy = _randn((N, Cout, Ho, Wo), 12)
    gnp = None
    if gn:
        gamma, beta = _randn((Ct,), 13).double() * 0.5 + 1.0, _randn((Ct,), 14).double()
        xg = x.double().view(N, GROUPS, -1)
        mean, var = xg.mean(-1, keepdim=True), xg.var(-1, unbiased=False, keepdim=True)
        rstd = (var + EPS).rsqrt().expand(N, GROUPS, Ct // GROUPS).reshape(N, Ct)
        mean = mean.expand(N, GROUPS, Ct // GROUPS).reshape(N, Ct)
        sc = (gamma * rstd).float()
        sh = (beta - mean * gamma * rstd).float()
        gnp = (sc.contiguous(), sh.contiguous())

    def grad(dt):
        a = x.to(dt)
        if gnp is not None:
            a = a * gnp[0].to(dt)[:, :, None, None] + gnp[1].to(dt)[:, :, None, None]
        if act:
            a = F.silu(a)
        if up:
            a = F.interpolate(a, scale_factor=2.0, mode="nearest")
        return _conv_dw(a, dy.to(dt), Cout, ks, stride, pad_lo)

    ones = torch.ones((N, Ct, H, W), dtype=torch.float64)
    if up:
        ones = F.interpolate(ones, scale_factor=2.0, mode="nearest")
    zero_mask = _conv_dw(ones, torch.ones_like(dy, dtype=torch.float64), Cout, ks, stride, pad_lo) == 0
    return x, dy, gnp, grad(torch.float64), grad(torch.float32), zero_mask


def _conv_dw(a, dy, Cout, ks, stride, pad_lo):
    """Weight gradient of conv(a) by autograd (dW does not depend on the weights)."""
    w = torch.zeros((Cout, a.shape[1], ks, ks), dtype=a.dtype, requires_grad=True)
    if ks == 1:
        y = F.conv2d(a, w)
    elif stride == 2 and not pad_lo:
        y = F.conv2d(F.pad(a, (0, 1, 0, 1)), w, stride=2)
    else:
        y = F.conv2d(a, w, stride=stride, padding=1)
    assert y.shape == dy.shape, (y.shape, dy.shape)
    y.backward(dy)
    return w.grad.detach()


def _shape_key(c):
    return tuple(c[k] for k in ("N", "C1", "C2", "H", "W", "Cout", "ks", "stride", "up", "pad_lo", "gn", "act", "xscale"))


def _sources(c, x, dev):
    """x1, x2 and the bstride arguments for case c: plain tensors, or channel slices of wider NaN-filled buffers."""
    C1, C2 = c["C1"], c["C2"]
    if c["bs"] is None:
        return x[:, :C1].contiguous().to(dev), (x[:, C1:].contiguous().to(dev) if C2 else None), {}
    e1, e2 = c["bs"]
    lead1, lead2 = e1 // 2, e2 // 2
    w1 = torch.full((c["N"], C1 + e1, c["H"], c["W"]), float("nan"))
    w1[:, lead1:lead1 + C1] = x[:, :C1]
    w2 = torch.full((c["N"], C2 + e2, c["H"], c["W"]), float("nan"))
    w2[:, lead2:lead2 + C2] = x[:, C1:]
    w1, w2 = w1.to(dev), w2.to(dev)
    x1, x2 = w1[:, lead1:lead1 + C1], w2[:, lead2:lead2 + C2]
    return x1, x2, dict(x1_bstride=x1.stride(0), x2_bstride=x2.stride(0))


def _run_wgrad(c, dev, x, dy, gnp, out=None):
    _, ops = _ops()
    x1, x2, bs = _sources(c, x, dev)
    gn = (gnp[0].to(dev), gnp[1].to(dev)) if gnp is not None else None
    with _Options(wgrad_path=c["path"], wgrad_max_split=c["cap"]):
        dW = ops.conv2d_wgrad(x1, dy.to(dev), c["Cout"], c["ks"], x2=x2, up=bool(c["up"]), stride=c["stride"], pad_lo=c["pad_lo"], gn=gn,
                              act=bool(c["act"]), accumulate=bool(c["acc"]), out=out, **bs)
        got = ops.last_wgrad_variant()
    p = _predict(c)
    assert got == (p["kernel"], p["reduce"], p["split"], p["tpb"]), (c["id"], got, p)
    return dW


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", WG_CASES, ids=[c["id"] for c in WG_CASES])
def test_wgrad(backend, c):
    dev = select(backend)
    x, dy, gnp, ref64, ref32, zero_mask = _wg_reference(*_shape_key(c))
    numel = ref64.numel()
    pre = _randn(ref64.shape, 15, float(ref64.abs().max()) * 0.5) if c["acc"] else torch.full(ref64.shape, CANARY)
    view, whole = _guarded(pre, dev, c["dw_off"])
    dW = _run_wgrad(c, dev, x, dy, gnp, out=view)
    assert dW.data_ptr() == view.data_ptr()
    assert _guard_intact(whole, numel, c["dw_off"]), (c["id"], "a store outside dW")
    got = dW.cpu().view(ref64.shape)
    if c["acc"]:
        ref64, ref32 = pre.double() + ref64, pre + ref32
    else:
        assert bool((got[zero_mask] == 0).all()), (c["id"], "a tap that only meets padding must be exactly 0")
    if c["xscale"] != 1.0:
        assert float(x.min()) <= -100 and float(x.max()) >= 100
    _judge("adm_conv2d_wgrad", "dW", got, ref64, ref32, _predict(c)["n"], _tag(backend, c["id"], _branch(c)), ceiling=1e-4)


@pytest.mark.parametrize("backend", BACKENDS)
def test_wgrad_sp_and_sp8_share_inputs(backend):
    """The four-wave and the eight-wave kernel on the same inputs, each against float64 (no bit identity between them: waves 4..7 of the
    eight-wave kernel own taps 5..8, so neither the tap split nor the staging order is the same — only the per-element sums are)."""
    dev = select(backend)
    a, b = [c for c in SEL_CASES if c["id"] in ("sp8-4x16", "sp-4x16")]
    assert _shape_key(a) == _shape_key(b) and (_predict(a)["kernel"], _predict(b)["kernel"]) == (SP8, SP)
    x, dy, gnp, ref64, ref32, _ = _wg_reference(*_shape_key(a))
    for c in (a, b):
        _judge("adm_conv2d_wgrad", "dW", _run_wgrad(c, dev, x, dy, gnp).cpu(), ref64, ref32, _predict(c)["n"],
               _tag(backend, c["id"] + "-shared", _branch(c)), ceiling=1e-4)


@pytest.mark.parametrize("backend", BACKENDS)
def test_wgrad_path_option(backend):
    """An unknown "wgrad_path" is rejected and not recorded: the launcher keeps the path it had."""
    select(backend)
    N, ops = _ops()
    c = dict(SEL_CASES[0])
    dev = select(backend)
    x, dy, gnp, _, _, _ = _wg_reference(*_shape_key(c))
    try:
        for bad in (-1, 4, 99):
            assert N.lib().adm_set_option(b"wgrad_path", bad) != 0
            assert b"wgrad_path" in N.lib().adm_last_error()
        _run_wgrad(c, dev, x, dy, gnp)                                     # still the heuristic: sp8
        N.check(N.lib().adm_set_option(b"wgrad_path", 2))
        assert N.lib().adm_set_option(b"wgrad_path", 7) != 0
        ops.conv2d_wgrad(x[:, :c["C1"]].contiguous().to(dev), dy.to(dev), c["Cout"], 3)
        assert ops.last_wgrad_variant()[0] == PF3F                         # still 2: no software-pipelined kernel
    finally:
        N.check(N.lib().adm_set_option(b"wgrad_path", 0))


# ================================================================ D. impulse identity
def _impulse_positions(c):
    """(n, co, oy, ox): the four corners, both sides of the tile seams, the last pixel of a ragged tile, the last image, first / last cout of a
    cout tile."""
    p = _predict(c)
    Ho, Wo, N, Cout = p["Ho"], p["Wo"], c["N"], c["Cout"]
    pos = [(0, 0, 0, 0), (0, 1, 0, Wo - 1), (0, 2, Ho - 1, 0), (N - 1, Cout - 1, Ho - 1, Wo - 1), (N - 1, 0, Ho // 2, Wo // 2)]
    if Wo > 16:
        pos += [(0, 5, 1, 15), (N - 1, 127 % Cout, 1, 16)]
    if Ho > 4:
        pos += [(0, 7, 3, Wo - 1), (N - 1, 31, 4, 0)]
    if Cout > 128:
        pos += [(0, 127, 0, 0), (N - 1, 128, Ho - 1, Wo - 1)]
    return sorted(set(pos))


IMPULSE_CASES = [
    wc("sp8", 2, 32, 32, 6, 24, 256, cap=1),                    # ragged in x and y (Wo = 24, Ho = 6), seams at ox 15|16 and oy 3|4, two cout tiles
    wc("sp", 2, 32, 32, 6, 24, 256, cap=1, path=1),
    wc("pf3f", 3, 32, 32, 8, 8, 128, cap=2),                    # two images per tile, ragged last tile (N = 3)
    wc("pf3f-by-option", 2, 32, 0, 6, 24, 128, cap=2, path=2),
    wc("pf3-seam-c40+24", 3, 40, 24, 8, 8, 96, cap=1),
    wc("pf3-upfold", 3, 32, 0, 4, 4, 160, up=1, cap=1),
    wc("pf3-upfold-wide", 1, 32, 0, 4, 12, 32, up=1, cap=1),    # 8x24 output through the fold: seams in x and y
    wc("gen31-4x4", 5, 32, 0, 4, 4, 160),
    wc("gen31-1x1", 70, 32, 0, 1, 1, 32),
    wc("gen31-2x16", 3, 40, 0, 2, 16, 32),
    wc("gen31-by-option", 2, 32, 0, 6, 24, 128, cap=1, path=3),
    wc("gen32-pad1", 2, 32, 0, 12, 48, 160, stride=2, pad_lo=1, cap=1),
    wc("gen32-pad0", 2, 32, 0, 12, 48, 160, stride=2, pad_lo=0, cap=1),
    wc("gen32-4x4-pad1", 5, 32, 0, 4, 4, 32, stride=2, pad_lo=1),
    wc("gen32-4x4-pad0", 5, 32, 0, 4, 4, 32, stride=2, pad_lo=0),
    wc("gen32-2x2-pad1", 70, 32, 0, 2, 2, 32, stride=2, pad_lo=1),
    wc("gen32-2x2-pad0", 70, 32, 0, 2, 2, 32, stride=2, pad_lo=0),
    wc("pf1f", 3, 128, 128, 8, 8, 256, ks=1, cap=2),
    wc("pf1", 3, 64, 32, 6, 24, 160, ks=1, cap=1),
    wc("gen11", 3, 64, 32, 6, 24, 160, ks=1, cap=1, path=3),
    wc("pf1-1x1", 70, 64, 0, 1, 1, 128, ks=1),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", IMPULSE_CASES, ids=[c["id"] for c in IMPULSE_CASES])
def test_wgrad_impulse(backend, c):
    """dy = one 1.0 at (n, co, oy, ox), no GroupNorm, no activation: row co of dW is the input patch under that pixel bit for bit (0 in the
    padding) and every other row is exactly 0 — no tolerance."""
    dev = select(backend)
    _, ops = _ops()
    N, Ct, ks, s, pad = c["N"], c["C1"] + c["C2"], c["ks"], c["stride"], c["pad_lo"]
    p = _predict(c)
    x = _randn((N, Ct, c["H"], c["W"]), 21)
    a = F.interpolate(x, scale_factor=2.0, mode="nearest") if c["up"] else x
    ap = F.pad(a, (pad, ks, pad, ks))                             # zero padding on every side the window can reach
    x1, x2, _ = _sources(c, x, dev)
    dy = torch.zeros((N, c["Cout"], p["Ho"], p["Wo"]), device=dev)
    with _Options(wgrad_path=c["path"], wgrad_max_split=c["cap"]):
        for (n, co, oy, ox) in _impulse_positions(c):
            dy[n, co, oy, ox] = 1.0
            dW = ops.conv2d_wgrad(x1, dy, c["Cout"], ks, x2=x2, up=bool(c["up"]), stride=s, pad_lo=pad).cpu()
            dy[n, co, oy, ox] = 0.0
            assert ops.last_wgrad_variant() == (p["kernel"], p["reduce"], p["split"], p["tpb"]), (c["id"], ops.last_wgrad_variant(), p)
            want = torch.zeros_like(dW)
            want[co] = ap[n, :, oy * s:oy * s + ks, ox * s:ox * s + ks]
            bad = (dW != want).nonzero()
            assert bad.numel() == 0, (c["id"], (n, co, oy, ox), "first mismatch (co, c, ky, kx)", bad[0].tolist(), len(bad))


# ================================================================ E. the reduce kernels through adm_wgrad_reduce
def rc(id, split, taps, numel, ws_off=0, dw_off=0, acc=0, device_only=False):
    return dict(id=id, split=split, taps=taps, numel=numel, ws_off=ws_off, dw_off=dw_off, acc=acc, device_only=device_only)


def _reduce_branch(c):
    """wgrad_reduce_kernel: float4 loads or the scalar fallback (per block: the ragged last float4), the four-chain loop, float4 or scalar
    stores, grid-stride trips; wgrad_reduce9_kernel: full / ragged last 64-pair block, trips."""
    acc = f"acc{c['acc']}"
    if c["taps"] == 9:
        M = c["numel"] // 9
        blocks = _cdiv(M, 64)
        return f"reduce9-{'ragged' if M % 64 else 'full'}-trips{_cdiv(blocks, 16384)}-waves{min(4, c['split'])}-{acc}"
    vec = c["numel"] % 4 == 0 and c["ws_off"] % 4 == 0
    dvec = c["taps"] == 1 and c["dw_off"] % 4 == 0
    chains = "chains4" if vec and c["split"] >= 13 else "chains1"
    tail = "+tail" if (c["split"] - 1) % 16 >= 4 or c["split"] < 13 else ""      # the one-chain loop after the four-chain one
    blocks = _cdiv(c["numel"], 256)
    return (f"reduce-{'vec' if vec else 'scalar'}-{chains}{tail if vec else ''}-{'dvec' if dvec and c['numel'] % 4 == 0 else 'dscalar'}"
            f"-trips{_cdiv(blocks, 4096)}-{acc}")


SPLITS = [1, 2, 3, 4, 5, 12, 13, 16, 17, 29]
REDUCE_CASES = [rc(f"t1-split{s}", s, 1, 1028, acc=s % 2) for s in SPLITS] + [
    rc(f"t9-split{s}-m100", s, 9, 900, dw_off=s % 4, acc=(s + 1) % 2) for s in SPLITS
] + [
    rc("t1-ragged-numel1027-split3", 3, 1, 1027), rc("t1-ragged-numel1027-split17-acc", 17, 1, 1027, acc=1),
    rc("t1-ragged-numel1026-dw1", 5, 1, 1026, dw_off=1, acc=1),
    rc("t1-ws-offset1-split3", 3, 1, 1028, ws_off=1), rc("t1-ws-offset1-split29-acc", 29, 1, 1028, ws_off=1, acc=1),
    rc("t1-dw-offset1-split13", 13, 1, 1028, dw_off=1), rc("t1-dw-offset2-split4-acc", 4, 1, 1028, dw_off=2, acc=1),
    rc("t1-dw-offset3-split16", 16, 1, 1028, dw_off=3), rc("t1-dw-offset1-ws-offset1-acc", 12, 1, 1028, ws_off=1, dw_off=1, acc=1),
    rc("t1-numel3", 5, 1, 3, acc=1), rc("t1-numel256-split13-acc0", 13, 1, 256), rc("t1-numel256-split13-acc1", 13, 1, 256, acc=1),
    rc("t9-m64-full", 13, 9, 576, acc=1), rc("t9-m128-full-acc0", 5, 9, 1152), rc("t9-m1", 3, 9, 9, acc=1),
    rc("t9-m191-ws-offset1", 17, 9, 191 * 9, ws_off=1, dw_off=1),
    # both grid-stride loops take a second trip: more than 4096 blocks of 256 floats, more than 16384 blocks of 64 (cout, cin) pairs
    rc("t1-grid-stride", 2, 1, 4096 * 256 + 3 * 256 + 8, acc=1),
    rc("t9-grid-stride", 2, 9, 9 * (16384 * 64 + 2 * 64 + 5), acc=1),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", REDUCE_CASES, ids=[c["id"] for c in REDUCE_CASES])
def test_wgrad_reduce(backend, c):
    """Random slabs against their float64 sum in the [tap][cout*cin] -> (cout, cin, tap) order; canaries around dW."""
    dev = select(backend)
    _, ops = _ops()
    split, taps, numel = c["split"], c["taps"], c["numel"]
    M = numel // taps
    ws = _randn((split * numel,), 31)
    prefill = _randn((numel,), 32) if c["acc"] else torch.full((numel,), CANARY)
    slabs = ws.view(split, numel)

    def order(t):
        return t.view(taps, M).t().reshape(-1)

    ref64 = order(slabs.double().sum(0)) + (prefill.double() if c["acc"] else 0.0)
    ref32 = order(slabs.sum(0)) + (prefill if c["acc"] else 0.0)
    wsd = torch.zeros(split * numel + 4, dtype=torch.float32, device=dev)
    assert wsd.data_ptr() % 16 == 0
    wsv = wsd[c["ws_off"]:c["ws_off"] + split * numel]
    wsv.copy_(ws)
    view, whole = _guarded(prefill, dev, c["dw_off"])
    ops.wgrad_reduce(wsv, split, numel, view, accumulate=bool(c["acc"]), taps=taps)
    assert ops.last_wgrad_variant()[1] == (9 if taps == 9 else 1)
    assert _guard_intact(whole, numel, c["dw_off"]), (c["id"], "a store outside dW")
    _judge("adm_wgrad_reduce", "dW", view.cpu(), ref64, ref32, split, _tag(backend, c["id"], _reduce_branch(c)))
    if split == 1 and not c["acc"]:
        assert torch.equal(view.cpu(), order(slabs[0])), (c["id"], "one slab: a transposing copy")


# ================================================================ F. the small-channel kernels
def sc_case(id, kind, Ch, Cother, N, H, W, gn=0, act=0, mis=None, pre=0, want=(True, True)):
    """kind "cin": adm_conv_small_cin_wgrad with Cin = Ch, Cout = Cother; "cout": adm_conv_small_cout_backward with Cout = Ch, Cin = Cother.
    mis: "x" / "dy" = that tensor is a view one float into its buffer (the scalar path by alignment); pre: dW is prefilled."""
    return dict(id=id, kind=kind, Ch=Ch, Cother=Cother, N=N, H=H, W=W, gn=gn, act=act, mis=mis, pre=pre, want=want)


def _small_branch(c):
    vec = c["W"] % 4 == 0 and c["mis"] is None
    b = f"{c['kind']}<{c['Ch']}>-{'quad' if vec else 'scalar'}{'-multi' if c['H'] * c['W'] > (1024 if vec else 256) else ''}"
    if c["kind"] == "cout":
        b += f"-groups{_cdiv(c['Cother'], 16)}{'r' if c['Cother'] % 16 else ''}-{'tail' if c['W'] % 4 else 'v4'}"
        b += f"-gn{c['gn']}act{c['act']}" + ("" if all(c["want"]) else ("-da-only" if c["want"][0] else "-dW-only"))
    return b + ("-prefilled" if c["pre"] else "")


SMALL_CASES = [sc_case(f"cin{k}-8x16", "cin", k, 5, 3, 8, 16, pre=k % 2) for k in (1, 2, 3, 4)] + [
    sc_case(f"cin{k}-7x{w}", "cin", k, 3, 2, 7, w, pre=(k + 1) % 2) for k, w in ((1, 6), (2, 9), (3, 6), (4, 9))
] + [
    sc_case(f"cin{k}-misaligned-{m}", "cin", k, 4, 2, 8, 16, mis=m) for k, m in ((1, "x"), (2, "dy"), (3, "x"), (4, "dy"))
] + [
    sc_case("cin1-24x48-multi-quad", "cin", 1, 2, 2, 24, 48), sc_case("cin4-24x48-multi-quad", "cin", 4, 2, 1, 24, 48, pre=1),
    sc_case("cin2-17x18-multi-scalar", "cin", 2, 2, 2, 17, 18),
] + [
    sc_case(f"cout{k}-8x16-cin{ci}", "cout", k, ci, 2, 8, 16, gn=k % 2, act=k % 2, pre=(k + 1) % 2) for k, ci in ((1, 32), (2, 8), (3, 40), (4, 16))
] + [
    sc_case(f"cout{k}-7x{w}-cin{ci}", "cout", k, ci, 2, 7, w, gn=(k + 1) % 2, act=k % 2, pre=k % 2) for k, w, ci in ((1, 6, 8), (2, 9, 40), (3, 6, 16), (4, 9, 8))
] + [
    sc_case(f"cout{k}-misaligned-{m}", "cout", k, 8, 2, 8, 16, gn=1, act=1, mis=m) for k, m in ((1, "dy"), (2, "x"), (3, "dy"), (4, "x"))
] + [
    sc_case("cout1-24x48-multi-quad", "cout", 1, 8, 2, 24, 48, gn=1, act=1), sc_case("cout4-24x48-multi-quad", "cout", 4, 40, 1, 24, 48, pre=1),
    sc_case("cout3-17x18-multi-scalar", "cout", 3, 8, 2, 17, 18, gn=1), sc_case("cout2-33x34-two-dgrad-blocks", "cout", 2, 8, 1, 33, 34, act=1),
    sc_case("cout2-da-only", "cout", 2, 40, 2, 8, 16, gn=1, act=1, want=(True, False)),
    sc_case("cout3-dW-only", "cout", 3, 8, 2, 7, 9, gn=1, act=1, pre=1, want=(False, True)),
    sc_case("cout1-da-only-tail", "cout", 1, 8, 2, 7, 6, want=(True, False)),
    sc_case("cout4-dW-only-quad", "cout", 4, 16, 2, 8, 16, act=1, want=(False, True)),
]


def _offset_view(t, dev, mis):
    """t on the device, as a view one float into a buffer when mis (16-byte misaligned), else 16-byte aligned."""
    buf = torch.zeros(t.numel() + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()] if mis else buf[:t.numel()]
    v.copy_(t.reshape(-1))
    return v.view(t.shape)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", SMALL_CASES, ids=[c["id"] for c in SMALL_CASES])
def test_small_conv_backward(backend, c):
    dev = select(backend)
    _, ops = _ops()
    N, H, W = c["N"], c["H"], c["W"]
    Cin, Cout = (c["Ch"], c["Cother"]) if c["kind"] == "cin" else (c["Cother"], c["Ch"])
    x, dy = _randn((N, Cin, H, W), 41), _randn((N, Cout, H, W), 42)
    w = _randn((Cout, Cin, 3, 3), 43, 0.2)
    gnp = None
    if c["gn"]:
        gnp = ((_randn((N, Cin), 44) * 0.3 + 1.0).contiguous(), _randn((N, Cin), 45).contiguous())

    def refs(dt):
        a = x.to(dt)
        if gnp is not None:
            a = a * gnp[0].to(dt)[:, :, None, None] + gnp[1].to(dt)[:, :, None, None]
        if c["act"]:
            a = F.silu(a)
        a = a.detach().requires_grad_(True)
        wt = w.to(dt).requires_grad_(True)
        F.conv2d(a, wt, padding=1).backward(dy.to(dt))
        return a.grad.detach(), wt.grad.detach()

    (da64, dw64), (da32, dw32) = refs(torch.float64), refs(torch.float32)
    pre = _randn(dw64.shape, 46, float(dw64.abs().max()) * 0.5) if c["pre"] else torch.zeros(dw64.shape)
    dWv, dWwhole = _guarded(pre, dev)
    xd, dyd = _offset_view(x, dev, c["mis"] == "x"), _offset_view(dy, dev, c["mis"] == "dy")
    tag = _tag(backend, c["id"], _small_branch(c))
    n_dw = N * H * W
    if c["kind"] == "cin":
        ops.conv_small_cin_wgrad(xd, dyd, out=dWv)
        assert _guard_intact(dWwhole, dw64.numel())
        _judge("adm_conv_small_cin_wgrad", "dW", dWv.cpu().view(dw64.shape), pre.double() + dw64, pre + dw32, n_dw, tag, ceiling=1e-4)
        return
    dav, dawhole = _guarded(torch.full(x.shape, CANARY), dev)
    gn = (gnp[0].to(dev), gnp[1].to(dev)) if gnp is not None else None
    ops.conv_small_cout_backward(xd, w.to(dev), dyd, gn=gn, act=bool(c["act"]), out=(dav, dWv), want=c["want"])
    assert _guard_intact(dawhole, x.numel()) and _guard_intact(dWwhole, dw64.numel())
    if c["want"][0]:
        _judge("adm_conv_small_cout_backward", "da", dav.cpu().view(x.shape), da64, da32, 9 * Cout, tag, ceiling=1e-4)
    else:
        assert bool((dawhole == CANARY).all()), "da = NULL: nothing may be written"
    if c["want"][1]:
        _judge("adm_conv_small_cout_backward", "dW", dWv.cpu().view(dw64.shape), pre.double() + dw64, pre + dw32, n_dw, tag, ceiling=1e-4)
    else:
        assert torch.equal(dWv.cpu().view(pre.shape), pre), "dW = NULL: nothing may be written"


# ================================================================ G. loud errors
ERROR_CASES = [
    ("ks5", dict(N=1, C1=32, H=8, W=8, Cout=32, ks=5), "ks must be 1 or 3"),
    ("stride2-ks1", dict(N=1, C1=32, H=8, W=8, Cout=32, ks=1, stride=2), "stride 2 only for 3x3"),
    ("wo12", dict(N=1, C1=32, H=4, W=12, Cout=32, ks=3), "powers of two"),
    ("ho3", dict(N=1, C1=32, H=3, W=16, Cout=32, ks=3), "powers of two"),
    ("ho3-1x1", dict(N=1, C1=128, H=3, W=16, Cout=128, ks=1), "powers of two"),
    ("wo6-stride2", dict(N=1, C1=32, H=8, W=12, Cout=32, ks=3, stride=2), "powers of two"),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name,shape,message", ERROR_CASES, ids=[e[0] for e in ERROR_CASES])
def test_wgrad_loud_errors(backend, name, shape, message):
    """Non-zero with a message, dW untouched, and the reported variant as it was."""
    dev = select(backend)
    N, ops = _ops()
    ks, stride = shape["ks"], shape.get("stride", 1)
    x = _randn((shape["N"], shape["C1"], shape["H"], shape["W"]), 51).to(dev)
    Ho, Wo = (shape["H"], shape["W"]) if stride == 1 else (shape["H"] // 2, shape["W"] // 2)
    dy = _randn((shape["N"], shape["Cout"], Ho, Wo), 52).to(dev)
    numel = shape["Cout"] * shape["C1"] * ks * ks
    view, whole = _guarded(torch.full((numel,), CANARY), dev)
    before = ops.last_wgrad_variant()
    with pytest.raises(N.NativeError, match=message):
        ops.conv2d_wgrad(x, dy, shape["Cout"], ks, stride=stride, pad_lo=1 if ks == 3 else 0, out=view)
    assert bool((whole == CANARY).all()), "dW written by a rejected call"
    assert ops.last_wgrad_variant() == before


def test_lds_rule_cannot_be_reached():
    """`conv_wgrad: patch too large for LDS` (64 * 129 + CB * PS floats <= 128 KiB): over every tile shape the launcher accepts (TW in 1..16, TH in
    1..4, powers of two) the largest patch is the 1x1 output's 64 images x 3x3 — no accepted shape is rejected by it."""
    worst = 0
    for ks, strides, CB in ((3, (1, 2), 32), (1, (1,), 128)):
        for stride in strides:
            for TW in (1, 2, 4, 8, 16):
                for TH in (1, 2, 4):
                    NI = 64 // (TW * TH)
                    PS = (NI * ((TH - 1) * stride + ks) * ((TW - 1) * stride + ks)) | 1
                    worst = max(worst, 4 * (64 * 129 + CB * PS))
    assert worst == 4 * (64 * 129 + 32 * 577) <= 128 * 1024


# ================================================================ the lists reach every branch
def test_case_lists_reach_every_branch():
    preds = [(c, _predict(c)) for c in WG_CASES]
    kernels = {p["kernel"] for _, p in preds}
    assert kernels == FP32_KERNELS, FP32_KERNELS - kernels
    assert {p["kernel"] for c, p in preds if c["path"] == 0} == FP32_KERNELS - {SP, GEN11}     # what the heuristic reaches by itself
    assert {_predict(c)["kernel"] for c in IMPULSE_CASES} == FP32_KERNELS
    assert {p["reduce"] for _, p in preds} == {1, 9}

    def depth(t):                                     # tiles per workgroup: 1, 2, 3, (4,) 5 and more
        return min(t, 5)
    for fam in ("sp8", "sp", "pf3", "pf1"):
        got = {depth(p["tpb"]) for _, p in preds if FAMILY[p["kernel"]] == fam}
        assert {1, 2, 3, 5} <= got, (fam, got)
        assert any(p["ragged_last"] and p["tpb"] > 1 for _, p in preds if FAMILY[p["kernel"]] == fam), (fam, "no short last workgroup")
        # consecutive tiles of one workgroup in different images, GroupNorm on
        assert any(c["gn"] and p["tpb"] > 1 and p["n_ptiles"] == _cdiv(c["N"], p["NI"]) > 1 for c, p in preds if FAMILY[p["kernel"]] == fam), fam
    for k in (PF3, PF3F, PF1, PF1F):                 # both members of the two prefetch families at every depth
        assert {1, 2, 3, 5} <= {depth(p["tpb"]) for _, p in preds if p["kernel"] == k}, k
    ids = {c["id"] for c in WG_CASES}
    assert len(ids) == len(WG_CASES)
    by = {c["id"]: (c, _predict(c)) for c in WG_CASES}
    # A: the refusals of the fast path, the generic kernel's shapes, stride 2 with both paddings, the 1x1 family's outputs
    for id, k in (("pf3-upfold", PF3), ("pf3-cout32", PF3), ("pf3-cout160", PF3), ("pf3-seam-c40+24", PF3), ("pf3-ct40-ragged-chunk", PF3),
                  ("pf3f-4x8-two-images", PF3F), ("gen31-by-option-4x16", GEN31), ("sp-4x16", SP), ("sp8-4x16", SP8)):
        assert by[id][1]["kernel"] == k, id
    assert {(p["Ho"], p["Wo"]) for c, p in preds if p["kernel"] == GEN31 and c["path"] == 0} >= {(4, 4), (2, 2), (1, 1), (2, 16), (8, 4)}
    assert {(p["Ho"], c["pad_lo"]) for c, p in preds if p["kernel"] == GEN32} >= {(h, pad) for h in (8, 2, 1) for pad in (0, 1)}
    for k in (PF1F, PF1, GEN11):
        assert {(p["Ho"], p["Wo"]) for c, p in preds if p["kernel"] == k} >= {(1, 1), (2, 2), (8, 8), (16, 32)}, k
    assert any(p["kernel"] == PF1 and c["gn"] for c, p in preds)
    # B: ragged tiles, two cout tiles, chunks inside x2
    assert any(p["Ho"] == 6 for _, p in preds) and any(p["Wo"] == 24 for _, p in preds)
    assert {p["NI"] for c, p in preds if c["N"] % 2 == 1 and c["N"] % p["NI"]} >= {2, 4, 16}
    assert any(c["N"] == 5 and p["NI"] == 16 for c, p in preds)
    assert any(c["Cout"] == 256 for c in WG_CASES) and any(c["C1"] == 64 and c["C2"] == 32 for c in WG_CASES)
    # C
    assert {FAMILY[p["kernel"]] for c, p in preds if c["bs"]} >= {"sp8", "sp", "pf3", "pf1", "gen"}
    assert {p["reduce"] for c, p in preds if c["acc"]} == {1, 9}
    assert {(c["dw_off"], p["reduce"]) for c, p in preds if c["dw_off"]} >= {(o, r) for o in (1, 2, 3) for r in (1, 9)}
    assert any(c["gn"] and not c["act"] for c in WG_CASES) and any(c["xscale"] > 1 and c["act"] for c in WG_CASES)
    # E
    rb = {_reduce_branch(c) for c in REDUCE_CASES}
    assert {c["split"] for c in REDUCE_CASES if c["taps"] == 1} >= set(SPLITS) and {c["split"] for c in REDUCE_CASES if c["taps"] == 9} >= set(SPLITS)
    for part in ("reduce-vec-chains4", "reduce-vec-chains1", "reduce-scalar", "-dvec-", "-dscalar-", "trips2", "reduce9-ragged", "reduce9-full",
                 "reduce9-full-trips1-waves4-acc0", "reduce9-full-trips1-waves4-acc1"):
        assert any(part in b for b in rb), part
    for kind in ("reduce-vec", "reduce-scalar", "reduce9"):
        for acc in ("acc0", "acc1"):
            assert any(b.startswith(kind) and b.endswith(acc) for b in rb), (kind, acc)
    assert any("dscalar" in b and b.endswith("acc1") for b in rb) and any("dscalar" in b and b.endswith("acc0") for b in rb)
    assert any(b.startswith("reduce9") and "trips2" in b for b in rb) and any(b.startswith("reduce-") and "trips2" in b for b in rb)
    assert any(c["taps"] == 1 and c["numel"] % 4 and True for c in REDUCE_CASES) and any(c["ws_off"] for c in REDUCE_CASES)
    # F
    sb = {_small_branch(c) for c in SMALL_CASES}
    for kind in ("cin", "cout"):
        for k in (1, 2, 3, 4):
            for walk in ("quad", "scalar"):
                assert any(b.startswith(f"{kind}<{k}>-{walk}") for b in sb), (kind, k, walk)
            assert any(c["kind"] == kind and c["Ch"] == k and c["mis"] for c in SMALL_CASES), (kind, k, "misaligned")
        assert any(b.startswith(kind) and "quad-multi" in b for b in sb) and any(b.startswith(kind) and "prefilled" in b for b in sb)
        assert {c["W"] for c in SMALL_CASES if c["kind"] == kind} >= {6, 9, 16}
    assert {c["Cother"] for c in SMALL_CASES if c["kind"] == "cout"} >= {8, 40}
    for part in ("-tail", "-v4", "gn1act1", "gn0act0", "-da-only", "-dW-only"):
        assert any(part in b for b in sb), part
