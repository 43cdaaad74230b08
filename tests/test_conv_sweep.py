"""Float64 sweep over the fp32 forward convolutions that are not Winograd: the implicit-GEMM family of k_conv_mfma.hip (the generic kernel, the
pipelined kernel, the two split-K launchers and their finish kernels) and the small-channel family of k_conv_small.hip (conv_in / conv_out
class), on both builds. The whole file runs with option "conv_wino" = 0 and "conv_bf16" at its default. Out of scope: the Winograd variants
4313-4317 (tests/test_conv_winograd.py, profiles/r05_accuracy.md), the 16-bit routes, the weight gradient (tests/test_wgrad_sweep.py).

Reference. The same fused operation in float64 torch on the CPU, from the SAME fp32 inputs: virtual concat, GroupNorm affine + SiLU on the load
path, nearest-x2 or zero-insertion upsample, padding, convolution, + bias + chan_add[n][co] + residual. The GroupNorm scale / shift handed to a
kernel are computed here in float64 and rounded to fp32 once; the reference applies those fp32 values in float64, so no statistics error enters.
The fp32 torch result of the same graph supplies e_torch_fp32.

Bars (the rule of tests/test_norm_sweep.py). g = max|d| / max|ref| over the tensor, h = the same ratio per (sample, cout) plane, maximised;
each <= M(n) * max(the same figure of fp32 torch, 4u), u = 2^-24, M(n) = max(8, sqrt(n / log2 n)), n = Ct * ks * ks, the length of the fmaf
chain (split K: still the whole K; the finish kernel adds the S slabs in order). The 1e-4 of the older tests stays as a ceiling on g. A plane
whose reference is exactly zero must be exactly zero. Figures are printed (`CONV_SWEEP ...`) before they are asserted; measured ratios:
profiles/conv_accuracy.md (tools/conv_accuracy.py).

Inputs. The weights of output channel co are scaled by a factor walking 1e-3 .. 1e3 over the output channels, bias / chan_add / residual the
same way: a loud channel cannot hide a quiet one from h. GroupNorm: per (sample, group) statistics mean/std 0, 0.25 and -30 (std 1, 0.1, 4), beta
in [1.5, 3], so the fp32 shift is at least 0.5 on EVERY channel and silu(shift) != 0: the zero padding, the zeros of up = 2 and the halo beyond a
ragged tile must stay exactly zero after the fused affine + SiLU — a kernel that activates padding is off by O(1) at the border. x1, x2 and
chan_add are slices of wider NaN-filled buffers (x1_bstride / x2_bstride / chan_add_stride), `out` sits between canaries.

Bit identity. For N > 1, out[N - 1] equals the same call on that sample alone (k_conv_mfma.hip: the partition depends on the layer only), and two
runs of one call are equal.

Dispatch. `_predict` restates launch_conv2d, dispatch_pf, launch_ksplit_generic and launch_conv_small; every case asserts it against
adm_last_conv_detail (variant, cout tile, split, finish kernel, tap mask, TW x TH x NI, register pipeline, cout parts of the grid).
`test_case_lists_reach_every_branch` asserts that the lists reach every branch named there. The environment switches (read once per process)
run in child processes: one fresh child per setting, one after the other, each under its own timeout; the parent judges what the child wrote.

Not reachable (shown by enumeration in test_pf_split_always_has_whole_float4): `total % 4 != 0` in dispatch_pf — every plane of at most 64
pixels that the pipelined 3x3 kernel tiles has a multiple of 4 pixels; S = 2 out of the `big` walk of launch_ksplit_generic (shown in
test_case_lists_reach_every_branch). A non-power-of-two plane does not keep a 1x1 convolution off the pipelined kernel (it runs there on 16 x 8
tiles), and zero insertion (up = 2) at 16 x 8 tiles runs on the pipelined 3x3 kernel; both are cases here, under the kernel that runs them.

The GroupNorm-fused finish (launch_ksplit_finish_gn) is reached through the test aid adm_conv2d_gn_finish, which announces the GroupNorm that
reads `out` the way the executors do: test_gn_fused_finish runs it with option "gn_fuse_finish" on and off, asserts `out` bit-identical to the
plain call and judges the scale / shift it leaves against float64 statistics of that output.
"""
import functools
import math
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                  # a child process of the environment-switch tests: no conftest has set the path up
    sys.path[:0] = [ROOT, os.path.join(ROOT, "audio-diffusion_amd"), os.path.join(ROOT, "tests")]

import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from native_backend import BACKENDS, select

U = 2.0 ** -24
CANARY = -12345.5
GUARD = 64                                  # floats of canary in front of and behind a guarded buffer (keeps its alignment)
GROUPS, EPS = 8, 1e-5
COMBOS = [(0.0, 1.0), (0.25, 1.0), (-30.0, 1.0), (0.0, 0.1), (-30.0, 4.0), (0.25, 0.1)]      # (mean / std, std) per (sample, group)
FIN_NONE, FIN_VEC4, FIN_SCALAR, FIN_GN = 0, 1, 2, 3
K_CIN, K_CIN_WIDE, K_COUT_WIDE, K_COUT = 1, 2, 3, 4
ENV0 = dict(pf=1, ksplit=1, kpf=1, in_wide=1, out_wide=1)
CK = 8


# ---------------------------------------------------------------- figures and bars
def _margin(n):
    return max(8.0, math.sqrt(n / math.log2(n))) if n > 2 else 8.0


def _ratios(t, ref64):
    """-> (g, h, zero planes ok): max|d| / max|ref| over the tensor and per (sample, cout) plane."""
    d = (t.double() - ref64).abs()
    g = float(d.max()) / (float(ref64.abs().max()) + 1e-300)
    if d.dim() < 3:
        return g, g, True
    dp, rp = d.flatten(2).amax(-1), ref64.abs().flatten(2).amax(-1)
    live = rp > 0
    h = float((dp[live] / rp[live]).max()) if bool(live.any()) else 0.0
    return g, h, bool((dp[~live] == 0).all())


def _judge(what, got, ref64, ref32, n, tag, ceiling=1e-4, planes=True):
    """got (kernel, fp32) against ref64 under M(n) * max(error of ref32, 4u), whole tensor (g) and per plane (h); printed, then asserted."""
    got = got.detach().cpu()
    assert got.shape == ref64.shape == ref32.shape, (what, tag, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), (what, tag, "kernel output is not finite")
    assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(ref64).all()), (what, tag, "reference is not finite")
    (gk, hk, zk), (gt, ht, _) = _ratios(got, ref64), _ratios(ref32, ref64)
    m = _margin(n)
    if not planes:
        hk, ht, zk = gk, gt, True
    for fig, ek, et in (("g", gk, gt), ("h", hk, ht))[:2 if planes else 1]:
        floor = max(et, 4 * U)
        print(f"CONV_SWEEP {tag} out={what} fig={fig} n={n} e_kernel={ek:.3e} e_torch_fp32={et:.3e} ratio={ek / floor:.2f} bound={m:.2f}")
    assert zk, (what, tag, "a plane whose reference is exactly zero must be exactly zero")
    assert gk <= m * max(gt, 4 * U), (what, tag, "g", gk, gt, m)
    assert hk <= m * max(ht, 4 * U), (what, tag, "h", hk, ht, m)
    if ceiling is not None:
        assert gk <= ceiling, (what, tag, gk, ceiling)


def _tag(backend, case, branch):
    return f"backend={backend} case={case} branch={branch}"


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _guarded(numel, dev):
    """-> (view, whole): a canary-filled device buffer with GUARD floats around the `numel` floats the kernel is given."""
    whole = torch.full((numel + 2 * GUARD,), CANARY, dtype=torch.float32).to(dev)
    view = whole[GUARD:GUARD + numel]
    assert (view.data_ptr() - whole.data_ptr()) == 4 * GUARD and whole.data_ptr() % 64 == 0
    return view, whole


def _guard_intact(whole, numel):
    w = whole.cpu()
    return bool((w[:GUARD] == CANARY).all()) and bool((w[GUARD + numel:] == CANARY).all())


def _ops():
    from audiodiffusion import _native, ops
    return _native, ops


class _Options:
    """Sets process-wide options for a block and puts the defaults back."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        N, _ = _ops()
        for k, v in self.kv.items():
            N.check(N.lib().adm_set_option(k.encode(), v))

    def __exit__(self, *exc):
        N, _ = _ops()
        for k in self.kv:
            N.check(N.lib().adm_set_option(k.encode(), -1))


def _sweep_options():
    return _Options(conv_wino=0)             # ("conv_bf16" stays at its default: fp32)


# ================================================================ the launchers' rules, restated
def _cdiv(a, b):
    return -(-a // b)


def _pow2(v):
    return v & (v - 1) == 0


def _out_dims(c):
    Hi, Wi = (2 * c["H"], 2 * c["W"]) if c["up"] else (c["H"], c["W"])
    if c["stride"] == 1:
        return Hi, Wi, Hi, Wi
    q = 2 if c["pad_lo"] else 1
    return Hi, Wi, (Hi + q - c["ks"]) // 2 + 1, (Wi + q - c["ks"]) // 2 + 1


def _is_small(c):
    Ct = c["C1"] + c["C2"]
    return Ct % CK != 0 or c["C1"] % CK != 0 or c["Cout"] % 4 != 0 or c["Cout"] < 32


def _predict(c, env=ENV0):
    """-> dict(variant, bm, S, finish, mask, TW, TH, NI, kpf, z, n): what launch_conv2d chooses for case c with "conv_wino" = 0."""
    if _is_small(c):
        return _predict_small(c, env)
    Ct, N, Cout, ks, stride = c["C1"] + c["C2"], c["N"], c["Cout"], c["ks"], c["stride"]
    _, _, Ho, Wo = _out_dims(c)
    Hi, Wi = _out_dims(c)[:2]
    pad = 0 if ks == 1 else c["pad_lo"]
    TW, TH = (16 if Wo >= 16 else Wo), (8 if Ho >= 8 else Ho)
    wide1x1 = ks == 1 and env["pf"] and _pow2(Wo) and _pow2(Ho) and Wo >= 4 and Wo * Ho >= 128
    if wide1x1:
        TW = 128 if Wo >= 128 else Wo
        TH = 128 // TW
    assert _pow2(TW) and _pow2(TH), "output dims below 16x8 must be powers of two"
    NI = 128 // (TW * TH)
    tiles_x, tiles_y, groups = _cdiv(Wo, TW), _cdiv(Ho, TH), _cdiv(N, NI)
    CS = (NI * ((TH - 1) * stride + ks) * ((TW - 1) * stride + ks) + 3) & ~3
    n_pt = tiles_x * tiles_y * groups
    bm = 32
    if Cout % 128 == 0 and n_pt * (Cout // 128) >= 256:
        bm = 128
    elif Cout % 64 == 0 and n_pt * (Cout // 64) >= 256:
        bm = 64
    p = dict(variant=ks * 100 + stride * 10 + bm // 32, bm=bm, S=1, finish=FIN_NONE, mask=0x1ff, TW=TW, TH=TH, NI=NI, kpf=0, z=1, n=Ct * ks * ks,
             Ho=Ho, Wo=Wo, n_pt=n_pt, groups=groups, tiles=(tiles_x, tiles_y), CS=CS, kernel="generic")
    total = N * Cout * Ho * Wo
    if env["pf"] and stride == 1 and ks == 3 and CS <= 256:
        p["variant"] += 2000
        p["kernel"] = "pf3"
        nch = Ct // CK
        if env["ksplit"] and Ho * Wo <= 64 and nch >= 16 and not c["wbs"] and total % 4 == 0:
            S = 8 if (nch <= 48 or Cout <= 256) else 4
            if c["single"]:
                S = 16
            while S > 1 and nch // S < 4:
                S -= 1
            if S > 1:
                p.update(variant=p["variant"] + 5, bm=64 if Cout % 64 == 0 else 32, S=S, finish=FIN_VEC4, kernel="pf3-split")
        return p
    split_1x1 = ks == 1 and Ho * Wo <= 16 and Ct // CK >= 8 and not c["wbs"]
    if (not split_1x1 and env["pf"] and ks == 1 and CS == 128 and Ct % 32 == 0 and c["C1"] % 32 == 0 and TW % 4 == 0 and Wo % 4 == 0
            and c["W"] % 4 == 0):
        p["variant"] += 2000
        p["kernel"] = "pf1"
        return p
    # launch_ksplit_generic
    nch, HWo = Ct // CK, Ho * Wo
    big = HWo > 64
    if not env["ksplit"] or c["wbs"] or nch < 8 or (big and not (c["single"] and ks == 3)):
        return p
    bmk = 128 if Cout % 128 == 0 else (64 if Cout % 64 == 0 else 32)
    S = 64 if HWo <= 4 else (32 if HWo <= 16 else (32 if c["single"] else 8))
    if big:
        wg1 = tiles_x * tiles_y * (Cout // bmk)
        if wg1 >= 128:
            return p
        S = 2
        while S < 16 and S * wg1 < 256:
            S *= 2
    S = min(S, nch // 2)
    if S < 2:
        return p
    mask = 0x1ff
    if ks == 3 and stride == 1:
        rows = [any(0 <= o + t - pad < Hi for o in range(Ho)) for t in range(3)]
        cols = [any(0 <= o + t - pad < Wi for o in range(Wo)) for t in range(3)]
        mask = sum(1 << (ty * 3 + tx) for ty in range(3) for tx in range(3) if rows[ty] and cols[tx])
    p.update(variant=ks * 100 + stride * 10 + bmk // 32 + 5, bm=bmk, S=S, mask=mask, kpf=int(bmk == 128 and stride == 1 and bool(env["kpf"])),
             finish=FIN_VEC4 if HWo % 4 == 0 else FIN_SCALAR, kernel="generic-split", big=big, ragged=nch % S != 0)
    return p


def _predict_small(c, env=ENV0):
    N, C1, H, W, Cout, ks = c["N"], c["C1"], c["H"], c["W"], c["Cout"], c["ks"]
    HW = H * W
    p = dict(variant=1001 if C1 <= 4 else 1002, S=1, finish=FIN_NONE, mask=0x1ff, NI=1, kpf=0, z=1, n=C1 * ks * ks, Ho=H, Wo=W)
    if C1 <= 4:
        if ks == 3 and W % 4 == 0 and env["in_wide"]:
            gx, z = (HW // 4 + 255) // 256, 1
            while gx * N * z < 256 and z < 16 and Cout // (2 * z) >= 8:
                z *= 2
            p.update(bm=K_CIN_WIDE, TW=1024, TH=1, z=z, kernel="cin-wide", stats_tiles=gx * 4)
        else:
            p.update(bm=K_CIN, TW=256, TH=1, kernel="cin")
        return p
    single_split = bool(c["single"]) and C1 >= 64
    if W % 64 == 0 and H % 16 == 0 and env["out_wide"] and not single_split:
        p.update(bm=K_COUT_WIDE, TW=64, TH=16, kernel="cout-wide")
        return p
    p.update(bm=K_COUT, TW=16, TH=16, kernel="cout")
    if env["ksplit"] and (HW <= 1024 or single_split) and C1 >= 64:
        p.update(S=8, finish=FIN_VEC4 if HW % 4 == 0 else FIN_SCALAR, kernel="cout-split")
    return p


def _detail_tuple(p):
    return (p["variant"], p["bm"], p["S"], p["finish"], p["mask"], p["TW"], p["TH"], p["NI"], p["kpf"], p["z"])


def _last_detail():
    N, _ = _ops()
    arr = (C.c_int * 12)(*([-1] * 12))
    v = N.lib().adm_last_conv_detail(arr, 12)
    assert v == arr[0] == N.lib().adm_last_conv_variant() and arr[10] == 0 and arr[11] == 0
    return tuple(arr[:10])


def _branch(c, env=ENV0):
    p = _predict(c, env)
    return f"{p['kernel']}-v{p['variant']}-bm{p['bm']}-S{p['S']}-f{p['finish']}-{p['TW']}x{p['TH']}x{p['NI']}" + ("-kpf" if p["kpf"] else "")


def cc(id, N, C1, C2, H, W, Cout, ks=3, stride=1, up=0, pad_lo=1, gn=1, act=1, chan=0, res=0, bs=(3, 5), wbs=0, single=0, stats=0):
    """One convolution case. chan: 0 none | 1 chan_add_stride == Cout | 2 a slice of a wider NaN-filled buffer (chan_add_stride > Cout);
    bs: extra channels of the wide NaN-filled x1 / x2 buffers (None: dense tensors, batch strides 0); wbs: per-sample weights; single: this
    call's single-sample rule; stats: the conv_in statistics epilogue."""
    if ks == 1:
        pad_lo = 0
    return dict(id=id, N=N, C1=C1, C2=C2, H=H, W=W, Cout=Cout, ks=ks, stride=stride, up=up, pad_lo=pad_lo, gn=gn, act=act, chan=chan, res=res,
                bs=bs, wbs=wbs, single=single, stats=stats)


# ---- A. pipelined 3x3 (conv_mfma_pf_kernel<3, ...>, CS <= 256), unsplit: the four tiles, ragged planes, N % NI != 0, the seam, bm, epilogues
PF3_CASES = [
    cc("pf3-16x8-chan+res", 2, 8, 0, 8, 16, 32, chan=2, res=1),
    cc("pf3-16x8-ragged-24x12-chan", 2, 8, 0, 12, 24, 32, chan=1),
    cc("pf3-16x8-ragged-40x20-res", 1, 8, 8, 20, 40, 32, res=1),
    cc("pf3-16x8-plain-dense", 2, 16, 0, 8, 16, 32, bs=None),
    cc("pf3-8x8-n3", 3, 8, 0, 8, 8, 32, chan=2, res=1),
    cc("pf3-8x4-n5", 5, 8, 0, 4, 8, 32, chan=2),
    cc("pf3-4x8-n5", 5, 8, 0, 8, 4, 32, res=1),
    cc("pf3-16x4-n3", 3, 8, 0, 4, 16, 32, chan=1, res=1),
    cc("pf3-16x4-ragged-24", 3, 8, 0, 4, 24, 32),
    cc("pf3-up1-4x8-to-8x16", 2, 16, 0, 4, 8, 32, up=1, gn=0, act=0, chan=2),
    cc("pf3-up1-gn-6x12-to-12x24", 2, 8, 0, 6, 12, 32, up=1, res=1),
    cc("pf3-seam-c8+24", 2, 8, 24, 8, 16, 64, chan=2, res=1),
    cc("pf3-gn-noact", 2, 8, 8, 8, 8, 32, act=0),
    cc("pf3-bm64", 16, 8, 0, 32, 64, 64, chan=2),
    cc("pf3-bm128", 16, 8, 0, 32, 64, 128, res=1),
    cc("pf3-bm64-ragged-n", 125, 8, 0, 4, 8, 512, chan=2, res=1),                # 32 image groups of 4, the last holds one image
]

# ---- B. pipelined split K (2316): planes of <= 64 pixels, >= 16 chunks
PF3_SPLIT_CASES = [
    cc("pfs-ct128-S4", 3, 128, 0, 8, 8, 64, chan=2, res=1),
    cc("pfs-ct144-S4-ragged", 2, 144, 0, 8, 8, 32, chan=1),
    cc("pfs-ct160-S5", 2, 64, 96, 4, 8, 64, res=1),
    cc("pfs-ct512-cout64-S8", 2, 256, 256, 8, 8, 64, chan=2),
    cc("pfs-ct512-cout512-S4", 1, 512, 0, 4, 16, 512, chan=2, res=1),
    cc("pfs-ct512-single-S16", 1, 512, 0, 8, 8, 96, single=1, chan=1, res=1),
    cc("pfs-ct136-S4-bm32-n5", 5, 136, 0, 8, 4, 96),
]

# ---- C. generic kernel, unsplit
GEN_CASES = [
    cc("gen-4x4-nch4", 9, 32, 0, 4, 4, 32, chan=2, res=1),
    cc("gen-16x2-nch7", 5, 24, 32, 2, 16, 64, chan=1),
    cc("gen-s2-pad1-16x32", 2, 16, 0, 16, 32, 32, stride=2, chan=2, res=1),
    cc("gen-s2-pad0-16x32", 2, 16, 0, 16, 32, 32, stride=2, pad_lo=0, chan=2, res=1),
    cc("gen-s2-pad1-ragged-24x40", 2, 8, 8, 24, 40, 32, stride=2, res=1),
    cc("gen-s2-pad0-ragged-24x40", 2, 8, 8, 24, 40, 32, stride=2, pad_lo=0, chan=1),
    cc("gen-s2-pad0-8x8-to-4x4", 9, 16, 0, 8, 8, 32, stride=2, pad_lo=0, chan=2),
    cc("gen-s2-pad1-odd-input-17x33", 1, 8, 0, 17, 33, 32, stride=2, res=1),
    cc("pf3-up2-8x16-to-16x32", 2, 32, 0, 8, 16, 32, up=2, gn=0, act=0),               # (at 16x8 tiles zero insertion runs on the pipelined kernel)
    cc("pf3-up2-gn-12x20-to-24x40", 1, 8, 0, 12, 20, 32, up=2, res=1),
    cc("gen-up2-2x2-to-4x4", 9, 32, 0, 2, 2, 32, up=2, gn=0, act=0, chan=2),
    cc("gen-up2-gn-1x8-to-2x16", 5, 16, 0, 1, 8, 32, up=2, res=1),
    cc("gen-1x1-c1-40", 2, 40, 24, 8, 16, 32, ks=1, chan=2, res=1),
    cc("gen-1x1-w6", 2, 32, 0, 16, 18, 32, ks=1, res=1),
    cc("gen-wbs-bm32", 3, 16, 0, 8, 16, 32, ks=1, gn=0, act=0, wbs=1),
    cc("gen-wbs-bm64", 4, 8, 0, 64, 128, 64, ks=1, gn=0, act=0, wbs=1),
    cc("pf3-wbs-3x3", 3, 8, 8, 12, 24, 32, wbs=1, chan=2, res=1),                      # (the pipelined kernel takes per-sample weights too)
    cc("gen-wbs-s2-single-unsplit", 2, 64, 0, 32, 32, 32, stride=2, single=1, wbs=1),  # the `big` split but for the per-sample weights
]

# ---- D. generic split K (x16 / x17 / x19): tap masks, S by plane, ragged parts, bm, two image groups, single_sample, the `big` branch, 1x1
GEN_SPLIT_CASES = [
    cc("gs-1x1-S64", 3, 512, 512, 1, 1, 32, chan=2, res=1),
    cc("gs-1x1-S32-clipped", 130, 512, 0, 1, 1, 64, chan=1),                      # N > 128 / plane: two image groups, the second holds 2
    cc("gs-2x2-S32", 5, 256, 256, 2, 2, 128, chan=2, res=1),
    cc("gs-1x4", 3, 64, 0, 1, 4, 32, res=1),
    cc("gs-4x1", 3, 64, 0, 4, 1, 32, chan=2),
    cc("gs-1x2-finish1", 3, 64, 8, 1, 2, 32, chan=2, res=1),
    cc("gs-2x1-finish1-no-terms", 3, 64, 0, 2, 1, 32),
    cc("gs-4x4-S8", 9, 128, 0, 4, 4, 64, chan=2, res=1),
    cc("gs-4x4-nch9-ragged", 2, 72, 0, 4, 4, 32, chan=1),
    cc("gs-4x4-bm128-kpf", 17, 64, 64, 4, 4, 128, res=1),
    cc("gs-up1-1x1-to-2x2", 3, 128, 0, 1, 1, 64, up=1, gn=0, act=0, chan=2),
    cc("gs-16x2-S8", 5, 128, 0, 2, 16, 64, chan=2, res=1),
    cc("gs-24x2-ragged-tile-in-x", 3, 64, 0, 2, 24, 32, chan=2, res=1),              # the split kernel's epilogue on a tile that ends inside the row
    cc("gs-8x8-single-S32", 1, 512, 0, 16, 16, 32, stride=2, single=1, chan=2, res=1),
    cc("gs-s2-4x4-to-2x2", 5, 128, 0, 4, 4, 128, stride=2, chan=2, res=1),
    cc("gs-s2-pad0-2x2-to-1x1", 3, 64, 64, 2, 2, 64, stride=2, pad_lo=0, chan=1, res=1),
    cc("gs-s2-16x16-to-8x8", 2, 64, 0, 16, 16, 32, stride=2, res=1),
    cc("gs-1x1conv-4x4-ct64", 9, 64, 0, 4, 4, 128, ks=1, chan=2, res=1),
    cc("gs-1x1conv-2x2-ct160", 16, 160, 0, 2, 2, 128, ks=1, res=1),
    cc("gs-1x1conv-1x1-finish1", 3, 64, 64, 1, 1, 32, ks=1, chan=2, res=1),
    cc("gs-1x1conv-4x4-ct56-not-split", 9, 56, 0, 4, 4, 32, ks=1, chan=2),
    cc("gs-1x1conv-plane32-ct64", 2, 64, 0, 4, 8, 32, ks=1, res=1),
    # the `big` branch: stride 2 under the single-sample rule, wg1 = tiles * Cout / bm workgroups per sample -> S = 16 (wg1 < 32), 8 (< 64),
    # 4 (< 128); wg1 >= 128: not taken. (S = 2 would need 2 * wg1 >= 256, which is not taken: test_case_lists_reach_every_branch)
    cc("gs-big-S16", 1, 256, 0, 32, 32, 32, stride=2, single=1, chan=2, res=1),           # 16x16 out: 2 tiles x 1 cout tile
    cc("gs-big-S8", 1, 128, 0, 64, 96, 96, stride=2, single=1, res=1),                    # 32x48 out: 12 tiles x 3 = 36
    cc("gs-big-S4", 1, 64, 0, 96, 128, 96, stride=2, single=1, pad_lo=0, chan=1),         # 48x64 out: 24 tiles x 3 = 72
    cc("gs-big-wg144-not-taken", 1, 64, 0, 128, 192, 96, stride=2, single=1),             # 64x96 out: 48 tiles x 3 = 144
    cc("gs-big-without-single-not-taken", 1, 256, 0, 32, 32, 32, stride=2),
]

# ---- E. pipelined 1x1 (dispatch_pf<1>)
PF1_CASES = [
    cc("pf1-row128", 1, 32, 0, 2, 128, 32, ks=1, chan=2, res=1),
    cc("pf1-row256-ragged-n", 2, 32, 0, 1, 256, 32, ks=1, res=1),
    cc("pf1-row64", 2, 32, 32, 2, 64, 32, ks=1, chan=1),
    cc("pf1-row16-plane128", 3, 32, 0, 8, 16, 64, ks=1, chan=2, res=1),
    cc("pf1-16x8-plane-below-128", 3, 32, 0, 4, 16, 32, ks=1, res=1),                  # 16 x 4 = 64 pixels: not wide, TW x TH = 16 x 4
    cc("pf1-8x8", 5, 64, 0, 8, 8, 32, ks=1, chan=2),
    cc("pf1-concat-seam", 2, 32, 96, 8, 16, 32, ks=1, chan=2, res=1),
    cc("pf1-plane-24x16-not-a-power-of-two", 2, 32, 32, 24, 16, 64, ks=1, chan=1),     # no wide rows, but 16 x 8 tiles: still the pipelined kernel
    cc("pf1-bm64", 4, 32, 0, 64, 128, 64, ks=1, chan=1),
    cc("pf1-bm128", 4, 32, 0, 64, 128, 128, ks=1, res=1),
]

MFMA_CASES = PF3_CASES + PF3_SPLIT_CASES + GEN_CASES + GEN_SPLIT_CASES + PF1_CASES

# ---- F. k_conv_small.hip
SMALL_CASES = [cc(f"cin{k}-ks{ks}-{name}", 2, k, 0, h, w, 12, ks=ks, gn=0, act=0, res=(k + ks) % 2, bs=None)
               for k in (1, 2, 3, 4) for ks in (1, 3) for (name, h, w) in (("wide", 8, 16), ("narrow", 7, 9))] + [
    cc("cin1-z-split-tiny-plane", 2, 1, 0, 8, 8, 32, gn=0, act=0, res=1, bs=None),
    cc("cin1-z-unsplit-large-plane", 1, 1, 0, 512, 512, 32, gn=0, act=0, bs=None),
    cc("cin2-stats", 2, 2, 0, 24, 32, 16, gn=0, act=0, res=1, bs=None, stats=1),
    cc("cin4-stats-z-split", 3, 4, 0, 16, 16, 64, gn=0, act=0, bs=None, stats=1),
] + [cc(f"cout{k}-wide", 2, 16, 0, 16, 64, k, gn=k % 2, act=k % 2, res=(k + 1) % 2, bs=None) for k in (1, 2, 3, 4)] + [
    cc(f"cout{k}-tiles-ragged-20x24", 2, 12, 0, 20, 24, k, gn=(k + 1) % 2, act=(k + 1) % 2, res=k % 2, bs=None) for k in (1, 2, 3, 4)
] + [
    cc("cout4-split-cin72-32x32", 2, 72, 0, 32, 32, 4, res=1, bs=None),
    cc("cout1-split-cin72-ragged-20x24", 2, 72, 0, 20, 24, 1, bs=None),
    cc("cout3-split-cin68-7x9-finish1", 2, 68, 0, 7, 9, 3, gn=0, act=0, res=1, bs=None),
    cc("cout2-cin72-plane-above-1024", 1, 72, 0, 33, 32, 2, bs=None),
    cc("cout2-cin56-below-64", 2, 56, 0, 16, 16, 2, res=1, bs=None),
    cc("cout2-single-64x16-split", 1, 72, 0, 16, 64, 2, single=1, res=1, bs=None),
    cc("cout2-single-cin16-stays-wide", 1, 16, 0, 16, 64, 2, single=1, bs=None),
    cc("cout1-wide-two-tiles", 1, 8, 0, 32, 128, 1, gn=0, act=0, bs=None),
]

ALL_CASES = MFMA_CASES + SMALL_CASES


# ================================================================ inputs and references
def _key(c):
    return tuple((k, (tuple(v) if isinstance(v, (list, tuple)) else v)) for k, v in sorted(c.items()) if k not in ("id", "bs", "single", "stats"))


@functools.lru_cache(maxsize=4)
def _reference(key):
    """Inputs (fp32) and both references of one case, computed once. -> dict(x, w, bias, chan, res, gn, ref64, ref32)."""
    c = dict(key)
    N, C1, C2, H, W, Cout, ks = c["N"], c["C1"], c["C2"], c["H"], c["W"], c["Cout"], c["ks"]
    Ct = C1 + C2
    _, _, Ho, Wo = _out_dims(c)
    x = _randn((N, Ct, H, W), 11)
    gnp = None
    if c["gn"]:
        G = GROUPS if Ct % GROUPS == 0 else 4
        xg = x.view(N, G, -1)
        for n in range(N):
            for g in range(G):
                r, s = COMBOS[(n * G + g) % len(COMBOS)]
                xg[n, g] = (xg[n, g] + r) * s
        gamma, beta = torch.rand((Ct,), generator=torch.Generator().manual_seed(13)).double() + 0.5, \
            torch.rand((Ct,), generator=torch.Generator().manual_seed(14)).double() * 1.5 + 1.5
        xd = x.double().view(N, G, -1)
        mean, var = xd.mean(-1, keepdim=True), xd.var(-1, unbiased=False, keepdim=True)
        rstd = (var + EPS).rsqrt().expand(N, G, Ct // G).reshape(N, Ct)
        mean = mean.expand(N, G, Ct // G).reshape(N, Ct)
        sc, sh = (gamma * rstd).float().contiguous(), (beta - mean * gamma * rstd).float().contiguous()
        assert float(sh.min()) >= 0.5 and float(F.silu(sh).min()) > 0.3, ("every channel's padding would show if it were activated", float(sh.min()))
        gnp = (sc, sh)
    cs = torch.logspace(-3, 3, Cout) if Cout > 1 else torch.ones(1)
    nw = N if c["wbs"] else 1
    w = _randn((nw, Cout, Ct, ks, ks), 12, (Ct * ks * ks) ** -0.5) * cs[None, :, None, None, None]
    bias = _randn((Cout,), 15) * cs
    chan = _randn((N, Cout), 16) * cs if c["chan"] else None
    res = _randn((N, Cout, Ho, Wo), 17) * cs[None, :, None, None] if c["res"] else None

    def graph(dt):
        a = x.to(dt)
        if gnp is not None:
            a = a * gnp[0].to(dt)[:, :, None, None] + gnp[1].to(dt)[:, :, None, None]
        if c["act"]:
            a = F.silu(a)
        if c["up"] == 1:
            a = F.interpolate(a, scale_factor=2.0, mode="nearest")
        elif c["up"] == 2:
            z = torch.zeros((N, Ct, 2 * H, 2 * W), dtype=dt)
            z[:, :, ::2, ::2] = a
            a = z
        if ks == 3:
            a = F.pad(a, (c["pad_lo"], 2, c["pad_lo"], 2))                  # zeros on every side the window can reach; cropped below
        ys = [F.conv2d(a[i:i + 1] if c["wbs"] else a, w[i].to(dt), stride=c["stride"])[:, :, :Ho, :Wo] for i in range(nw)]
        y = torch.cat(ys, 0) + bias.to(dt)[None, :, None, None]
        assert y.shape == (N, Cout, Ho, Wo), (y.shape, (N, Cout, Ho, Wo))
        if chan is not None:
            y = y + chan.to(dt)[:, :, None, None]
        if res is not None:
            y = y + res.to(dt)
        return y

    return dict(x=x, w=w, bias=bias, chan=chan, res=res, gn=gnp, ref64=graph(torch.float64), ref32=graph(torch.float32))


def _wide(t, extra, dev):
    """t (N, C, ...) as a channel slice of a NaN-filled buffer with `extra` more channels."""
    lead = extra // 2
    wide = torch.full((t.shape[0], t.shape[1] + extra) + tuple(t.shape[2:]), float("nan"))
    wide[:, lead:lead + t.shape[1]] = t
    wide = wide.to(dev)
    return wide[:, lead:lead + t.shape[1]], wide


def _launch(c, r, dev, rows=None, out=None, stats=None, gn_next=None, stats_tiles=None):
    """adm_conv2d for case c on inputs r (rows: only these samples, as their own batch). -> (out view, whole guarded buffer or None).
    gn_next = (gamma, beta, groups): through adm_conv2d_gn_finish -> (out, whole, taken, scale, shift)."""
    N, ops = _ops()
    sel = (lambda t: t) if rows is None else (lambda t: t[rows])
    x = sel(r["x"])
    Nn, C1, C2, Cout, ks = x.shape[0], c["C1"], c["C2"], c["Cout"], c["ks"]
    keep = []
    a = N.ConvArgs()
    if c["bs"] is None:
        x1, x2 = x[:, :C1].contiguous().to(dev), (x[:, C1:].contiguous().to(dev) if C2 else None)
    else:
        x1, w1 = _wide(x[:, :C1], c["bs"][0], dev)
        a.x1_bstride = x1.stride(0)
        x2 = None
        if C2:
            x2, w2 = _wide(x[:, C1:], c["bs"][1], dev)
            a.x2_bstride = x2.stride(0)
            keep.append(w2)
        keep.append(w1)
    a.x1, a.C1 = C.c_void_p(x1.data_ptr()), C1
    a.x2, a.C2 = (C.c_void_p(x2.data_ptr()), C2) if x2 is not None else (None, 0)
    a.N, a.H, a.W = Nn, c["H"], c["W"]
    a.up, a.stride, a.ks, a.pad_lo = c["up"], c["stride"], ks, c["pad_lo"]
    if r["gn"] is not None:
        sc, sh = sel(r["gn"][0]).contiguous().to(dev), sel(r["gn"][1]).contiguous().to(dev)
        a.gn_scale, a.gn_shift = N.ptr(sc), N.ptr(sh)
        keep += [sc, sh]
    a.act = c["act"]
    w = sel(r["w"]) if c["wbs"] else r["w"]
    wp = torch.stack([ops.pack_conv_weight(w[i].contiguous().to(dev)) for i in range(w.shape[0])]).contiguous()
    if c["wbs"]:
        a.w_bstride = wp.stride(0)
    bias = r["bias"].to(dev)
    a.wpacked, a.bias, a.Cout = N.ptr(wp), N.ptr(bias), Cout
    if c["chan"]:
        ch = sel(r["chan"])
        if c["chan"] == 2:
            chv, chw = _wide(ch, 7, dev)
            keep.append(chw)
        else:
            chv = ch.contiguous().to(dev)
        assert chv.stride(1) == 1
        a.chan_add, a.chan_add_stride = C.c_void_p(chv.data_ptr()), chv.stride(0)
        keep.append(chv)
    if c["res"]:
        rs = sel(r["res"]).contiguous().to(dev)
        a.residual = N.ptr(rs)
        keep.append(rs)
    a.single_sample = 1 if c["single"] else 0
    _, _, Ho, Wo = _out_dims(c)
    numel = Nn * Cout * Ho * Wo
    whole = None
    if out is None:
        out, whole = _guarded(numel, dev)
    a.out = C.c_void_p(out.data_ptr())
    if stats is not None:
        a.stats_out, a.stats_tiles = N.ptr(stats), (stats.shape[2] if stats_tiles is None else stats_tiles)
    if gn_next is not None:
        gamma, beta, groups = gn_next
        gd, bd = gamma.to(dev), beta.to(dev)
        scale, shift = torch.full((Nn, Cout), CANARY, device=dev), torch.full((Nn, Cout), CANARY, device=dev)
        taken = C.c_int(-1)
        N.check(N.lib().adm_conv2d_gn_finish(C.byref(a), N.ptr(gd), N.ptr(bd), groups, EPS, N.ptr(scale), N.ptr(shift), C.byref(taken),
                                             N.stream_for(x1)))
        return out.cpu().view(Nn, Cout, Ho, Wo), whole, taken.value, scale.cpu(), shift.cpu()
    N.check(N.lib().adm_conv2d(C.byref(a), N.stream_for(x1)))
    got = out.cpu().view(Nn, Cout, Ho, Wo)
    del keep
    return got, whole


def _check_case(backend, c, env=ENV0):
    """Runs case c in this process and judges it. -> the output (CPU)."""
    dev = select(backend)
    r = _reference(_key(c))
    p = _predict(c, env)
    tag = _tag(backend, c["id"], _branch(c, env))
    numel = r["ref64"].numel()
    stats = None
    if c["stats"]:
        stats = torch.full((c["N"], c["Cout"], p["stats_tiles"], 2), float("nan"), dtype=torch.float64, device=dev)
    t0 = time.perf_counter()
    got, whole = _launch(c, r, dev, stats=stats)
    dt = time.perf_counter() - t0
    assert _last_detail() == _detail_tuple(p), (c["id"], "dispatch", _last_detail(), _detail_tuple(p))
    assert _guard_intact(whole, numel), (c["id"], "a store outside out")
    print(f"CONV_SWEEP_TIME {tag} seconds={dt:.3f}")
    _judge("out", got, r["ref64"], r["ref32"], p["n"], tag)
    again, _ = _launch(c, r, dev)
    assert torch.equal(again, got), (c["id"], "two runs of one call differ")
    if c["N"] > 1:
        last = c["N"] - 1
        alone, _ = _launch(c, r, dev, rows=slice(last, last + 1))
        assert torch.equal(alone[0], got[last]), (c["id"], "a sample's bits depend on its batch", float((alone[0] - got[last]).abs().max()))
    if stats is not None:
        st = stats.cpu()
        assert bool(torch.isfinite(st).all())
        HW = c["H"] * c["W"]
        padded = torch.zeros((c["N"], c["Cout"], p["stats_tiles"] * 256))
        padded[:, :, :HW] = got.flatten(2)
        tiles = padded.view(c["N"], c["Cout"], p["stats_tiles"], 256)
        for k, pw in ((0, 1), (1, 2)):
            _judge(f"stats{k}", st[..., k].float(), tiles.double().pow(pw).sum(-1), tiles.pow(pw).sum(-1), 256, tag, ceiling=None)
    return got


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", ALL_CASES, ids=[c["id"] for c in ALL_CASES])
def test_conv(backend, c):
    select(backend)
    with _sweep_options():
        _check_case(backend, c)


# ================================================================ G. loud errors of launch_conv_small
def _refusal(id, message, **kw):
    base = dict(N=1, C1=2, C2=0, H=8, W=8, Cout=8, ks=3, gn=0, act=0, bs=None)
    base.update(kw)
    return (id, cc(id, **base), message)


REFUSALS = [
    _refusal("concat", "virtual concat not supported", C2=2),
    _refusal("stride2", "stride 1, no upsample only", stride=2),
    _refusal("up1", "stride 1, no upsample only", up=1),
    _refusal("chan-add", "chan_add not supported", chan=1),
    _refusal("cin-gn", "no fused norm/activation", gn=1, C1=4),
    _refusal("cin-act", "no fused norm/activation", act=1),
    _refusal("cout-ks1", "unsupported shape", C1=16, Cout=2, ks=1),
    _refusal("cout-pad0", "unsupported shape", C1=16, Cout=2, pad_lo=0),
    _refusal("neither-small", "unsupported shape", C1=12, Cout=8),
    _refusal("cin-narrow-stats", "no statistics epilogue", W=9, stats=1),           # (adm_conv_stats_tiles is 0 for it: stats_tiles = 0 passes conv2d's check)
    _refusal("cin-ks1-stats", "no statistics epilogue", ks=1, stats=1),
    _refusal("cin-slice", "batch strides", C1=2, bs=(3, 0)),
    _refusal("cout-slice", "batch strides", C1=16, Cout=2, bs=(3, 0)),
    _refusal("cout-per-sample-weights", "batch strides", C1=16, Cout=2, wbs=1),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("id,c,message", REFUSALS, ids=[e[0] for e in REFUSALS])
def test_small_loud_errors(backend, id, c, message):
    """Every ADM_REQUIRE of launch_conv_small: non-zero with its message, and nothing written."""
    dev = select(backend)
    N, _ = _ops()
    assert _is_small(c)
    r = _reference(_key(c))
    out, whole = _guarded(r["ref64"].numel(), dev)
    stats = torch.full((c["N"], c["Cout"], 4, 2), CANARY, dtype=torch.float64, device=dev) if c["stats"] else None
    with _sweep_options():
        with pytest.raises(N.NativeError, match=message):
            _launch(c, r, dev, out=out, stats=stats, stats_tiles=0)
    assert bool((whole == CANARY).all()), "out written by a rejected call"
    assert stats is None or bool((stats == CANARY).all()), "stats_out written by a rejected call"


def test_pf_split_always_has_whole_float4():
    """dispatch_pf's split asks for `total % 4 == 0` (its finish is ksplit_finish_kernel, four pixels per thread): over every output plane of at
    most 64 pixels that launch_conv2d tiles and hands to the pipelined 3x3 kernel (CS <= 256) the plane itself is a multiple of 4 pixels, so the
    rule can never send a layer to the unsplit kernel and no float4 of the finish straddles two channels."""
    planes = set()
    for Ho in range(1, 65):
        for Wo in range(1, 65):
            TW, TH = (16 if Wo >= 16 else Wo), (8 if Ho >= 8 else Ho)
            if Ho * Wo > 64 or not (_pow2(TW) and _pow2(TH)):
                continue
            NI = 128 // (TW * TH)
            if ((NI * (TH + 2) * (TW + 2) + 3) & ~3) <= 256:
                planes.add((Ho, Wo))
    assert planes == {(8, 8), (4, 8), (4, 16)} | {(h, 4) for h in range(8, 17)}, planes            # (Ho, Wo): every Wo is 4, 8 or 16
    assert all((h * w) % 4 == 0 for h, w in planes)


# ================================================================ H. the environment switches (read once per process)
CHILD_SETTINGS = {
    "pf0": (dict(ADM_CONV_PF="0"), dict(pf=0), [
        cc("pf0-gen3-16x8-bm32", 2, 8, 8, 12, 24, 32, chan=2, res=1),
        cc("pf0-gen3-16x8-bm64", 16, 8, 0, 32, 64, 64, chan=1),
        cc("pf0-gen3-16x8-bm128", 16, 8, 0, 32, 64, 128, res=1),
        cc("pf0-gen3-8x8-ct128-split", 3, 128, 0, 8, 8, 64, chan=2, res=1),
        cc("pf0-gen1-16x8", 3, 32, 0, 8, 16, 64, ks=1, chan=2, res=1),
    ]),
    "ksplit0": (dict(ADM_CONV_KSPLIT="0"), dict(ksplit=0), [
        cc("ksplit0-pf3-ct128", 3, 128, 0, 8, 8, 64, chan=2, res=1),
        cc("ksplit0-gen-4x4", 9, 128, 0, 4, 4, 64, chan=2, res=1),
        cc("ksplit0-gen-1x1", 3, 64, 0, 1, 1, 32, res=1),
        cc("ksplit0-cout-cin72", 2, 72, 0, 32, 32, 4, res=1, bs=None),
    ]),
    "ksp-pipe0": (dict(ADM_KSP_PIPE="0"), dict(kpf=0), [
        cc("kpf0-4x4-bm128", 17, 64, 64, 4, 4, 128, res=1),
        cc("kpf0-2x2-bm128", 5, 256, 256, 2, 2, 128, chan=2, res=1),
        cc("kpf0-1x1conv-4x4-bm128", 9, 64, 0, 4, 4, 128, ks=1, chan=2, res=1),
        cc("kpf0-1x4-bm128", 3, 64, 0, 1, 4, 128, res=1),
    ]),
    "in-wide0": (dict(ADM_CONV_IN_WIDE="0"), dict(in_wide=0), [
        cc(f"inwide0-cin{k}", 2, k, 0, 8, 16, 12, gn=0, act=0, res=k % 2, bs=None) for k in (1, 2, 3, 4)
    ]),
    "out-wide0": (dict(ADM_CONV_OUT_WIDE="0"), dict(out_wide=0), [
        cc(f"outwide0-cout{k}", 2, 16, 0, 16, 64, k, gn=k % 2, act=k % 2, res=(k + 1) % 2, bs=None) for k in (1, 2, 3, 4)
    ]),
}
BIT_IDENTICAL_TO_DEFAULT = {"ksp-pipe0"}     # k_conv_mfma.hip, KPF: "Same MFMA order: bit-identical"
CHILD_TIMEOUT = 300


def _child_main(backend, setting, path):
    dev = select(backend)
    _, env, cases = CHILD_SETTINGS[setting]
    env = dict(ENV0, **env)
    outs = {}
    with _sweep_options():
        for c in cases:
            r = _reference(_key(c))
            got, whole = _launch(c, r, dev)
            p = _predict(c, env)
            assert _last_detail() == _detail_tuple(p), (c["id"], "dispatch", _last_detail(), _detail_tuple(p))
            assert _guard_intact(whole, r["ref64"].numel()), (c["id"], "a store outside out")
            outs[c["id"]] = got
    torch.save(outs, path)


_ABNORMAL = {}                               # backend -> the setting whose child ended abnormally: nothing more is started on that backend


def _run_child(backend, setting):
    select(backend)                                                      # (builds the emulation library before the child needs it)
    assert backend not in _ABNORMAL, f"the child of setting {_ABNORMAL[backend]} ended abnormally: no further child is started"
    env = dict(os.environ, **CHILD_SETTINGS[setting][0])
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "out.pt")
        try:
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", backend, setting, path], env=env, capture_output=True,
                                 text=True, timeout=CHILD_TIMEOUT)
        except subprocess.TimeoutExpired:
            _ABNORMAL[backend] = setting
            raise
        if run.returncode not in (0, 1):                                 # (1: a Python exception, e.g. a failed assertion in the child)
            _ABNORMAL[backend] = setting
        assert run.returncode == 0, (setting, run.returncode, run.stdout[-3000:], run.stderr[-3000:])
        return torch.load(path)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("setting", list(CHILD_SETTINGS))
def test_environment_switches(backend, setting):
    """One fresh child per setting, one after the other (pytest runs them in order); after a child that ended abnormally — a signal, a time
    limit — no further child is started on that backend: the remaining settings fail at once."""
    _, envp, cases = CHILD_SETTINGS[setting]
    assert len(cases) <= 6
    outs = _run_child(backend, setting)
    env = dict(ENV0, **envp)
    for c in cases:
        r = _reference(_key(c))
        _judge("out", outs[c["id"]], r["ref64"], r["ref32"], _predict(c, env)["n"], _tag(backend, c["id"], f"{setting}:" + _branch(c, env)))
        if setting in BIT_IDENTICAL_TO_DEFAULT:
            with _sweep_options():
                here, _ = _launch(c, r, select(backend))
                assert _last_detail() == _detail_tuple(_predict(c)) and _predict(c)["kpf"] == 1
            assert torch.equal(here, outs[c["id"]]), (c["id"], "the register-pipelined split kernel is not bit-identical to the plain one")


# ================================================================ I. the GroupNorm-fused finish (launch_ksplit_finish_gn)
GN_FINISH_CASES = [c for c in PF3_SPLIT_CASES + GEN_SPLIT_CASES if c["id"] in (
    "pfs-ct128-S4", "pfs-ct144-S4-ragged", "pfs-ct512-single-S16", "gs-1x1-S64", "gs-2x2-S32", "gs-1x2-finish1", "gs-4x4-S8", "gs-4x4-bm128-kpf",
    "gs-s2-16x16-to-8x8", "gs-1x1conv-4x4-ct64", "gs-1x1conv-1x1-finish1", "gs-big-S16")] + [PF3_CASES[0]]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("c", GN_FINISH_CASES, ids=[c["id"] for c in GN_FINISH_CASES])
def test_gn_fused_finish(backend, c):
    """A convolution announced as the executors announce it when a GroupNorm reads its output (adm_conv2d_gn_finish): a split launch on a plane of
    at most 8x8 pixels leaves that GroupNorm's scale / shift from its finish pass; option "gn_fuse_finish" = 0, a `big` split or an unsplit
    launch do not. `out` is bit-identical in all of them, and scale / shift are judged against float64 statistics of that very output."""
    dev = select(backend)
    N, _ = _ops()
    r = _reference(_key(c))
    p = _predict(c)
    Cout, groups = c["Cout"], 4
    gamma = torch.rand((Cout,), generator=torch.Generator().manual_seed(61)) + 0.5
    beta = _randn((Cout,), 62)
    fusable = p["S"] > 1 and not p.get("big")
    with _sweep_options():
        plain, _ = _launch(c, r, dev)
        for on in (1, 0):
            with _Options(gn_fuse_finish=on):
                got, whole, taken, scale, shift = _launch(c, r, dev, gn_next=(gamma, beta, groups))
                det = _last_detail()
            assert _guard_intact(whole, plain.numel())
            assert torch.equal(got, plain), (c["id"], on, "the tensor must not depend on who computes the statistics")
            assert taken == int(bool(on and fusable)), (c["id"], on, taken)
            want = dict(p, finish=FIN_GN) if taken else p
            assert det == _detail_tuple(want), (c["id"], on, det, _detail_tuple(want))
            if not taken:
                assert bool((scale == CANARY).all()) and bool((shift == CANARY).all())
                continue
            tag = _tag(backend, c["id"], _branch(c) + "-gnfinish")

            def stats(dt):
                y = got.to(dt).view(c["N"], groups, -1)
                mean, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
                rstd = (var + EPS).rsqrt().expand(-1, -1, Cout // groups).reshape(c["N"], Cout)
                mean = mean.expand(-1, -1, Cout // groups).reshape(c["N"], Cout)
                sc = gamma.to(dt) * rstd
                return sc, beta.to(dt) - mean * sc
            (sc64, sh64), (sc32, sh32) = stats(torch.float64), stats(torch.float32)
            n = (Cout // groups) * p["Ho"] * p["Wo"]
            _judge("gn_scale", scale, sc64, sc32, n, tag, ceiling=None, planes=False)
            _judge("gn_shift", shift, sh64, sh32, n, tag, ceiling=None, planes=False)


# ================================================================ the lists reach every branch
def test_case_lists_reach_every_branch():
    ids = [c["id"] for c in ALL_CASES]
    assert len(set(ids)) == len(ids)
    P = [(c, _predict(c)) for c in ALL_CASES]
    by = {c["id"]: (c, p) for c, p in P}

    def some(pred, what):
        assert any(pred(c, p) for c, p in P), what

    # pipelined 3x3, unsplit
    pf3 = [(c, p) for c, p in P if p.get("kernel") == "pf3"]
    assert {(p["TW"], p["TH"], p["NI"]) for _, p in pf3} >= {(16, 8, 1), (8, 8, 2), (8, 4, 4), (4, 8, 4), (16, 4, 2)}
    assert {p["Wo"] for _, p in pf3} >= {24, 40} and {p["Ho"] for _, p in pf3} >= {12, 20}
    assert any(c["up"] == 1 for c, _ in pf3) and {p["NI"] for c, p in pf3 if c["N"] % p["NI"]} >= {2, 4}
    assert any(c["C1"] == 8 and c["C2"] == 24 for c, _ in pf3)
    assert {p["bm"] for _, p in pf3} == {32, 64, 128} and {p["variant"] for _, p in pf3} == {2311, 2312, 2314}
    assert {(bool(c["chan"]), bool(c["res"])) for c, _ in pf3} == {(a, b) for a in (False, True) for b in (False, True)}
    # pipelined split K
    pfs = [(c, p) for c, p in P if p.get("kernel") == "pf3-split"]
    assert all(p["variant"] in (2316, 2317) and p["Ho"] * p["Wo"] <= 64 for _, p in pfs)
    assert {(c["C1"] + c["C2"], p["S"]) for c, p in pfs} >= {(128, 4), (144, 4), (160, 5), (512, 8), (512, 4), (512, 16)}
    assert {p["bm"] for _, p in pfs} == {32, 64} and any(c["single"] and p["S"] == 16 for c, p in pfs)
    assert by["pfs-ct512-cout64-S8"][1]["S"] == 8 and by["pfs-ct512-cout512-S4"][1]["S"] == 4
    # generic, unsplit
    gen = [(c, p) for c, p in P if p.get("kernel") == "generic"]
    assert {(p["Ho"], p["Wo"]) for c, p in gen if c["ks"] == 3 and c["stride"] == 1 and not c["up"]} >= {(4, 4), (2, 16)}
    assert {(c["pad_lo"], p["Wo"] % 16 == 0 and p["Ho"] % 8 == 0) for c, p in gen if c["stride"] == 2} == {(a, b) for a in (0, 1) for b in (False, True)}
    assert any(c["up"] == 2 for c, _ in gen) and any(c["up"] == 2 for c, _ in pf3)
    one = [(c, p) for c, p in gen if c["ks"] == 1 and not c["wbs"]]
    assert any(c["C1"] % 32 for c, _ in one) and any(c["W"] % 4 for c, _ in one)
    assert {p["bm"] for c, p in gen if c["wbs"]} >= {32, 64} and all(p["NI"] == 1 and p["S"] == 1 for c, p in P if c["wbs"])
    some(lambda c, p: c["wbs"] and (c["C1"] + c["C2"]) // CK >= 8, "per-sample weights keep a long K loop unsplit")
    # generic split K
    gs = [(c, p) for c, p in P if p.get("kernel") == "generic-split"]
    assert {p["variant"] for _, p in gs} >= {316, 317, 319, 326, 327, 329, 116, 119}
    assert {(p["Ho"], p["Wo"]) for c, p in gs if c["ks"] == 3 and c["stride"] == 1} >= {(1, 1), (2, 2), (1, 4), (4, 1), (4, 4), (1, 2), (2, 16)}
    assert {p["mask"] for _, p in gs} >= {0x010, 0x038, 0x092, 0x1ff}                        # 1x1: the centre | 1x4: the middle row | 4x1: the middle column
    assert {p["S"] for _, p in gs} >= {64, 32, 8, 4, 16} and any(p["ragged"] for _, p in gs)
    assert by["gs-4x4-nch9-ragged"][1]["S"] == 4 and by["gs-1x1-S32-clipped"][1]["groups"] == 2
    some(lambda c, p: p.get("kernel") == "generic-split" and p["Wo"] % p["TW"] != 0, "a split launch whose last tile of a row is ragged")
    assert {(p["bm"], p["kpf"]) for _, p in gs} >= {(32, 0), (64, 0), (128, 1), (128, 0)}     # (128, 0): stride 2
    assert {p["finish"] for _, p in gs} == {FIN_VEC4, FIN_SCALAR}
    for fin in (FIN_VEC4, FIN_SCALAR):
        assert {(bool(c["chan"]), bool(c["res"])) for c, p in P if p["finish"] == fin} >= {(True, True), (True, False), (False, True)}, fin
        assert any(c["chan"] == 2 for c, p in P if p["finish"] == fin), fin
    for fin in (FIN_VEC4, FIN_SCALAR):
        some(lambda c, p: p["finish"] == fin and not c["chan"] and not c["res"], ("finish with neither term", fin))
    some(lambda c, p: c["up"] == 1 and p.get("kernel") == "generic-split" and p["Ho"] == 2, "up = 1 from 1x1")
    some(lambda c, p: c["single"] and p.get("kernel") == "generic-split" and p["Ho"] * p["Wo"] == 64 and p["S"] == 32, "single 8x8")
    big = {c["id"]: p for c, p in P if c["id"].startswith("gs-big")}
    assert {p["S"] for p in big.values() if p.get("big")} == {4, 8, 16}
    assert big["gs-big-wg144-not-taken"]["S"] == 1 and big["gs-big-without-single-not-taken"]["S"] == 1
    # S = 2 cannot come out of the `big` walk (it stops at 2 only if 2 * wg1 >= 256, and wg1 >= 128 is not taken), nor out of the clip (nch >= 8)
    for wg1 in range(1, 128):
        S = 2
        while S < 16 and S * wg1 < 256:
            S *= 2
        assert S >= 4
    assert by["gs-1x1conv-4x4-ct64"][1]["S"] > 1 and by["gs-1x1conv-4x4-ct56-not-split"][1]["S"] == 1
    assert by["gs-1x1conv-plane32-ct64"][1]["kernel"] == "pf1"
    # pipelined 1x1
    pf1 = [(c, p) for c, p in P if p.get("kernel") == "pf1"]
    assert {(p["TW"], p["TH"]) for _, p in pf1} >= {(128, 1), (64, 2), (16, 8), (16, 4), (8, 8)}
    assert {p["bm"] for _, p in pf1} == {32, 64, 128} and any(c["C2"] for c, _ in pf1) and any(not _pow2(p["Ho"]) for _, p in pf1)
    # small-channel family
    sm = [(c, p) for c, p in P if _is_small(c)]
    assert {(c["C1"], c["ks"], p["kernel"]) for c, p in sm if c["C1"] <= 4} >= {(k, ks, kern) for k in (1, 2, 3, 4)
                                                                                for (ks, kern) in ((3, "cin-wide"), (3, "cin"), (1, "cin"))}
    assert {p["z"] for c, p in sm if p["kernel"] == "cin-wide" and c["Cout"] == 32} >= {1, 4}
    assert any(c["stats"] for c, _ in sm) and any(c["res"] for c, p in sm if p["kernel"].startswith("cin"))
    for kern in ("cout-wide", "cout"):
        assert {c["Cout"] for c, p in sm if p["kernel"] == kern} == {1, 2, 3, 4}, kern
        assert {c["gn"] for c, p in sm if p["kernel"] == kern} == {0, 1}, kern
    assert any(c["H"] == 20 and c["W"] == 24 for c, p in sm if p["kernel"] == "cout")
    assert {(c["C1"], p["kernel"]) for c, p in sm} >= {(72, "cout-split"), (72, "cout"), (56, "cout"), (68, "cout-split")}
    assert {p["finish"] for c, p in sm if p["kernel"] == "cout-split"} == {FIN_VEC4, FIN_SCALAR}
    some(lambda c, p: c["single"] and p.get("kernel") == "cout-split" and (c["H"], c["W"]) == (16, 64), "single_sample on a 64x16 plane")
    # the environment switches
    pf0 = [_predict(c, dict(ENV0, pf=0)) for c in CHILD_SETTINGS["pf0"][2]]
    assert {(p["variant"], p["TW"], p["TH"]) for p in pf0} >= {(311, 16, 8), (312, 16, 8), (314, 16, 8), (111, 16, 8)}
    assert all(_predict(c, dict(ENV0, ksplit=0))["S"] == 1 and _predict(c)["S"] > 1 for c in CHILD_SETTINGS["ksplit0"][2])
    assert all(_predict(c)["kpf"] == 1 and _predict(c, dict(ENV0, kpf=0))["kpf"] == 0 for c in CHILD_SETTINGS["ksp-pipe0"][2])
    assert all(_predict(c)["kernel"] == "cin-wide" and _predict(c, dict(ENV0, in_wide=0))["kernel"] == "cin" for c in CHILD_SETTINGS["in-wide0"][2])
    assert all(_predict(c)["kernel"] == "cout-wide" and _predict(c, dict(ENV0, out_wide=0))["kernel"] == "cout" for c in CHILD_SETTINGS["out-wide0"][2])


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    _child_main(sys.argv[2], sys.argv[3], sys.argv[4])
