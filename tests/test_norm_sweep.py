"""Float64 sweep over the norm, reduction and time-embedding kernels: every branch of every launcher, on both builds.

Four families, each entry against the same operation in float64 torch on the CPU:
  A. GroupNorm: `adm_groupnorm_stats`, `adm_groupnorm_stats_ex`, `adm_groupnorm_finalize`, `adm_groupnorm_backward`
  B. LayerNorm and GEGLU: `adm_layernorm_nct`, `adm_layernorm_nct_backward`, `adm_geglu`, `adm_geglu_backward`
  C. reductions and small dense layers of the backward pass: `adm_chan_sums`, `adm_linear_backward`, `adm_sumpool2x2`, `adm_accumulate`
  D. time embedding: `adm_time_embedding`, `adm_temb_proj` (test aids: the executors launch these kernels at their model's shapes only)

Every case names the branch or instantiation it is meant to reach, recomputed here from the launcher's (or the kernel's) own rule, and
`test_case_lists_reach_every_branch` asserts that the lists below reach each of them, so an edit of a list cannot silently drop one.

Bars (the rule of tests/test_attention_sweep.py). For every compared tensor g = max|d| / max|ref| against float64, and
g_kernel <= M(n) * max(g_torch_fp32, 4u), u = 2^-24, M(n) = max(8, sqrt(n / log2 n)), n = the number of terms of that output's longest
reduction: cg * HW for GroupNorm y, mean, rstd and dx, N * HW for dgamma / dbeta; C for LayerNorm y, dx and its statistics, N * T for its
dgamma / dbeta; HW / N * HW for the per-(n, c) / per-c channel sums; B for dW and db, J for dX of the linear layers; K for the time embedding;
4 for the elementwise kernels (GEGLU, accumulate, sumpool2x2). Where a shape and input of the older tests is re-run, the ceiling that test
asserts stays as a ceiling (2e-5 / 2e-4 GroupNorm forward, 1e-4 its backward, 2e-6 LayerNorm forward and GEGLU, 1e-5 LayerNorm and linear
backward, 1e-4 the rest). Figures are printed (`NORM_SWEEP ...`) before they are asserted; measured ratios: profiles/norm_accuracy.md.

Slices. Where a destination is a slice of a wider buffer (`dst_bs > per_sample`, `nc_stride > C`, the rows behind `out` of temb_proj, every
gradient buffer) the surroundings hold a canary that must come back untouched; where a SOURCE is a slice (`ldy > J`) the surroundings hold NaN,
so one read outside the slice makes the output non-finite.

dgamma / dbeta of GroupNorm and `out_c` of chan_sums are fp32 atomics over n on the device: no bit identity between two runs is asserted for
them. It is asserted for everything that is deterministic by construction: scale, shift, mean_rstd, dx, `out_nc`, LayerNorm, emb and temb.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from native_backend import BACKENDS, select

U = 2.0 ** -24
CANARY = -12345.5
GUARD = 64                                  # floats of canary on either side of a guarded buffer (keeps 256-byte alignment)


# ---------------------------------------------------------------- figures and bars
def _margin(n):
    return max(8.0, math.sqrt(n / math.log2(n))) if n > 2 else 8.0


def _g(a, ref):
    return float((a.double() - ref).abs().max() / (ref.abs().max() + 1e-300))


def _judge(entry, what, got, ref64, ref32, n, tag, ceiling=None, scale=None):
    """got (kernel, fp32) against ref64 under M(n) * max(error of ref32, 4u); the figures are printed before they are asserted.
    scale: what max|d| is divided by where the reference is exactly zero (in place of max|ref|)."""
    got = got.detach().cpu()
    ref64, ref32 = ref64.detach(), ref32.detach()
    assert got.shape == ref64.shape == ref32.shape, (entry, what, tag, got.shape, ref64.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), (entry, what, tag, "kernel output is not finite")
    assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(ref64).all()), (entry, what, tag, "reference is not finite")
    e_kernel, e_torch = _g(got, ref64), _g(ref32, ref64)
    if scale is not None:
        e_kernel, e_torch = float((got.double() - ref64).abs().max()) / scale, float((ref32.double() - ref64).abs().max()) / scale
    floor = max(e_torch, 4 * U)
    bound = _margin(n) * floor
    print(f"NORM_SWEEP {tag} entry={entry} out={what} n={n} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} "
          f"ratio={e_kernel / floor:.2f} bound={_margin(n):.2f}")
    assert e_kernel <= bound, (entry, what, tag, e_kernel, e_torch, bound)
    if ceiling is not None:
        assert e_kernel <= ceiling, (entry, what, tag, e_kernel, ceiling)


def _tag(backend, case, branch):
    return f"backend={backend} case={case} branch={branch}"


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


def _guarded(init, dev):
    """-> (view, whole): `init` copied into the middle of a canary-filled device buffer; the view is what the kernel is given."""
    whole = torch.full((init.numel() + 2 * GUARD,), CANARY, dtype=torch.float32)
    whole[GUARD:GUARD + init.numel()] = init.reshape(-1)
    whole = whole.to(dev)
    return whole[GUARD:GUARD + init.numel()].view(init.shape), whole


def _guard_intact(whole):
    w = whole.cpu()
    return bool((w[:GUARD] == CANARY).all()) and bool((w[-GUARD:] == CANARY).all())


def _native():
    from audiodiffusion import _native
    return _native, _native.lib()


# ================================================================ A. GroupNorm
RATIOS, STDS = [0.0, 0.25, 30.0, 1000.0], [1e-3, 1.0, 30.0]
COMBOS = [(r, s) for r in RATIOS for s in STDS]
CONST = 0.7                                 # the all-constant group of a "mixed" case: var = 0, rstd = eps^-1/2


def _gn_input(N, C, groups, HW, stats, seed):
    """(N, C, HW) with per-(sample, group) statistics: "mixed" walks the twelve (mean/std, std) pairs over the (sample, group) index and makes
    group 1 of sample 0 constant; a pair (mean/std, std) gives every group those; "old" is the input of the older tests (3 * randn + 1.5)."""
    x = _randn((N, groups, (C // groups) * HW), seed)
    if stats == "old":
        return (x * 3 + 1.5).reshape(N, C, HW).contiguous()
    for n in range(N):
        for g in range(groups):
            r, s = COMBOS[(n * groups + g) % len(COMBOS)] if stats == "mixed" else stats
            x[n, g] = (x[n, g] + r) * s
    if stats == "mixed":
        x[0, 1 % groups] = CONST
    return x.reshape(N, C, HW).contiguous()


def _gn_fwd_branch(HW):
    """gn_stats_kernel's three walks, and inside the channel-major one whether the four-deep loop and the remainder loop run."""
    if HW % 4:
        return "scalar"
    q = HW // 4
    if q >= 256:
        deep, rem = q > 768, q % 1024 != 0
        return "planes256" + ("_deep" if deep else "") + ("_rem" if rem else "")
    return "planes_sub" if 256 % q == 0 else "float4_flat"


def _gn_streaming(N, C, HW):
    return N * C * HW * 4 >= (64 << 20)


def _gn_bwd_branch(N, C, HW, acc1, acc2, C2):
    """gn_bwd_stats / gn_bwd_apply: streaming instantiation, float4 or scalar walk, the in-flight iterations a thread really uses (stats: of
    256 * 4 float4 per pass; apply: of gx * 256 * 4), the apply grid gx, more than one pass of the stats loop, the accumulate flags."""
    nt = "nt" if _gn_streaming(N, C, HW) else "ld"
    gx = max(1, (HW + 4095) // 4096)
    if HW % 4:
        return f"{nt}-scalar-gx{gx}-acc{acc1}{acc2 if C2 else 'x'}"
    n4 = HW // 4
    us = min(4, -(-n4 // 256))
    ua = min(4, -(-n4 // (gx * 256)))
    return f"{nt}-v4-su{us}{'+' if n4 > 1024 else ''}-au{ua}-gx{gx}-acc{acc1}{acc2 if C2 else 'x'}"


# (id, N, C1, C2, groups, HW, stats, act, acc1, acc2)
GN_CASES = [
    ("hw1-cg1", 2, 32, 0, 32, 1, "mixed", 1, 0, 0),
    ("hw1-cg2", 3, 64, 0, 32, 1, "mixed", 0, 1, 0),
    ("hw7", 2, 64, 0, 32, 7, "mixed", 1, 1, 0),
    ("hw49-g4", 3, 16, 0, 4, 49, "mixed", 0, 0, 0),
    ("hw16-seam-in", 2, 64, 32, 32, 16, "mixed", 1, 0, 1),
    ("hw64-g8", 1, 32, 0, 8, 64, "mixed", 1, 0, 0),
    ("hw24", 2, 64, 0, 32, 24, "mixed", 0, 0, 0),
    ("hw384-g4", 2, 16, 0, 4, 384, "mixed", 1, 1, 0),
    ("hw1024-cg1", 1, 32, 0, 32, 1024, "mixed", 1, 0, 0),
    ("hw1024-seam-on", 2, 16, 16, 4, 1024, "mixed", 0, 1, 1),
    ("hw1028-seam-on", 2, 32, 32, 8, 1028, "mixed", 1, 1, 0),
    ("hw4096-g8", 1, 32, 0, 8, 4096, "mixed", 1, 1, 0),
    ("hw4096-N3", 3, 8, 8, 4, 4096, "mixed", 0, 0, 1),
    ("hw4100-N3", 3, 8, 0, 4, 4100, "mixed", 1, 0, 0),
    ("hw4100-seam-in", 1, 6, 10, 4, 4100, "mixed", 0, 1, 1),
    ("hw4160-seam-in", 2, 20, 44, 8, 4160, "mixed", 1, 0, 0),
    ("hw4608-seam-on", 1, 32, 32, 8, 4608, "mixed", 0, 0, 1),
    ("hw8192", 1, 32, 0, 32, 8192, "mixed", 1, 0, 0),
    ("hw8192-acc", 2, 8, 8, 4, 8192, "mixed", 1, 1, 1),
    ("hw12288-gx3", 1, 16, 0, 4, 12288, "mixed", 1, 1, 0),
    ("hw65536-gx16", 1, 32, 0, 32, 65536, "mixed", 1, 0, 0),
    ("hw65536-gx16-acc", 1, 4, 4, 4, 65536, "mixed", 0, 1, 1),
    ("hw4098-scalar-gx2", 2, 8, 0, 4, 4098, "mixed", 1, 1, 0),
    ("stream-64MiB", 2, 64, 0, 32, 131072, "mixed", 1, 0, 0),
    ("stream-64MiB-acc", 2, 32, 32, 32, 131072, "mixed", 0, 1, 1),
    ("below-64MiB", 2, 64, 0, 32, 131068, "mixed", 1, 0, 0),
] + [
    (f"uniform-r{r:g}-s{s:g}", 2, 16, 16, 8, 256, (r, s), i % 2, (i // 2) % 2, (i // 4) % 2) for i, (r, s) in enumerate(COMBOS)
] + [   # the shapes and inputs of tests/test_kernels.py::test_groupnorm_stats and tests/test_backward.py::test_groupnorm_silu_backward
    ("old-32-0-64", 2, 32, 0, 32, 64, "old", 1, 0, 0), ("old-64-32-16", 2, 64, 32, 32, 16, "old", 1, 0, 0),
    ("old-96-96-4", 2, 96, 96, 32, 4, "old", 1, 0, 0), ("old-32-0-1", 2, 32, 0, 32, 1, "old", 1, 0, 0),
    ("old-64-0-1024", 2, 64, 0, 32, 1024, "old", 0, 0, 0), ("old-32-0-256", 2, 32, 0, 32, 256, "old", 0, 0, 0),
]
GN_IDS = [c[0] for c in GN_CASES]
EPS_GN = 1e-5
OLD_GN_FWD = {"old-32-0-64", "old-64-32-16", "old-96-96-4", "old-32-0-1", "old-64-0-1024"}      # test_kernels.py::test_groupnorm_stats
OLD_GN_BWD = {"old-32-0-64", "old-64-32-16", "old-96-96-4", "old-32-0-256"}                     # test_backward.py::test_groupnorm_silu_backward


def _gn_tensors(case):
    cid, N, C1, C2, groups, HW, stats, act, acc1, acc2 = case
    seed = 100 + 13 * GN_IDS.index(cid)
    C = C1 + C2
    x = _gn_input(N, C, groups, HW, stats, seed)
    if stats == "old":
        x[:, C1:] = _randn((N, C2, HW), seed + 1)
    gamma, beta = _randn((C,), seed + 2) * 0.5 + 1.0, _randn((C,), seed + 3)
    return x, gamma.contiguous(), beta.contiguous()


def _gn_refs(x, gamma, beta, groups, act, da, dtype):
    """-> (y, a = act(y), dx, dgamma, dbeta, mean, rstd) in `dtype`."""
    xr, g, b = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.group_norm(xr, groups, g, b, EPS_GN)
    a = F.silu(y) if act else y
    grads = (None, None, None)
    if da is not None:
        a.backward(da.to(dtype))
        grads = (xr.grad, g.grad, b.grad)
    xg = x.to(dtype).reshape(x.shape[0], groups, -1)
    mean = xg.mean(-1)
    rstd = (xg.var(-1, unbiased=False) + EPS_GN).rsqrt()
    return (y.detach(), a.detach()) + grads + (mean, rstd)


def _split(x, C1, dev):
    x1 = x[:, :C1].contiguous().to(dev)
    x2 = x[:, C1:].contiguous().to(dev) if x.shape[1] > C1 else None
    return x1, x2


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", GN_CASES, ids=GN_IDS)
def test_groupnorm_forward_sweep(backend, case):
    """`adm_groupnorm_stats` and `adm_groupnorm_stats_ex`: y = x * scale + shift (the products in float64, so the figure is the kernel's scale and
    shift alone) and mean_rstd against float64; the two entries and two runs agree to the bit."""
    dev = select(backend)
    from audiodiffusion import ops
    cid, N, C1, C2, groups, HW, stats, act, acc1, acc2 = case
    C = C1 + C2
    x, gamma, beta = _gn_tensors(case)
    x1, x2 = _split(x, C1, dev)
    gd, bd = gamma.to(dev), beta.to(dev)
    sc, sh = ops.groupnorm_stats(x1, gd, bd, groups, EPS_GN, x2=x2)
    sc2, sh2, mr = ops.groupnorm_stats_ex(x1, gd, bd, groups, EPS_GN, x2=x2)
    sc3, sh3, mr3 = ops.groupnorm_stats_ex(x1, gd, bd, groups, EPS_GN, x2=x2)
    for a, b in ((sc, sc2), (sh, sh2), (sc2, sc3), (sh2, sh3), (mr, mr3)):
        assert torch.equal(a.cpu(), b.cpu()), (cid, "scale / shift / mean_rstd differ between the entries or between two runs")
    r64 = _gn_refs(x, gamma, beta, groups, 0, None, torch.float64)
    r32 = _gn_refs(x, gamma, beta, groups, 0, None, torch.float32)
    n = (C // groups) * HW
    tag = _tag(backend, cid, _gn_fwd_branch(HW))
    y = x.double() * sc.cpu().double()[:, :, None] + sh.cpu().double()[:, :, None]
    ceiling = None if cid not in OLD_GN_FWD else (2e-4 if n == 1 else 2e-5)
    _judge("adm_groupnorm_stats", "y", y, r64[0], r32[0], n, tag, ceiling=ceiling)
    _judge("adm_groupnorm_stats_ex", "mean", mr.cpu()[..., 0], r64[5], r32[5], n, tag)
    _judge("adm_groupnorm_stats_ex", "rstd", mr.cpu()[..., 1], r64[6], r32[6], n, tag)
    if stats == "mixed" and N * groups > 1:     # the constant group: var = 0 exactly, rstd = eps^-1/2
        assert abs(float(mr.cpu()[0, 1 % groups, 1]) / EPS_GN ** -0.5 - 1) < 4 * U and float(mr.cpu()[0, 1 % groups, 0]) == pytest.approx(CONST, rel=2 * U)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", GN_CASES, ids=GN_IDS)
def test_groupnorm_backward_sweep(backend, case):
    """`adm_groupnorm_backward`: dx1, dx2, dgamma, dbeta against float64 autograd of act(group_norm(cat(x1, x2))), every gradient buffer non-zero
    beforehand (dgamma / dbeta always accumulate; dx1 / dx2 under acc1 / acc2) and surrounded by a canary."""
    dev = select(backend)
    from audiodiffusion import ops
    nat, lib = _native()
    cid, N, C1, C2, groups, HW, stats, act, acc1, acc2 = case
    C = C1 + C2
    seed = 5000 + 17 * GN_IDS.index(cid)
    x, gamma, beta = _gn_tensors(case)
    da = _randn((N, C, HW), seed)
    r64 = _gn_refs(x, gamma, beta, groups, act, da, torch.float64)
    r32 = _gn_refs(x, gamma, beta, groups, act, da, torch.float32)
    x1, x2 = _split(x, C1, dev)
    gd, bd, dad = gamma.to(dev), beta.to(dev), da.to(dev)
    _, _, mr = ops.groupnorm_stats_ex(x1, gd, bd, groups, EPS_GN, x2=x2)
    # One element per group: xhat = 0 and dx = rstd * (g * gamma - mean(g * gamma)) = 0 exactly, dgamma = 0 too. max|ref| is rounding noise
    # there, so these two figures are divided by the size of the terms that cancel, eps^-1/2 * max|da * gamma| and max|da|, instead.
    degenerate = (C // groups) * HW == 1
    sx = EPS_GN ** -0.5 * float((da * gamma[None, :, None]).abs().max()) if degenerate else None
    sg = float(da.abs().max()) if degenerate else None
    init_x = _randn((N, C, HW), seed + 1, 0.5 * (sx or float(r64[2].abs().max())))   # what the gradient buffers hold beforehand (garbage where acc = 0)
    init_g = _randn((C,), seed + 2, 0.5 * (sg or float(r64[3].abs().max())))
    init_b = _randn((C,), seed + 3, 0.5 * float(r64[4].abs().max()))
    assert _gn_streaming(N, C, HW) == (cid.startswith("stream"))

    def run():
        dx1, w1 = _guarded(init_x[:, :C1].contiguous(), dev)
        dx2, w2 = _guarded(init_x[:, C1:].contiguous(), dev) if C2 else (None, None)
        dg, wg = _guarded(init_g, dev)
        db, wb = _guarded(init_b, dev)
        s12 = torch.empty((N, groups, 2), dtype=torch.float32, device=dev)
        nat.check(lib.adm_groupnorm_backward(nat.ptr(x1), C1, nat.ptr(x2), C2, nat.ptr(dad), N, HW, groups, nat.ptr(mr), nat.ptr(gd), nat.ptr(bd),
                                             act, nat.ptr(s12), nat.ptr(dg), nat.ptr(db), nat.ptr(dx1), acc1, nat.ptr(dx2), acc2,
                                             nat.stream_for(x1)))
        out = (dx1.cpu(), dx2.cpu() if C2 else None, dg.cpu(), db.cpu())
        for w in (w1, w2, wg, wb):
            assert w is None or _guard_intact(w), (cid, "a gradient buffer's surroundings were written")
        return out

    dx1, dx2, dg, db = run()
    cg = C // groups
    tag = _tag(backend, cid, _gn_bwd_branch(N, C, HW, acc1, acc2, C2))
    ceiling = 1e-4 if cid in OLD_GN_BWD else None

    def expect(ref, init, acc):
        return ref + init.to(ref.dtype) if acc else ref

    for r in (r64, r32):
        assert r[2].shape == (N, C, HW)
    _judge("adm_groupnorm_backward", "dx1", dx1, expect(r64[2][:, :C1], init_x[:, :C1], acc1), expect(r32[2][:, :C1], init_x[:, :C1], acc1),
           cg * HW, tag, ceiling=ceiling, scale=sx)
    if C2:
        _judge("adm_groupnorm_backward", "dx2", dx2, expect(r64[2][:, C1:], init_x[:, C1:], acc2), expect(r32[2][:, C1:], init_x[:, C1:], acc2),
               cg * HW, tag, ceiling=ceiling)
    _judge("adm_groupnorm_backward", "dgamma", dg, expect(r64[3], init_g, 1), expect(r32[3], init_g, 1), N * HW, tag, ceiling=ceiling, scale=sg)
    _judge("adm_groupnorm_backward", "dbeta", db, expect(r64[4], init_b, 1), expect(r32[4], init_b, 1), N * HW, tag, ceiling=ceiling)
    if not _gn_streaming(N, C, HW):             # dx is deterministic (block-ordered fp64 sums); dgamma / dbeta are atomics over n: not compared
        again = run()
        assert torch.equal(again[0], dx1) and (not C2 or torch.equal(again[1], dx2)), (cid, "dx differs between two runs")


FIN_CASES = [   # (id, C1, tiles1, C2, tiles2, groups)
    ("t1", 32, 1, 0, 0, 8), ("t255", 32, 255, 0, 0, 8), ("t256", 32, 256, 0, 0, 32), ("t257", 16, 257, 0, 0, 4),
    ("two-3-257-seam-in", 20, 3, 12, 257, 4), ("two-256-1-seam-on", 16, 256, 16, 1, 4),
]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", FIN_CASES, ids=[c[0] for c in FIN_CASES])
def test_groupnorm_finalize_sweep(backend, case):
    """`adm_groupnorm_finalize` on fp64 (sum, sum of squares) partials built here, per channel over `tiles` uneven pixel tiles: inside the bars, and
    equal to the read pass. Both add the same numbers in float64 in another order, so mean and rstd agree to a rounding of the float they are
    stored as (2u relative): scale within 4u of its size and shift within 8u of |scale * mean| + |beta|."""
    dev = select(backend)
    from audiodiffusion import ops
    cid, C1, t1, C2, t2, groups = case
    N, HW, C = 2, 1024, C1 + C2
    seed = 9000 + 7 * [c[0] for c in FIN_CASES].index(cid)
    x = _gn_input(N, C, groups, HW, "mixed", seed)
    gamma, beta = _randn((C,), seed + 2) * 0.5 + 1.0, _randn((C,), seed + 3)

    def partials(part, tiles):
        st = torch.zeros(part.shape[:2] + (tiles, 2), dtype=torch.float64)
        for t, chunk in enumerate(torch.tensor_split(part.double(), tiles, dim=2)):
            st[:, :, t, 0], st[:, :, t, 1] = chunk.sum(-1), (chunk * chunk).sum(-1)
        return st.contiguous().to(dev)

    st1 = partials(x[:, :C1], t1)
    st2 = partials(x[:, C1:], t2) if C2 else None
    gd, bd = gamma.to(dev), beta.to(dev)
    sc, sh = ops.groupnorm_finalize(st1, gd, bd, groups, EPS_GN, HW, st2=st2)
    sc_b, sh_b = ops.groupnorm_finalize(st1, gd, bd, groups, EPS_GN, HW, st2=st2)
    assert torch.equal(sc.cpu(), sc_b.cpu()) and torch.equal(sh.cpu(), sh_b.cpu())
    x1, x2 = _split(x, C1, dev)
    rsc, rsh = ops.groupnorm_stats(x1, gd, bd, groups, EPS_GN, x2=x2)
    r64 = _gn_refs(x, gamma, beta, groups, 0, None, torch.float64)
    r32 = _gn_refs(x, gamma, beta, groups, 0, None, torch.float32)
    n = (C // groups) * HW
    tag = _tag(backend, cid, f"tiles{t1}" + (f"+{t2}" if C2 else ""))
    y = x.double() * sc.cpu().double()[:, :, None] + sh.cpu().double()[:, :, None]
    _judge("adm_groupnorm_finalize", "y", y, r64[0], r32[0], n, tag)
    sc, sh, rsc, rsh = (t.cpu().double() for t in (sc, sh, rsc, rsh))
    mean_c = r64[5].repeat_interleave(C // groups, dim=1)
    d_sc, d_sh = float(((sc - rsc).abs() / rsc.abs()).max()), float(((sh - rsh).abs() / ((rsc * mean_c).abs() + beta.double().abs())).max())
    print(f"NORM_SWEEP {tag} entry=adm_groupnorm_finalize out=vs_read_pass scale_rel={d_sc:.3e} shift_rel={d_sh:.3e}")
    assert d_sc <= 4 * U and d_sh <= 8 * U, (cid, d_sc, d_sh)


# ================================================================ B. LayerNorm and GEGLU
LN_C, LN_T, LN_RATIO = [2, 3, 4, 32, 96, 320, 1280], [5, 63, 64, 65, 256, 257, 320, 4096], [0.0, 0.15, 30.0]
EPS_LN = 1e-5


def _ln_cases():
    out = []
    for k, C in enumerate(LN_C):
        for j, T in enumerate(LN_T):            # N and accumulate walk all four pairs along C at every T; the mean / std ratio walks along both
            N = 1 if ((k + j) % 2 or C * T > 500_000) else 3
            out.append((f"C{C}-T{T}", N, C, T, LN_RATIO[(k + 2 * j) % 3], (k // 2 + j) % 2))
    out += [("old-2-32-32", 2, 32, 32, "old", 0), ("old-1-96-256", 1, 96, 256, "old", 0), ("old-3-64-5", 3, 64, 5, "old", 0),
            ("old-2-128-128", 2, 128, 128, "old", 0), ("old-1-320-256", 1, 320, 256, "old", 0)]
    return out


LN_CASES = _ln_cases()
LN_IDS = [c[0] for c in LN_CASES]


def _ln_fwd_branch(C, T):
    return "tile64" if T % 64 == 0 and C >= 4 else "lane"


def _ln_bwd_branch(T, acc):
    return ("wg1" if T <= 256 else f"wg{-(-T // 256)}") + ("-full" if T % 256 == 0 else "-ragged") + f"-acc{acc}"


def _ln_refs(x, gamma, beta, dy, dtype):
    xr, g, b = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    y = F.layer_norm(xr.permute(0, 2, 1), (x.shape[1],), g, b, EPS_LN).permute(0, 2, 1)
    y.backward(dy.to(dtype))
    xd = x.to(dtype)
    mean = xd.mean(1)
    rstd = (xd.var(1, unbiased=False) + EPS_LN).rsqrt()
    return y.detach(), xr.grad, g.grad, b.grad, mean, rstd


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", LN_CASES, ids=LN_IDS)
def test_layernorm_sweep(backend, case):
    """`adm_layernorm_nct` and `adm_layernorm_nct_backward` (dx (=|+=), its saved statistics, dgamma / dbeta added onto non-zero buffers)."""
    dev = select(backend)
    from audiodiffusion import ops
    nat, lib = _native()
    cid, N, C, T, ratio, acc = case
    seed = 20000 + 11 * LN_IDS.index(cid)
    x = _randn((N, C, T), seed) * 2 + 0.3 if ratio == "old" else _randn((N, C, T), seed) + ratio
    gamma, beta, dy = _randn((C,), seed + 1) + 1.0, _randn((C,), seed + 2), _randn((N, C, T), seed + 3)
    r64, r32 = _ln_refs(x, gamma, beta, dy, torch.float64), _ln_refs(x, gamma, beta, dy, torch.float32)
    xd, gd, bd, dyd = x.to(dev), gamma.to(dev), beta.to(dev), dy.to(dev)
    old = ratio == "old"
    tag = _tag(backend, cid, _ln_fwd_branch(C, T))
    y = ops.layernorm_nct(xd, gd, bd, EPS_LN)
    _judge("adm_layernorm_nct", "y", y, r64[0], r32[0], C, tag, ceiling=2e-6 if old else None)
    assert torch.equal(ops.layernorm_nct(xd, gd, bd, EPS_LN).cpu(), y.cpu())
    if N > 1:                                   # a sample's bits do not depend on the batch it is in
        assert torch.equal(ops.layernorm_nct(xd[N - 1:].contiguous(), gd, bd, EPS_LN).cpu(), y[N - 1:].cpu())

    init_x = _randn((N, C, T), seed + 4, 0.5 * float(r64[1].abs().max()))
    init_g, init_b = _randn((C,), seed + 5, 0.5 * float(r64[2].abs().max())), _randn((C,), seed + 6, 0.5 * float(r64[3].abs().max()))

    def run():
        dx, wx = _guarded(init_x, dev)
        dg, wg = _guarded(init_g, dev)
        db, wb = _guarded(init_b, dev)
        st, ws = _guarded(torch.zeros(2 * N * T), dev)
        nat.check(lib.adm_layernorm_nct_backward(nat.ptr(xd), nat.ptr(dyd), nat.ptr(gd), nat.ptr(dx), acc, nat.ptr(st), nat.ptr(dg), nat.ptr(db),
                                                 N, C, T, EPS_LN, nat.stream_for(xd)))
        out = tuple(t.cpu() for t in (dx, dg, db, st))
        assert all(_guard_intact(w) for w in (wx, wg, wb, ws)), (cid, "a buffer's surroundings were written")
        return out

    dx, dg, db, st = run()
    tag = _tag(backend, cid, _ln_bwd_branch(T, acc))
    ceiling = 1e-5 if old else None
    ex = (lambda r: r[1] + init_x.to(r[1].dtype)) if acc else (lambda r: r[1])
    _judge("adm_layernorm_nct_backward", "dx", dx, ex(r64), ex(r32), C, tag, ceiling=ceiling)
    _judge("adm_layernorm_nct_backward", "dgamma", dg, r64[2] + init_g.double(), r32[2] + init_g, N * T, tag, ceiling=ceiling)
    _judge("adm_layernorm_nct_backward", "dbeta", db, r64[3] + init_b.double(), r32[3] + init_b, N * T, tag, ceiling=ceiling)
    st = st.reshape(N, T, 2)
    _judge("adm_layernorm_nct_backward", "mean", st[..., 0], r64[4], r32[4], C, tag)
    _judge("adm_layernorm_nct_backward", "rstd", st[..., 1], r64[5], r32[5], C, tag)
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(again, (dx, dg, db, st.reshape(-1)))), (cid, "two runs differ")


# (id, N, C4, T, gate scale)
GEGLU_CASES = [("35-s1", 2, 5, 7, 1), ("35-s8", 2, 5, 7, 8), ("1056-s3", 1, 32, 33, 3), ("300-s8", 3, 3, 100, 8), ("300-s1", 3, 3, 100, 1),
               ("1024-s3", 2, 32, 32, 3), ("257-s8", 1, 1, 257, 8), ("old", 2, 32, 32, "old")]


def _geglu_refs(x, dy, dtype):
    xr = x.to(dtype).clone().requires_grad_(True)
    h, gate = xr.chunk(2, dim=1)
    out = h * F.gelu(gate)
    out.backward(dy.to(dtype))
    return out.detach(), xr.grad


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", GEGLU_CASES, ids=[c[0] for c in GEGLU_CASES])
def test_geglu_sweep(backend, case):
    """`adm_geglu` and `adm_geglu_backward`; gate scale 8 takes |gate| to about 30, where 1 + erf cancels and exp(-g^2 / 2) underflows."""
    dev = select(backend)
    from audiodiffusion import ops
    cid, N, C4, T, scale = case
    seed = 30000 + 3 * [c[0] for c in GEGLU_CASES].index(cid)
    x = _randn((N, 2 * C4, T), seed)
    if scale == "old":
        x = x * 3
    else:
        x[:, C4:] *= scale
        if scale == 8:
            assert float(x[:, C4:].abs().max()) > 16
    dy = _randn((N, C4, T), seed + 1)
    r64, r32 = _geglu_refs(x, dy, torch.float64), _geglu_refs(x, dy, torch.float32)
    per = C4 * T
    tag = _tag(backend, cid, "per%256=0" if per % 256 == 0 else "ragged")
    ceiling = 2e-6 if scale == "old" else None
    out = ops.geglu(x.to(dev))
    _judge("adm_geglu", "out", out, r64[0], r32[0], 4, tag, ceiling=ceiling)
    dx = ops.geglu_backward(x.to(dev), dy.to(dev))
    _judge("adm_geglu_backward", "dh", dx[:, :C4], r64[1][:, :C4], r32[1][:, :C4], 4, tag, ceiling=ceiling)
    _judge("adm_geglu_backward", "dgate", dx[:, C4:], r64[1][:, C4:], r32[1][:, C4:], 4, tag, ceiling=ceiling)
    assert torch.equal(ops.geglu(x.to(dev)).cpu(), out.cpu()) and torch.equal(ops.geglu_backward(x.to(dev), dy.to(dev)).cpu(), dx.cpu())


# ================================================================ C. reductions and small dense layers of the backward pass
# (id, N, C, HW, nc_stride (0: out_nc NULL), nc_accumulate, out_c given)
CS_CASES = [
    ("hw7", 3, 5, 7, 5, 0, 1), ("hw64", 3, 32, 64, 32, 0, 1), ("hw64-slice-acc", 2, 8, 64, 24, 1, 1), ("hw3072", 1, 4, 3072, 4, 0, 1),
    ("hw3076-slice", 3, 4, 3076, 9, 0, 1), ("hw4096-acc", 1, 3, 4096, 3, 1, 0), ("hw16388-slice-acc", 2, 3, 16388, 7, 1, 1),
    ("hw65536", 1, 2, 65536, 2, 0, 1), ("hw4098-c-only", 3, 4, 4098, 0, 0, 1), ("hw65536-slice", 3, 2, 65536, 5, 0, 0),
    ("old", 3, 32, 64, 32, 0, 1),
]


def _cs_branch(HW, nc_stride, C, acc, has_c):
    if HW % 4:
        walk = "scalar"
    else:
        n4 = HW // 4
        walk = "v4" + ("_chains4" if n4 > 768 else "") + ("_rem" if n4 <= 768 or n4 % 1024 else "")
    nc = "nc_null" if nc_stride == 0 else ("nc_slice" if nc_stride > C else "nc_dense") + f"-acc{acc}"
    return f"{walk}-{nc}-{'c' if has_c else 'c_null'}"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", CS_CASES, ids=[c[0] for c in CS_CASES])
def test_chan_sums_sweep(backend, case):
    dev = select(backend)
    nat, lib = _native()
    cid, N, C, HW, ncs, acc, has_c = case
    seed = 40000 + 5 * [c[0] for c in CS_CASES].index(cid)
    dy = _randn((N, C, HW), seed) + (0.0 if cid == "old" else 0.25)
    init_nc, init_c = _randn((N, max(ncs, 1)), seed + 1, 0.5 * math.sqrt(HW)), _randn((C,), seed + 2, 0.5 * math.sqrt(N * HW))
    dyd = dy.to(dev)

    def run():
        nc, wn = _guarded(init_nc, dev)
        oc, wc = _guarded(init_c, dev)
        nat.check(lib.adm_chan_sums(nat.ptr(dyd), N, C, HW, nat.ptr(nc) if ncs else None, ncs, acc, nat.ptr(oc) if has_c else None,
                                    nat.stream_for(dyd)))
        assert _guard_intact(wn) and _guard_intact(wc)
        return nc.cpu(), oc.cpu()

    nc, oc = run()
    tag = _tag(backend, cid, _cs_branch(HW, ncs, C, acc, has_c))
    ceiling = 1e-4 if cid == "old" else None
    s64, s32 = dy.double().sum(2), dy.sum(2)
    if ncs:
        e = (lambda s: s + init_nc[:, :C].to(s.dtype)) if acc else (lambda s: s)
        _judge("adm_chan_sums", "out_nc", nc[:, :C], e(s64), e(s32), HW, tag, ceiling=ceiling)
        assert torch.equal(nc[:, C:], init_nc[:, C:]), (cid, "the columns behind the slice were written")
        assert torch.equal(run()[0], nc), (cid, "out_nc differs between two runs")
    else:
        assert torch.equal(nc, init_nc)
    if has_c:                                   # always accumulated (atomics over n: no bit identity asserted)
        _judge("adm_chan_sums", "out_c", oc, dy.double().sum((0, 2)) + init_c.double(), dy.sum((0, 2)) + init_c, N * HW, tag, ceiling=ceiling)
    else:
        assert torch.equal(oc, init_c)


LIN_SHAPES = [(1, 7, 5), (4, 96, 64), (33, 100, 130), (16, 1248, 512), (3, 512, 128)]
# (B, J, K, x_silu, ldy - J, col0, outputs): outputs "wx" both, "w" dX NULL, "x" dW NULL
LIN_CASES = ([(B, J, K, s, 0, 0, "wx") for (B, J, K) in LIN_SHAPES for s in (0, 1)]
             + [(33, 100, 130, 1, 57, 20, "wx"), (16, 1248, 512, 0, 8736, 4992, "wx"), (1, 7, 5, 0, 3, 3, "wx"), (3, 512, 128, 1, 512, 512, "x"),
                (4, 96, 64, 1, 0, 0, "w"), (4, 96, 64, 0, 0, 0, "x"), (33, 100, 130, 0, 1, 0, "w")])


def _lin_id(c):
    B, J, K, s, pad, col0, outs = c
    return f"B{B}-J{J}-K{K}-silu{s}-ldy{J + pad}-{outs}"


def _lin_branch(c):
    B, J, K, s, pad, col0, outs = c
    return f"{'k%16=0' if K % 16 == 0 else 'k_ragged'}-{'ldy>J' if pad else 'dense'}-silu{s}-{outs}"


def _lin_refs(dY, X, W, x_silu, dtype):
    Xr, Wr, b = X.to(dtype).clone().requires_grad_(True), W.to(dtype).clone().requires_grad_(True), torch.zeros(W.shape[0], dtype=dtype, requires_grad=True)
    F.linear(F.silu(Xr) if x_silu else Xr, Wr, b).backward(dY.to(dtype))
    return Wr.grad, b.grad, Xr.grad


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", LIN_CASES, ids=[_lin_id(c) for c in LIN_CASES])
def test_linear_backward_sweep(backend, case):
    """`adm_linear_backward`: dW and db are `+=` onto non-zero buffers, dX is written; dY may be a column slice of a wider matrix whose other
    columns hold NaN; a NULL dW leaves db alone, a NULL dX writes nothing."""
    dev = select(backend)
    nat, lib = _native()
    B, J, K, x_silu, pad, col0, outs = case
    seed = 50000 + 9 * LIN_CASES.index(case)
    ldy = J + pad
    dY = _randn((B, J), seed)
    X, W = _randn((B, K), seed + 1), _randn((J, K), seed + 2, K ** -0.5)
    wide = torch.full((B, ldy), float("nan"))
    wide[:, col0:col0 + J] = dY
    assert 0 <= col0 <= pad
    r64, r32 = _lin_refs(dY, X, W, x_silu, torch.float64), _lin_refs(dY, X, W, x_silu, torch.float32)
    init_w, init_b = _randn((J, K), seed + 3, 0.5 * float(r64[0].abs().max())), _randn((J,), seed + 4, 0.5 * float(r64[1].abs().max()))
    wided, Xd, Wd = wide.to(dev), X.to(dev), W.to(dev)
    dYp = nat.C.c_void_p(wided.data_ptr() + 4 * col0)

    def run():
        dW, ww = _guarded(init_w, dev)
        db, wb = _guarded(init_b, dev)
        dX, wx = _guarded(torch.full((B, K), CANARY), dev)
        nat.check(lib.adm_linear_backward(dYp, ldy, nat.ptr(Xd), nat.ptr(Wd), B, J, K, x_silu, nat.ptr(dW) if "w" in outs else None, nat.ptr(db),
                                          nat.ptr(dX) if "x" in outs else None, nat.stream_for(Xd)))
        assert all(_guard_intact(w) for w in (ww, wb, wx))
        return dW.cpu(), db.cpu(), dX.cpu()

    dW, db, dX = run()
    tag = _tag(backend, _lin_id(case), _lin_branch(case))
    ceiling = 1e-5 if (B, J, K, pad) == (4, 96, 64, 0) else None
    if "w" in outs:
        _judge("adm_linear_backward", "dW", dW, r64[0] + init_w.double(), r32[0] + init_w, B, tag, ceiling=ceiling)
        _judge("adm_linear_backward", "db", db, r64[1] + init_b.double(), r32[1] + init_b, B, tag, ceiling=ceiling)
    else:
        assert torch.equal(dW, init_w) and torch.equal(db, init_b), "a NULL dW must leave dW and db alone"
    if "x" in outs:
        _judge("adm_linear_backward", "dX", dX, r64[2], r32[2], J, tag, ceiling=ceiling)
    else:
        assert bool((dX == CANARY).all()), "a NULL dX must write nothing"
    again = run()
    assert all(torch.equal(a, b) for a, b in zip(again, (dW, db, dX))), "two runs differ"


# (id, N, per_sample, dst_bs - per_sample, src_bs - per_sample, accumulate, pointer offset in floats)
ACC_CASES = [
    ("v4", 3, 1024, 0, 0, 1, 0), ("v4-store", 1, 1024, 0, 0, 0, 0), ("v4-dst-slice", 3, 256, 512, 0, 1, 0), ("v4-src-slice", 2, 260, 0, 64, 0, 0),
    ("scalar-size", 3, 1023, 0, 0, 1, 0), ("scalar-size-slice", 2, 30, 3, 0, 0, 0), ("scalar-stride", 2, 64, 2, 0, 1, 0),
    ("scalar-misaligned", 3, 1024, 0, 0, 1, 1), ("scalar-misaligned-slice", 2, 512, 256, 0, 0, 3), ("v4-grid-stride", 1, 4 * 1048576 + 8, 0, 0, 1, 0),
    ("one", 1, 1, 0, 0, 1, 0),
]


def _acc_branch(per, dpad, spad, off):
    vec = (per | (per + dpad) | (per + spad)) % 4 == 0 and off % 4 == 0
    return ("float4" if vec else "scalar") + ("-dst_slice" if dpad else "") + ("-src_slice" if spad else "") + ("-grid_stride" if per // 4 > 4096 * 256 else "")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", ACC_CASES, ids=[c[0] for c in ACC_CASES])
def test_accumulate_sweep(backend, case):
    """`adm_accumulate`: one fp32 addition per element, so beside the bars the result equals torch's fp32 sum to the bit."""
    dev = select(backend)
    nat, lib = _native()
    cid, N, per, dpad, spad, acc, off = case
    seed = 60000 + [c[0] for c in ACC_CASES].index(cid)
    dbs, sbs = per + dpad, per + spad
    dst0, src = _randn((N, dbs), seed), _randn((N, sbs), seed + 1)
    whole = torch.full((N * dbs + 2 * GUARD + 4,), CANARY)
    base = GUARD + off                           # GUARD floats are 256 bytes: `off` floats away from a 16-byte boundary
    whole[base:base + N * dbs] = dst0.reshape(-1)
    srcw = torch.zeros(N * sbs + 4)
    srcw[off:off + N * sbs] = src.reshape(-1)
    whole, srcw = whole.to(dev), srcw.to(dev)
    assert whole.data_ptr() % 16 == 0 and srcw.data_ptr() % 16 == 0
    nat.check(lib.adm_accumulate(nat.C.c_void_p(whole.data_ptr() + 4 * base), dbs, nat.C.c_void_p(srcw.data_ptr() + 4 * off), sbs, per, N, acc,
                                 nat.stream_for(whole)))
    whole = whole.cpu()
    got = whole[base:base + N * dbs].reshape(N, dbs)
    assert bool((whole[:base] == CANARY).all()) and bool((whole[base + N * dbs:] == CANARY).all()), (cid, "written outside the destination")
    assert torch.equal(got[:, per:], dst0[:, per:]), (cid, "written behind a sample's slice")
    want32 = dst0[:, :per] + src[:, :per] if acc else src[:, :per].clone()
    want64 = dst0[:, :per].double() + src[:, :per].double() if acc else src[:, :per].double()
    _judge("adm_accumulate", "dst", got[:, :per], want64, want32, 4, _tag(backend, cid, _acc_branch(per, dpad, spad, off)), ceiling=1e-4)
    assert torch.equal(got[:, :per], want32)


# (id, planes (N, C), H, W, accumulate)
POOL_CASES = [("2x2", (1, 1), 2, 2, 0), ("old-8x16", (2, 16), 8, 16, 0), ("6x10-acc", (3, 5), 6, 10, 1), ("64x2-acc", (2, 3), 64, 2, 1),
              ("grid-stride", (1, 1), 2050, 2048, 0), ("grid-stride-acc", (1, 1), 2048, 2052, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", POOL_CASES, ids=[c[0] for c in POOL_CASES])
def test_sumpool2x2_sweep(backend, case):
    dev = select(backend)
    from audiodiffusion import ops
    cid, (N, C), H, W, acc = case
    seed = 70000 + [c[0] for c in POOL_CASES].index(cid)
    x, init = _randn((N, C, H, W), seed), _randn((N, C, H // 2, W // 2), seed + 1, 2.0)
    out, whole = _guarded(init, dev)
    assert ops.sumpool2x2(x.to(dev), out=out, accumulate=bool(acc)) is out
    assert _guard_intact(whole)

    def ref(dtype):
        s = x.to(dtype).reshape(N, C, H // 2, 2, W // 2, 2).sum((3, 5))
        return s + init.to(dtype) if acc else s

    stride = (N * C * (H // 2) * (W // 2) + 255) // 256 > 4096
    _judge("adm_sumpool2x2", "out", out, ref(torch.float64), ref(torch.float32), 4, _tag(backend, cid, f"acc{acc}" + ("-grid_stride" if stride else "")),
           ceiling=1e-4)


# ================================================================ D. time embedding
TE_SHAPES = [(128, 512), (128, 256), (64, 256), (32, 128), (32, 100), (20, 52), (32, 96)]
TE_T = [0.0, 1.0, 999.0, 0.5]
TE_CASES = [(di, de, flip, B, (3 * TE_SHAPES.index((di, de)) + flip + [1, 3, 8].index(B)) % 4, 1)
            for (di, de) in TE_SHAPES for flip in (0, 1) for B in (1, 3, 8)] + [(128, 512, 1, 3, 0, 0), (64, 256, 0, 1, 2, 0)]


def _te_id(c):
    di, de, flip, B, t0, aligned = c
    return f"in{di}-emb{de}-flip{flip}-B{B}-t{TE_T[t0]:g}" + ("" if aligned else "-misaligned")


def _te_branch(di, de, aligned):
    """time_embedding_kernel: float4 row groups need both widths % 32 == 0 and 16-byte aligned weights; linear_1 has a register form for
    128 -> k * 128, linear_2 one for 512 -> 512, and the float4 form of linear_2 needs the rows of a workgroup (dim_emb / 8, rounded up) % 8 == 0."""
    vec = di % 32 == 0 and de % 32 == 0 and aligned
    rows = -(-de // 8)
    l1 = "l1_in128" if vec and di == 128 and de % 128 == 0 else ("l1_vec" if vec else "l1_scalar")
    l2 = "l2_512" if vec and de == 512 and rows % 8 == 0 else ("l2_vec" if vec and rows % 8 == 0 else "l2_scalar")
    return f"{l1}-{l2}-rows%8={'0' if rows % 8 == 0 else 'r'}"


def _silu(v):
    return v * torch.sigmoid(v)


def _te_refs(arg, flip, w1, b1, w2, b2, dtype):
    """arg = float32(t * freq), the fp32 product of the kernel (and of diffusers); everything after it in `dtype`."""
    a = arg.to(dtype)
    sinus = torch.cat([a.cos(), a.sin()] if flip else [a.sin(), a.cos()], dim=1)
    z = sinus @ w1.to(dtype).T + b1.to(dtype)
    emb = _silu(z) @ w2.to(dtype).T + b2.to(dtype)
    return sinus, z, emb, _silu(emb)


def _misaligned(t, dev):
    """`t` on the device at an address 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 8, dtype=torch.float32, device=dev)
    off = next(o for o in range(1, 8) if (flat.data_ptr() + 4 * o) % 16 == 4)
    view = flat[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", TE_CASES, ids=[_te_id(c) for c in TE_CASES])
def test_time_embedding_sweep(backend, case):
    """`adm_time_embedding`: emb, emb_act = silu(emb), save_z and save_sinus against float64 of linear_2(silu(linear_1([cos | sin](float32(t * freq)))))."""
    dev = select(backend)
    from audiodiffusion import ops
    di, de, flip, B, t0, aligned = case
    seed = 80000 + 7 * TE_CASES.index(case)
    half = di // 2
    t = torch.tensor([TE_T[(t0 + b) % 4] for b in range(B)], dtype=torch.float32)
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    w1, b1 = _randn((de, di), seed, di ** -0.5), _randn((de,), seed + 1, 0.1)
    w2, b2 = _randn((de, de), seed + 2, de ** -0.5), _randn((de,), seed + 3, 0.1)
    arg = t[:, None] * freqs[None, :]
    assert arg.dtype == torch.float32
    r64, r32 = _te_refs(arg, flip, w1, b1, w2, b2, torch.float64), _te_refs(arg, flip, w1, b1, w2, b2, torch.float32)
    put = (lambda w: w.to(dev)) if aligned else (lambda w: _misaligned(w, dev))
    td, fd, w1d, b1d, w2d, b2d = t.to(dev), freqs.to(dev), put(w1), b1.to(dev), put(w2), b2.to(dev)
    emb, act, sinus, z = ops.time_embedding(td, fd, w1d, b1d, w2d, b2d, flip=bool(flip), save=True)
    tag = _tag(backend, _te_id(case), _te_branch(di, de, bool(aligned)))
    _judge("adm_time_embedding", "save_sinus", sinus, r64[0], r32[0], 4, tag)
    _judge("adm_time_embedding", "save_z", z, r64[1], r32[1], di, tag)
    _judge("adm_time_embedding", "emb", emb, r64[2], r32[2], max(di, de), tag, ceiling=1e-4)
    _judge("adm_time_embedding", "emb_act", act, r64[3], r32[3], max(di, de), tag, ceiling=1e-4)
    _judge("adm_time_embedding", "emb_act_of_emb", act, _silu(emb.cpu().double()), _silu(emb.cpu()), 4, tag)     # emb_act is the SiLU of the emb beside it
    emb_b, act_b = ops.time_embedding(td, fd, w1d, b1d, w2d, b2d, flip=bool(flip))          # the optional outputs left out: the same bits
    assert torch.equal(emb_b.cpu(), emb.cpu()) and torch.equal(act_b.cpu(), act.cpu())
    if B > 1:                                   # a sample's bits do not depend on the batch it is in
        alone, _ = ops.time_embedding(td[B - 1:].contiguous(), fd, w1d, b1d, w2d, b2d, flip=bool(flip))
        assert torch.equal(alone.cpu(), emb[B - 1:].cpu())


TP_B, TP_K, TP_R = [1, 7, 8, 9, 32], [512, 128, 100], [9984, 50, 17]
TP_CASES = [(B, K, R) for B in TP_B for K in TP_K for R in TP_R]


def _tp_branch(B, K, R, activated):
    """launch_temb_proj: one wave per row below eight samples, else eight samples staged in LDS per workgroup of 16 rows, with a register form
    for K = 512; ragged: rows % 16 (staged) or % 4 (per row) and samples % 8."""
    act = "act" if activated else "raw"
    if B < 8:
        return f"row<{act}>-{'r%4=0' if R % 4 == 0 else 'r_ragged'}"
    return f"staged<{act}>-{'k512' if K == 512 else 'k_generic'}-{'r%16=0' if R % 16 == 0 else 'r_ragged'}-{'b%8=0' if B % 8 == 0 else 'b_ragged'}"


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("B,K,R", TP_CASES, ids=[f"B{b}-K{k}-R{r}" for b, k, r in TP_CASES])
def test_temb_proj_sweep(backend, B, K, R):
    """`adm_temb_proj` from emb (the kernel applies the SiLU) and from silu(emb) (the form the executors launch); eight canary rows behind `out`."""
    dev = select(backend)
    nat, lib = _native()
    seed = 90000 + 3 * TP_CASES.index((B, K, R))
    emb, w, bias = _randn((B, K), seed, 1.5), _randn((R, K), seed + 1, K ** -0.5), _randn((R,), seed + 2, 0.3)
    emb_act = _silu(emb)                         # fp32: what the activated form is given
    wd, bd = w.to(dev), bias.to(dev)
    for activated, src in ((0, emb), (1, emb_act)):
        ref64 = (src.double() if activated else _silu(src.double())) @ w.double().T + bias.double()
        ref32 = (src if activated else _silu(src)) @ w.T + bias
        srcd = src.to(dev)

        def run():
            whole = torch.full((B + 8, R), CANARY, dtype=torch.float32, device=dev)
            nat.check(lib.adm_temb_proj(nat.ptr(srcd), nat.ptr(wd), nat.ptr(bd), nat.ptr(whole), B, K, R, activated, nat.stream_for(srcd)))
            whole = whole.cpu()
            assert bool((whole[B:] == CANARY).all()), ((B, K, R), "rows behind the batch were written")
            return whole[:B]

        out = run()
        _judge("adm_temb_proj", "temb", out, ref64, ref32, K, _tag(backend, f"B{B}-K{K}-R{R}", _tp_branch(B, K, R, activated)), ceiling=1e-4)
        assert torch.equal(run(), out), "two runs differ"


# ================================================================ coverage of the lists above (no library needed)
def test_case_lists_reach_every_branch():
    """Every branch named in the headers of the families is reached by at least one case; the labels are the ones the cases print."""
    # --- A. GroupNorm forward walks
    fwd = {_gn_fwd_branch(c[5]) for c in GN_CASES}
    assert fwd >= {"scalar", "planes_sub", "float4_flat", "planes256_rem", "planes256_deep", "planes256_deep_rem"}, fwd
    hws = {c[5] for c in GN_CASES}
    assert hws >= {1, 24, 384, 1024, 1028, 4096, 4100, 4160, 4608, 8192, 65536, 131072, 131068}, hws
    # backward: in-flight iterations of both kernels, grids, streaming, scalar walk, accumulate flags
    bwd = [_gn_bwd_branch(c[1], c[2] + c[3], c[5], c[8], c[9], c[3]) for c in GN_CASES]
    for needle in ("-su1-", "-su2-", "-su4-", "-su4+-", "-au1-", "-au2-", "-au3-", "-au4-", "-gx1-", "-gx2-", "-gx3-", "-gx16-", "-gx32-", "nt-v4", "ld-v4",
                   "ld-scalar-gx1", "ld-scalar-gx2", "-acc00", "-acc01", "-acc10", "-acc11", "-acc0x", "-acc1x"):
        assert any(needle in b for b in bwd), (needle, bwd)
    assert any(b.startswith("nt-") and b.endswith("acc11") for b in bwd)                     # the streaming apply with both accumulate loads
    assert {c[1] for c in GN_CASES} == {1, 2, 3} and {c[4] for c in GN_CASES} >= {32, 8, 4} and {c[7] for c in GN_CASES} == {0, 1}
    assert any((c[2] + c[3]) // c[4] == 1 for c in GN_CASES)                                 # cg = 1
    seams = {(c[2] % ((c[2] + c[3]) // c[4]) == 0) for c in GN_CASES if c[3]}                # the seam of a virtual concat: on / inside a group
    assert seams == {True, False}
    assert {c[6] for c in GN_CASES if isinstance(c[6], tuple)} == set(COMBOS)
    assert sorted(_gn_streaming(c[1], c[2] + c[3], c[5]) for c in GN_CASES if c[5] in (131072, 131068)) == [False, True, True]
    assert {t for c in FIN_CASES for t in (c[2], c[4])} >= {1, 255, 256, 257} and any(c[3] and c[2] != c[4] for c in FIN_CASES)
    # --- B. LayerNorm
    assert {(c[2], c[3]) for c in LN_CASES} >= {(C, T) for C in LN_C for T in LN_T}
    assert {_ln_fwd_branch(c[2], c[3]) for c in LN_CASES} == {"tile64", "lane"}
    assert any(c[2] < 4 and c[3] % 64 == 0 for c in LN_CASES) and any(c[2] >= 4 and c[3] % 64 for c in LN_CASES)      # both halves of the rule
    for T_side in (lambda T: T < 256, lambda T: T == 256, lambda T: T > 256):
        assert {(c[1] > 1, c[5]) for c in LN_CASES if T_side(c[3])} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    assert {c[4] for c in LN_CASES} >= set(LN_RATIO)
    assert any((c[2] * c[3]) % 256 for c in GEGLU_CASES) and {c[4] for c in GEGLU_CASES} >= {1, 3, 8}
    # --- C. reductions
    cs = [_cs_branch(c[3], c[4], c[2], c[5], c[6]) for c in CS_CASES]
    for needle in ("scalar-", "v4_rem-", "v4_chains4-", "v4_chains4_rem-", "nc_slice-acc0", "nc_slice-acc1", "nc_dense-acc0", "nc_dense-acc1", "nc_null", "-c_null"):
        assert any(needle in b for b in cs), (needle, cs)
    assert {c[:3] for c in LIN_CASES} == set(LIN_SHAPES) and {(c[:3], c[3]) for c in LIN_CASES} >= {(s, x) for s in LIN_SHAPES for x in (0, 1)}
    lin = [_lin_branch(c) for c in LIN_CASES]
    for needle in ("k_ragged-", "k%16=0-", "-ldy>J-", "-dense-", "-w", "-x", "-wx"):
        assert any(needle in b for b in lin), (needle, lin)
    assert any(c[4] and c[5] for c in LIN_CASES) and any(c[:3] == (16, 1248, 512) and c[4] for c in LIN_CASES)       # a stacked time_emb_proj slice
    acc = {_acc_branch(c[2], c[3], c[4], c[6]) for c in ACC_CASES}
    assert acc >= {"float4", "float4-dst_slice", "float4-src_slice", "scalar", "scalar-dst_slice", "float4-grid_stride"}, acc
    assert any(c[6] % 4 for c in ACC_CASES) and any(c[2] % 4 for c in ACC_CASES) and {c[5] for c in ACC_CASES} == {0, 1}
    assert {c[4] for c in POOL_CASES} == {0, 1}
    # --- D. time embedding
    te = {_te_branch(c[0], c[1], bool(c[5])) for c in TE_CASES}
    assert te >= {"l1_in128-l2_512-rows%8=0", "l1_in128-l2_vec-rows%8=0", "l1_vec-l2_vec-rows%8=0", "l1_vec-l2_scalar-rows%8=r",
                  "l1_scalar-l2_scalar-rows%8=r", "l1_scalar-l2_scalar-rows%8=0"}, te
    assert {(c[0], c[1]) for c in TE_CASES} >= {(128, 512), (128, 256), (64, 256), (32, 128), (32, 100), (20, 52)}
    assert {(c[2], c[3]) for c in TE_CASES} == {(f, b) for f in (0, 1) for b in (1, 3, 8)}
    assert {TE_T[(c[4] + b) % 4] for c in TE_CASES if c[3] == 1 for b in (0,)} == set(TE_T)                          # every timestep also alone
    tp = {_tp_branch(B, K, R, a) for (B, K, R) in TP_CASES for a in (0, 1)}
    assert len(tp) == 2 * (2 + 2 * 2 * 2) and len(TP_CASES) == 45, tp
