"""Float64 sweep over the softmax-attention kernels' whole dispatch space.

Every forward and backward attention entry (`adm_attention`, `adm_attention_blocked`, `adm_cross_attention`,
`adm_attention_backward`, `adm_attention_backward_blocked`, `adm_cross_attention_backward`) against the same operation in
float64 torch on the CPU, over seeded random shapes plus pinned ones on both sides of every dispatch rule, with inputs that
go from a diffuse to a one-hot softmax ("sharpness": q and k each scaled by sqrt(sharpness), so the logits' standard
deviation is the sharpness), key orders that are the worst case of the online softmax, and logits hundreds away from zero.
`adm_last_attention_variant()` (family * 100 + head_dim) must report the kernel family the rules give, recomputed here.

Bars. Two figures per compared tensor, both against float64: g = max|d| / max|ref| over the tensor, and (forward outputs
only) h = the same ratio per (sample, head), maximised. Each is bounded by the float32 torch reference's OWN error on the same
inputs times a margin: e_kernel <= M(T) * max(e_torch_fp32, 4u), u = 2^-24, M(T) = max(8, sqrt(T / log2 T)) (T = S for
cross-attention). The kernels add T terms serially where torch adds them pairwise / vectorised, which for independent roundings
costs about sqrt(T / log2 T); the floor of 8 covers the spread between the maxima of two rounding-noise samples and the
hardware exponential on x * log2(e); 4u keeps the bound from collapsing where torch is exact. At sharpness 1 and T <= 1024
the bars the suite already uses stay as ceilings (forward g <= 5e-6, backward g <= 2e-5). A kernel that drops a key,
mis-scales a block or combines maxima wrongly is off by >= 1e-3. Measured ratios: profiles/attention_accuracy.md.

The one-slab backward kernel's LDS rule is 4 * (4 T d + 3 T) <= 64 KiB, which (d16, T256) and (d32, T128) exceed by the 3 T
floats of softmax statistics: there `adm_attention_backward` returns its LDS error and the blocked kernel is the one that runs
(pinned below as such, with (d16, T244 | T245) and (d32, T125 | T126), the two sides of the rule at those head dimensions).
"""
import math
import random

import pytest
import torch

from native_backend import BACKENDS, select

U = 2.0 ** -24
ONE_PASS, SPLIT4, BLOCKED, MFMA, CROSS, BWD, BWD_BLOCKED, CROSS_BWD = 1, 2, 3, 4, 5, 6, 7, 8
FAMILY = {ONE_PASS: "one_pass", SPLIT4: "split4", BLOCKED: "blocked", MFMA: "mfma", CROSS: "cross", BWD: "bwd_one_slab",
          BWD_BLOCKED: "bwd_blocked", CROSS_BWD: "cross_bwd"}
HEAD_DIMS = [4, 8, 16, 32, 64]
PLANES = [(2, 2), (4, 4), (5, 7), (8, 8), (10, 10), (8, 16), (16, 16), (16, 20), (24, 24), (16, 32), (32, 32), (33, 32)]
SHARPNESS = [1, 4, 16, 64]
LDS = 64 * 1024


# ---------------------------------------------------------------- figures and bars
def _margin(T):
    return max(8.0, math.sqrt(T / math.log2(T))) if T > 2 else 8.0


def _g(a, ref):
    return float((a.double() - ref).abs().max() / (ref.abs().max() + 1e-300))


def _h(a, ref, slabs):
    """max|d| / max|ref| per (sample, head) slab, maximised: a head whose output is small is not hidden by a loud one."""
    d = (a.double() - ref).reshape(slabs, -1).abs().amax(1)
    return float((d / (ref.reshape(slabs, -1).abs().amax(1) + 1e-300)).max())


def _judge(what, got, ref64, ref32, T, tag, slabs=0, ceiling=None):
    """got (kernel, fp32) against ref64 under M(T) * max(error of ref32, 4u); figures are printed before they are asserted."""
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all()), (what, tag, "kernel output is not finite")
    assert bool(torch.isfinite(ref32).all()) and bool(torch.isfinite(ref64).all()), (what, tag, "reference is not finite")
    figures = [("g", _g(got, ref64), _g(ref32, ref64))]
    if slabs:
        figures.append(("h", _h(got, ref64, slabs), _h(ref32, ref64, slabs)))
    for name, e_kernel, e_torch in figures:
        floor = max(e_torch, 4 * U)
        bound = _margin(T) * floor
        print(f"ATTN_SWEEP {tag} {what} {name} e_kernel={e_kernel:.3e} e_torch_fp32={e_torch:.3e} ratio={e_kernel / floor:.2f} "
              f"bound={_margin(T):.2f}")
        assert e_kernel <= bound, (what, tag, name, e_kernel, e_torch, bound)
        if ceiling is not None and name == "g":
            assert e_kernel <= ceiling, (what, tag, e_kernel, ceiling)


def _tag(backend, family, d, T, sharp):
    return f"backend={backend} family={FAMILY[family]} d={d} T={T} sharpness={sharp}"


# ---------------------------------------------------------------- references (float64 to judge by, float32 to size the bound)
def _ref_attention(qkv, d, dtype):
    Nn, C3, H, W = qkv.shape
    C, T = C3 // 3, H * W
    q, k, v = qkv.to(dtype).reshape(Nn, 3, C // d, d, T).unbind(1)            # (N, heads, d, T)
    s = torch.einsum("nhdt,nhdj->nhtj", q, k) * d ** -0.5
    return torch.einsum("nhtj,nhdj->nhdt", s.softmax(-1), v).reshape(Nn, C, H, W)


def _ref_attention_backward(qkv, dout, d, dtype):
    x = qkv.to(dtype).clone().requires_grad_(True)
    _ref_attention(x, d, dtype).backward(dout.to(dtype))
    return x.grad


def _ref_cross(q, ctx, wk, wv, d, dtype):
    q, ctx, wk, wv = (t.to(dtype) for t in (q, ctx, wk, wv))
    Nn, C, H, W = q.shape
    k = (ctx @ wk.T).reshape(Nn, -1, C // d, d)                               # (N, S, heads, d)
    v = (ctx @ wv.T).reshape(Nn, -1, C // d, d)
    s = torch.einsum("nhdt,nshd->nhts", q.reshape(Nn, C // d, d, H * W), k) * d ** -0.5
    return torch.einsum("nhts,nshd->nhdt", s.softmax(-1), v).reshape(Nn, C, H, W)


def _randn(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _make_qkv(Nn, heads, d, plane, sharp, seed):
    qkv = _randn((Nn, 3, heads * d) + tuple(plane), seed)
    qkv[:, :2] *= math.sqrt(sharp)
    return qkv.reshape(Nn, 3 * heads * d, *plane).contiguous()


# ---------------------------------------------------------------- the dispatch rules, recomputed
def _mfma_rule(d, T):
    return d in (16, 32, 64) and T % 128 == 0 and T % (256 if d <= 32 else 128) == 0


def _forward_family(entry, d, T, aligned=True):
    """entry: "att" = adm_attention, "ss" = adm_attention under "single_sample" = 1, "blk" = adm_attention_blocked."""
    if entry == "blk":
        return BLOCKED
    if _mfma_rule(d, T) and aligned:
        return MFMA
    if 2 * T * d * 4 > LDS:
        return BLOCKED
    if entry == "ss" and T >= 64 and T % 4 == 0 and d in (4, 8, 16):
        return SPLIT4
    return ONE_PASS


def _bwd_one_slab_fits(d, T):
    return d <= 32 and 4 * (4 * T * d + 3 * T) <= LDS


def _variant(lib):
    return int(lib.adm_last_attention_variant())


# ---------------------------------------------------------------- (a) + (b) forward sweep
def _forward_cases(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        d, heads, Nn = rng.choice(HEAD_DIMS), rng.randint(1, 3), rng.randint(1, 3)
        plane = rng.choice(PLANES)
        entry = rng.choice(["att", "att", "ss", "ss", "blk"])
        kb = rng.choice([0, 16, 24, 100]) if entry == "blk" else 0
        sharp = rng.choice(SHARPNESS)
        if plane[0] * plane[1] * d > 64 * 1024:
            continue
        out.append((Nn, heads, d, plane, entry, kb, sharp))
    return out


PINNED_FORWARD = [
    (2, 2, 8, (32, 32), "att", 0, 4), (2, 2, 8, (33, 32), "att", 0, 4),        # the two sides of the 64 KiB one-pass limit
    (1, 1, 16, (64, 64), "att", 0, 4), (2, 2, 32, (32, 32), "att", 0, 16),     # the conditional UNet's shapes: several key blocks on the MFMA kernel
    (2, 2, 64, (16, 16), "att", 0, 4), (1, 2, 64, (16, 32), "att", 0, 1),
    (2, 2, 8, (16, 20), "att", 0, 1), (2, 2, 8, (24, 24), "att", 0, 16),       # several query workgroups, the last ragged
    (2, 2, 16, (8, 24), "ss", 0, 4), (3, 1, 16, (8, 8), "ss", 0, 16),          # split4<16>: only where the shape is not MFMA-eligible
    (2, 2, 4, (10, 10), "ss", 0, 64), (2, 3, 4, (16, 16), "ss", 0, 1),
    (2, 1, 16, (16, 32), "att", 0, 1), (2, 1, 32, (16, 32), "att", 0, 64),     # MFMA d16 / d32 at two key blocks
    (2, 1, 32, (2, 2), "att", 0, 4), (1, 2, 64, (8, 8), "att", 0, 16),         # attention_kernel<32 / 64>
]
FORWARD = _forward_cases(80, seed=20261016) + PINNED_FORWARD


def _fid(c):
    Nn, heads, d, plane, entry, kb, sharp = c
    return f"N{Nn}-h{heads}-d{d}-{plane[0]}x{plane[1]}-{entry}{kb if entry == 'blk' else ''}-s{sharp}"


def _run_forward(ops, lib, entry, qkv, d, kb):
    """-> (output, variant reported); the "single_sample" option is put back whatever happens."""
    from audiodiffusion import _native
    if entry == "blk":
        out = ops.attention_blocked(qkv, d, kb)
        return out, _variant(lib)
    if entry == "ss":
        _native.check(lib.adm_set_option(b"single_sample", 1))
    try:
        out = ops.attention(qkv, d)
        return out, _variant(lib)
    finally:
        if entry == "ss":
            _native.check(lib.adm_set_option(b"single_sample", -1))


def _check_forward(backend, dev, qkv, d, entry, kb, sharp, family=None):
    from audiodiffusion import _native, ops
    lib = _native.lib()
    Nn, C3, H, W = qkv.shape
    C, T = C3 // 3, H * W
    x = qkv.to(dev)
    aligned = x.data_ptr() % 16 == 0
    assert bool(lib.adm_attention_mfma_eligible(C, T, d)) == _mfma_rule(d, T), (C, T, d)
    want = _forward_family(entry, d, T, aligned) if family is None else family
    out, variant = _run_forward(ops, lib, entry, x, d, kb)
    assert variant == want * 100 + d, (variant, FAMILY[want], d, T)
    if entry != "blk":                      # MFMA exactly when the library's own rule says so (and the pointer allows the 16-byte loads)
        assert (variant // 100 == MFMA) == (bool(lib.adm_attention_mfma_eligible(C, T, d)) and aligned)
    ceiling = 5e-6 if sharp == 1 and T <= 1024 else None
    host = qkv.cpu()
    _judge("out", out, _ref_attention(host, d, torch.float64), _ref_attention(host, d, torch.float32), T,
           _tag(backend, want, d, T, sharp), slabs=Nn * (C // d), ceiling=ceiling)
    if Nn > 1:                              # a sample's bits do not depend on the batch it is in
        alone, v1 = _run_forward(ops, lib, entry, x[Nn - 1:].contiguous(), d, kb)
        assert v1 == variant and torch.equal(alone.cpu(), out[Nn - 1:].cpu()), (FAMILY[want], d, T)
    return out


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", FORWARD, ids=[_fid(c) for c in FORWARD])
def test_forward_sweep(backend, case):
    dev = select(backend)
    Nn, heads, d, plane, entry, kb, sharp = case
    qkv = _make_qkv(Nn, heads, d, plane, sharp, seed=1000 + FORWARD.index(case))
    _check_forward(backend, dev, qkv, d, entry, kb, sharp)


def test_forward_sweep_reaches_every_kernel():
    """Every family x head-dimension pair the rules can reach occurs at least twice in the list above (each case asserts that the launch
    report equals the variant counted here), and the MFMA kernel runs with >= 2 key blocks at each of its head dimensions."""
    seen = {}
    blocks = {16: 0, 32: 0, 64: 0}
    for Nn, heads, d, plane, entry, kb, sharp in FORWARD:
        T = plane[0] * plane[1]
        fam = _forward_family(entry, d, T)
        seen[fam * 100 + d] = seen.get(fam * 100 + d, 0) + 1
        if fam == MFMA:
            blocks[d] = max(blocks[d], T // (256 if d <= 32 else 128))
    reachable = ([ONE_PASS * 100 + d for d in HEAD_DIMS] + [SPLIT4 * 100 + d for d in (4, 8, 16)]
                 + [BLOCKED * 100 + d for d in HEAD_DIMS] + [MFMA * 100 + d for d in (16, 32, 64)])
    assert len(reachable) == 16 and len(FORWARD) >= 80 + len(PINNED_FORWARD)
    assert {v: seen.get(v, 0) for v in reachable if seen.get(v, 0) < 2} == {}, seen
    assert set(seen) <= set(reachable), seen
    assert all(b >= 2 for b in blocks.values()), blocks
    for c in PINNED_FORWARD[:12]:           # the pinned shapes sit where they were put
        assert c in FORWARD
    fam = lambda i: _forward_family(PINNED_FORWARD[i][4], PINNED_FORWARD[i][2], PINNED_FORWARD[i][3][0] * PINNED_FORWARD[i][3][1])  # noqa: E731
    assert [fam(i) for i in range(12)] == [ONE_PASS, BLOCKED, MFMA, MFMA, MFMA, MFMA, ONE_PASS, ONE_PASS, SPLIT4, SPLIT4, SPLIT4, SPLIT4]


# ---------------------------------------------------------------- (c) adversarial key orders for the online softmax
def _reorder_keys(qkv, d, mode):
    """Per (sample, head): k and v permuted together so that query 0's logits rise ("inc") or fall ("dec") strictly along the key axis,
    or ("spike") the last key scaled so that its logit for query 0 is 60 above every other."""
    Nn, C3, H, W = qkv.shape
    C, T = C3 // 3, H * W
    x = qkv.reshape(Nn, 3, C // d, d, T).clone()
    for n in range(Nn):
        for h in range(C // d):
            q0 = x[n, 0, h, :, 0].double()
            s = (q0 @ x[n, 1, h].double()) * d ** -0.5                         # (T,)
            if mode == "spike":
                a = float((s[:-1].max() + 60.0) / s[-1])
                assert abs(a) < 40, a                                          # (the seeds below keep the factor ordinary)
                x[n, 1, h, :, -1] *= a
                s = (q0 @ x[n, 1, h].double()) * d ** -0.5
                assert float(s[-1] - s[:-1].max()) > 59.9
            else:
                order = torch.argsort(s, descending=(mode == "dec"))
                x[n, 1, h] = x[n, 1, h][:, order]
                x[n, 2, h] = x[n, 2, h][:, order]
                s = (q0 @ x[n, 1, h].double()) * d ** -0.5
                step = s[1:] - s[:-1]
                assert bool((step > 0).all() if mode == "inc" else (step < 0).all())
    return x.reshape(Nn, C3, H, W).contiguous()


ORDER_FORWARD = [(8, (10, 10), "blk", 16), (32, (10, 10), "blk", 24), (4, (16, 20), "blk", 24), (64, (5, 7), "blk", 16),
                 (16, (24, 32), "att", 0), (32, (24, 32), "att", 0), (64, (16, 24), "att", 0)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["inc", "dec", "spike"])
@pytest.mark.parametrize("d,plane,entry,kb", ORDER_FORWARD, ids=[f"d{c[0]}-T{c[1][0] * c[1][1]}-{c[2]}{c[3]}" for c in ORDER_FORWARD])
def test_forward_adversarial_key_orders(backend, d, plane, entry, kb, mode):
    """The running maximum rises in every key block (the worst case of the exp(m_old - m_new) correction), never after the first, or jumps by
    60 on the very last key (of a ragged last block where the kernel has one)."""
    dev = select(backend)
    T = plane[0] * plane[1]
    qkv = _reorder_keys(_make_qkv(2, 2, d, plane, 16, seed=102 + d), d, mode)
    want = MFMA if entry == "att" else BLOCKED
    if want == MFMA:
        assert T // (256 if d <= 32 else 128) >= 3
    _check_forward(backend, dev, qkv, d, entry, kb, 16, family=want)


# ---------------------------------------------------------------- (d) logits far from zero
def _shifted_qkv(Nn, heads, d, plane, seed):
    """q and k scaled by 2, then every key of head h moved by c_h = 50 sqrt(d) r_h / |r_h|: query t's logits all move by q_t . c_h d^-0.5,
    a per-query shift with a standard deviation of about 100 (row maxima from about -350 to +340)."""
    T = plane[0] * plane[1]
    x = _make_qkv(Nn, heads, d, plane, 4, seed).reshape(Nn, 3, heads, d, T)
    r = _randn((heads, d), seed + 1).double()
    c = (50.0 * math.sqrt(d) * r / r.norm(dim=1, keepdim=True)).float()
    x[:, 1] += c[None, :, :, None]
    q, k = x[:, 0].double(), x[:, 1].double()
    rowmax = (torch.einsum("nhdt,nhdj->nhtj", q, k) * d ** -0.5).amax(-1)
    assert int((rowmax < -100).sum()) >= 8 and int((rowmax > 100).sum()) >= 8, (float(rowmax.min()), float(rowmax.max()))
    return x.reshape(Nn, 3 * heads * d, *plane).contiguous()


SHIFT_FORWARD = [(4, (10, 10), "att", 0, ONE_PASS), (8, (8, 8), "att", 0, ONE_PASS), (64, (8, 8), "att", 0, ONE_PASS),
                 (4, (10, 10), "ss", 0, SPLIT4), (8, (8, 8), "ss", 0, SPLIT4), (16, (8, 8), "ss", 0, SPLIT4),
                 (8, (10, 10), "blk", 24, BLOCKED), (32, (16, 20), "blk", 24, BLOCKED),
                 (16, (16, 16), "att", 0, MFMA), (32, (32, 32), "att", 0, MFMA), (64, (16, 16), "att", 0, MFMA)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("d,plane,entry,kb,family", SHIFT_FORWARD,
                         ids=[f"{FAMILY[c[4]]}-d{c[0]}-T{c[1][0] * c[1][1]}" for c in SHIFT_FORWARD])
def test_forward_logits_far_from_zero(backend, d, plane, entry, kb, family):
    """Fails when a row maximum is initialised above the data, dropped, or combined wrongly across the four lanes of split4 or across key
    blocks (inf / inf or 0 / 0): every output finite and inside the bars, with row maxima below -100 and above +100."""
    dev = select(backend)
    T = plane[0] * plane[1]
    assert _forward_family(entry, d, T) == family
    _check_forward(backend, dev, _shifted_qkv(2, 2, d, plane, seed=500 + d + T), d, entry, kb, "shift", family=family)


# ---------------------------------------------------------------- (e) the alignment fallback
@pytest.mark.parametrize("backend", BACKENDS)
def test_forward_alignment_fallback(backend):
    """An MFMA-eligible shape whose pointer is 4 bytes off a 16-byte boundary takes a vector-ALU kernel (the MFMA kernel stages K and V with
    16-byte loads): reported as such, inside the bars, and equal to the aligned MFMA result and to the blocked kernel's up to those bars."""
    dev = select(backend)
    from audiodiffusion import _native, ops
    lib = _native.lib()
    Nn, heads, d, plane = 2, 2, 16, (16, 16)
    T, C = 256, heads * d
    qkv = _make_qkv(Nn, heads, d, plane, 4, seed=31)
    flat = torch.empty(qkv.numel() + 8, dtype=torch.float32, device=dev)
    off = next(o for o in range(1, 8) if (flat.data_ptr() + 4 * o) % 16 == 4)
    view = flat[off:off + qkv.numel()].view(qkv.shape)
    view.copy_(qkv)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous() and lib.adm_attention_mfma_eligible(C, T, d) == 1
    off_out = _check_forward(backend, dev, view, d, "att", 0, 4)              # the rules recomputed with aligned = False: one pass
    assert _variant(lib) == ONE_PASS * 100 + d
    aligned = ops.attention(qkv.to(dev), d)
    assert _variant(lib) == MFMA * 100 + d
    blocked = ops.attention_blocked(qkv.to(dev), d, 0)
    ref64, ref32 = _ref_attention(qkv, d, torch.float64), _ref_attention(qkv, d, torch.float32)
    bound = _margin(T) * max(_g(ref32, ref64), 4 * U)
    for name, other in (("mfma", aligned), ("blocked", blocked)):
        _judge("out", other, ref64, ref32, T, _tag(backend, MFMA if name == "mfma" else BLOCKED, d, T, 4), slabs=Nn * heads)
        assert _g(off_out.cpu(), other.cpu().double()) <= 2 * bound, name      # two results inside the bar are within twice the bar of each other


# ---------------------------------------------------------------- (f) cross-attention, forward and backward
def _cross_cases(n, seed):
    rng = random.Random(seed)
    out = [(d, S, rng.choice([12, 33]), rng.choice([(4, 8), (10, 10), (16, 20)]), rng.choice(SHARPNESS))
           for d in HEAD_DIMS for S in (1, 2, 7, 77)]                          # every head dimension at every sequence length
    while len(out) < n:
        out.append((rng.choice(HEAD_DIMS), rng.choice([1, 2, 7, 77]), rng.choice([12, 33]), rng.choice([(4, 8), (10, 10), (16, 20)]),
                    rng.choice(SHARPNESS)))
    return out


CROSS_CASES = _cross_cases(32, seed=5)


def _cross_inputs(Nn, heads, d, S, Dc, plane, sharp, seed):
    C = heads * d
    q = _randn((Nn, C) + tuple(plane), seed) * math.sqrt(sharp)
    ctx = _randn((Nn, S, Dc), seed + 1)
    wk = _randn((C, Dc), seed + 2) * (Dc ** -0.5 * math.sqrt(sharp))
    wv = _randn((C, Dc), seed + 3) * Dc ** -0.5
    return q, ctx, wk, wv, _randn((Nn, C) + tuple(plane), seed + 4)


def _cross_refs(q, ctx, wk, wv, dy, d, dtype):
    q, wk, wv = (t.to(dtype).clone().requires_grad_(True) for t in (q, wk, wv))
    out = _ref_cross(q, ctx, wk, wv, d, dtype)
    out.backward(dy.to(dtype))
    return out.detach(), q.grad, wk.grad, wv.grad


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("d,S,Dc,plane,sharp", CROSS_CASES,
                         ids=[f"{i}-d{c[0]}-S{c[1]}-Dc{c[2]}-T{c[3][0] * c[3][1]}-s{c[4]}" for i, c in enumerate(CROSS_CASES)])
def test_cross_attention_sweep(backend, d, S, Dc, plane, sharp):
    dev = select(backend)
    from audiodiffusion import _native, ops
    lib = _native.lib()
    Nn, heads = 2, 2
    T = plane[0] * plane[1]
    q, ctx, wk, wv, dy = _cross_inputs(Nn, heads, d, S, Dc, plane, sharp, seed=900 + 7 * d + S)
    on_dev = lambda *ts: [t.to(dev) for t in ts]  # noqa: E731
    out = ops.cross_attention(*on_dev(q, ctx, wk, wv), d)
    assert _variant(lib) == CROSS * 100 + d
    r64, r32 = _cross_refs(q, ctx, wk, wv, dy, d, torch.float64), _cross_refs(q, ctx, wk, wv, dy, d, torch.float32)
    easy = sharp == 1
    _judge("out", out, r64[0], r32[0], S, _tag(backend, CROSS, d, S, sharp), slabs=Nn * heads, ceiling=5e-6 if easy else None)
    if 4 * S * d * 4 > LDS:                  # the backward keeps dK and dV of the head in LDS too (d64, S77): its own loud error, nothing launched
        with pytest.raises(RuntimeError, match="LDS K/V slab"):
            ops.cross_attention_backward(*on_dev(q, ctx, wk, wv, dy), d)
        assert (d, S) == (64, 77) and _variant(lib) == CROSS * 100 + d
        return
    dq, dwk, dwv = ops.cross_attention_backward(*on_dev(q, ctx, wk, wv, dy), d)
    assert _variant(lib) == CROSS_BWD * 100 + d
    tag = _tag(backend, CROSS_BWD, d, S, sharp)
    _judge("dWv", dwv, r64[3], r32[3], S, tag, ceiling=2e-5 if easy else None)
    if S == 1:       # one key: the softmax is 1, every token receives V, and q and to_k have no gradient
        v = (ctx @ wv.T).transpose(1, 2).reshape(Nn, heads * d, 1, 1).expand_as(q)
        assert _g(out.cpu(), v.double()) < 2e-6
        assert float(dq.abs().max()) == 0 and float(dwk.abs().max()) < 1e-6 * float(r64[3].abs().max())
    else:
        _judge("dq", dq, r64[1], r32[1], S, tag, ceiling=2e-5 if easy else None)
        _judge("dWk", dwk, r64[2], r32[2], S, tag, ceiling=2e-5 if easy else None)


@pytest.mark.parametrize("backend", BACKENDS)
def test_cross_attention_lds_slab_limits(backend):
    """Forward: 2 S d 4 <= 64 KiB (d64: S128 runs, S129 is an error return with nothing launched); the backward keeps dK and dV in LDS as
    well, 4 S d 4 <= 64 KiB (d64: S64 runs, S65 is the error)."""
    dev = select(backend)
    from audiodiffusion import _native, ops
    lib = _native.lib()
    d, Nn, heads, Dc, plane = 64, 1, 2, 12, (4, 8)
    on_dev = lambda *ts: [t.to(dev) for t in ts]  # noqa: E731
    for S, fwd_fits, bwd_fits in ((64, True, True), (65, True, False), (128, True, False), (129, False, False)):
        q, ctx, wk, wv, dy = _cross_inputs(Nn, heads, d, S, Dc, plane, 4, seed=40 + S)
        assert fwd_fits == (2 * S * d * 4 <= LDS) and bwd_fits == (4 * S * d * 4 <= LDS)
        ops.attention(_make_qkv(1, 1, 4, (2, 2), 1, 1).to(dev), 4)             # a launch of another family: the report below is this call's
        r64, r32 = _cross_refs(q, ctx, wk, wv, dy, d, torch.float64), _cross_refs(q, ctx, wk, wv, dy, d, torch.float32)
        if fwd_fits:
            out = ops.cross_attention(*on_dev(q, ctx, wk, wv), d)
            assert _variant(lib) == CROSS * 100 + d
            _judge("out", out, r64[0], r32[0], S, _tag(backend, CROSS, d, S, 4), slabs=Nn * heads)
        else:
            with pytest.raises(RuntimeError, match="LDS K/V slab"):
                ops.cross_attention(*on_dev(q, ctx, wk, wv), d)
            assert _variant(lib) == ONE_PASS * 100 + 4                         # nothing launched
        ops.attention(_make_qkv(1, 1, 4, (2, 2), 1, 1).to(dev), 4)
        if bwd_fits:
            dq, dwk, dwv = ops.cross_attention_backward(*on_dev(q, ctx, wk, wv, dy), d)
            assert _variant(lib) == CROSS_BWD * 100 + d
            for what, got, i in (("dq", dq, 1), ("dWk", dwk, 2), ("dWv", dwv, 3)):
                _judge(what, got, r64[i], r32[i], S, _tag(backend, CROSS_BWD, d, S, 4))
        else:
            with pytest.raises(RuntimeError, match="LDS K/V slab"):
                ops.cross_attention_backward(*on_dev(q, ctx, wk, wv, dy), d)
            assert _variant(lib) == ONE_PASS * 100 + 4


# ---------------------------------------------------------------- (g) backward sweep
def _backward_cases(n, seed):
    rng = random.Random(seed)
    out = []
    while len(out) < n:
        d, heads, Nn = rng.choice(HEAD_DIMS), rng.randint(1, 2), rng.randint(1, 2)
        plane = rng.choice(PLANES)
        if plane[0] * plane[1] * d > 64 * 1024:
            continue
        out.append((Nn, heads, d, plane, rng.choice([0, 16, 24]), rng.choice(SHARPNESS)))
    return out


PINNED_BACKWARD = [
    (1, 2, 8, (18, 26), 0, 4), (1, 2, 8, (7, 67), 0, 4),                       # d8: T468 is the last that fits the one-slab kernel, T469 does not
    (2, 2, 4, (10, 10), 16, 16), (1, 2, 16, (4, 61), 0, 4), (1, 2, 16, (5, 49), 24, 4), (1, 2, 32, (5, 25), 0, 1), (1, 2, 32, (6, 21), 16, 1),
    (1, 2, 16, (16, 16), 0, 4), (1, 2, 32, (8, 16), 0, 4),                     # 4 T d floats alone are 64 KiB here: the statistics no longer fit
    (1, 2, 64, (16, 16), 0, 4), (1, 1, 16, (32, 32), 0, 16),
]
BACKWARD = _backward_cases(40, seed=20261017) + PINNED_BACKWARD


def _bid(c):
    Nn, heads, d, plane, block, sharp = c
    return f"N{Nn}-h{heads}-d{d}-{plane[0]}x{plane[1]}-b{block}-s{sharp}"


def _check_backward(backend, dev, qkv, dout, d, block, sharp):
    from audiodiffusion import _native, ops
    lib = _native.lib()
    Nn, C3, H, W = qkv.shape
    C, T = C3 // 3, H * W
    r64 = _ref_attention_backward(qkv, dout, d, torch.float64).reshape(Nn, 3, C, T)
    r32 = _ref_attention_backward(qkv, dout, d, torch.float32).reshape(Nn, 3, C, T)
    ceiling = 2e-5 if sharp == 1 and T <= 1024 else None
    x, g = qkv.to(dev), dout.to(dev)

    def judge(got, family):                 # dq, dk and dv separately: at high sharpness they differ in size by orders of magnitude
        got = got.cpu().reshape(Nn, 3, C, T)
        for i, what in enumerate(("dq", "dk", "dv")):
            _judge(what, got[:, i], r64[:, i], r32[:, i], T, _tag(backend, family, d, T, sharp), ceiling=ceiling)

    got = ops.attention_backward_blocked(x, g, d, block)
    assert _variant(lib) == BWD_BLOCKED * 100 + d
    judge(got, BWD_BLOCKED)
    if _bwd_one_slab_fits(d, T):
        got = ops.attention_backward(x, g, d)
        assert _variant(lib) == BWD * 100 + d
        judge(got, BWD)
    elif d <= 32:                           # a loud error, nothing launched: the report is still the blocked launch above
        with pytest.raises(RuntimeError, match="64 KiB of LDS"):
            ops.attention_backward(x, g, d)
        assert _variant(lib) == BWD_BLOCKED * 100 + d
    return _bwd_one_slab_fits(d, T)


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("case", BACKWARD, ids=[_bid(c) for c in BACKWARD])
def test_backward_sweep(backend, case):
    dev = select(backend)
    Nn, heads, d, plane, block, sharp = case
    seed = 3000 + BACKWARD.index(case)
    qkv, dout = _make_qkv(Nn, heads, d, plane, sharp, seed), _randn((Nn, heads * d) + tuple(plane), seed + 500)
    _check_backward(backend, dev, qkv, dout, d, block, sharp)


def test_backward_sweep_reaches_both_kernels_at_every_head_dimension():
    one_slab, blocked = {}, {}
    for Nn, heads, d, plane, block, sharp in BACKWARD:
        blocked[d] = blocked.get(d, 0) + 1
        if _bwd_one_slab_fits(d, plane[0] * plane[1]):
            one_slab[d] = one_slab.get(d, 0) + 1
    assert len(BACKWARD) >= 40 + len(PINNED_BACKWARD)
    assert all(blocked.get(d, 0) >= 2 for d in HEAD_DIMS) and all(one_slab.get(d, 0) >= 2 for d in (4, 8, 16, 32)), (one_slab, blocked)
    fits = [_bwd_one_slab_fits(c[2], c[3][0] * c[3][1]) for c in PINNED_BACKWARD]
    assert fits == [True, False, True, True, False, True, False, False, False, False, False]
    assert [c[3][0] * c[3][1] for c in PINNED_BACKWARD[:2]] == [468, 469]


ORDER_BACKWARD = [(8, (10, 10), 16), (32, (10, 10), 24), (64, (5, 7), 16), (4, (16, 20), 24)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("mode", ["inc", "dec", "spike"])
@pytest.mark.parametrize("d,plane,block", ORDER_BACKWARD, ids=[f"d{c[0]}-T{c[1][0] * c[1][1]}-b{c[2]}" for c in ORDER_BACKWARD])
def test_backward_adversarial_key_orders(backend, d, plane, block, mode):
    dev = select(backend)
    qkv = _reorder_keys(_make_qkv(2, 2, d, plane, 16, seed=177 + d), d, mode)
    _check_backward(backend, dev, qkv, _randn((2, 2 * d) + tuple(plane), 178 + d), d, block, 16)


SHIFT_BACKWARD = [(8, (8, 8), 0, True), (16, (10, 10), 24, True), (4, (10, 10), 16, True), (64, (8, 8), 24, False), (8, (16, 32), 0, False)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("d,plane,block,one_slab", SHIFT_BACKWARD, ids=[f"d{c[0]}-T{c[1][0] * c[1][1]}-b{c[2]}" for c in SHIFT_BACKWARD])
def test_backward_logits_far_from_zero(backend, d, plane, block, one_slab):
    dev = select(backend)
    T = plane[0] * plane[1]
    qkv = _shifted_qkv(2, 2, d, plane, seed=700 + d + T)
    assert _check_backward(backend, dev, qkv, _randn((2, 2 * d) + tuple(plane), 701 + d), d, block, "shift") == one_slab


# ---------------------------------------------------------------- (h) the executor takes the same turns
TRAIN_CFGS = {
    "T256-one-slab": (dict(sample_size=16, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
                           down_block_types=("AttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "AttnUpBlock2D")), 256),
    "T1024-blocked": (dict(sample_size=32, in_channels=1, out_channels=1, layers_per_block=1, block_out_channels=(32, 32),
                           down_block_types=("AttnDownBlock2D", "DownBlock2D"), up_block_types=("UpBlock2D", "AttnUpBlock2D")), 1024),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(TRAIN_CFGS))
def test_training_executor_picks_the_backward_kernel_by_the_same_rule(backend, name):
    """The attention level of the first down block is the last attention the backward pass reaches: after a training step the launch report
    is the one-slab kernel where the head (d = 8) fits 64 KiB of LDS and the blocked one where it does not (32x32 tokens)."""
    dev = select(backend)
    from audiodiffusion import _native, ops
    from audiodiffusion.unet import UNet2DModel
    from oracle.unet import UNet2DModel as OracleUNet
    cfg, T = TRAIN_CFGS[name]
    torch.manual_seed(0)
    mine = UNet2DModel(**cfg).load_state_dict(OracleUNet(**cfg).state_dict())
    d = cfg.get("attention_head_dim", 8)
    mine.enable_training()
    ss = cfg["sample_size"]
    x, tgt = _randn((1, 1, ss, ss), 1), _randn((1, 1, ss, ss), 2)
    ops.attention_blocked(_make_qkv(1, 1, 4, (2, 2), 1, 1).to(dev), 4)         # another family: the report below is the training step's
    assert _variant(_native.lib()) == BLOCKED * 100 + 4
    loss = mine.train_step(x.to(dev), torch.tensor([500]), tgt.to(dev))
    assert math.isfinite(float(loss))
    want = BWD if _bwd_one_slab_fits(d, T) else BWD_BLOCKED
    assert (want == BWD) == (T == 256)
    assert _variant(_native.lib()) == want * 100 + d, (_variant(_native.lib()), FAMILY[want], d)
