"""The side-stream overlap of the inference executor (`Net::plan_side_overlap` / `Net::run`, net_exec.hip; option "side_overlap").

A plain 1x1 convolution whose inputs are ready a few ops early (the resnets' conv_shortcut) is launched on a second HIP stream in front of
op hoist_from[j] and joined at its own position j. On the GPU the ops of the window [hoist_from[j], j) run CONCURRENTLY with it, so none
of them may (a) read bytes j writes, (b) write bytes j writes or (c) write bytes j reads. The emulator runs j in line at its hoisted
position: (a) and (b) corrupt its results, which the parity tests notice, but (c) does not show there (j has read its input before the
window op overwrites it). So the plans themselves are checked here, from the executor's own report of what every op reads and writes
(`adm_unet_plan_ops` / `adm_vae_plan_ops`: tensor ids and device byte ranges, derived from the launch arguments), on the emulator and on
the device; and with the option switched in-process, results with and without the side stream are compared bit for bit.
"""
import contextlib
import ctypes as C
import os
import re
from collections import namedtuple

import pytest
import torch

import test_unet as tu
import test_unet_condition as tc
import test_vae as tv
from native_backend import BACKENDS, select

CONV = 1   # adm_plan_op.kind


def _N():
    from audiodiffusion import _native
    return _native


def set_overlap(v):
    import audiodiffusion
    audiodiffusion.set_option("side_overlap", v)


@contextlib.contextmanager
def overlap(v):
    """The process-wide option at v for the block; back to -1 (the environment's default) whatever happens."""
    try:
        set_overlap(v)
        yield
    finally:
        set_overlap(-1)


def env_default():
    """What "side_overlap" = -1 means in this process: ADM_SIDE_OVERLAP (read with atoi), unset = on."""
    e = os.environ.get("ADM_SIDE_OVERLAP")
    if e is None:
        return True
    m = re.match(r"\s*([+-]?\d+)", e)
    return m is not None and int(m.group(1)) != 0


# ----------------------------------------------------------------------------------------------------------------- the report
# kind, hoist (= hoist_from), convolution shape / flags, tensor ids read / written, byte ranges [lo, hi) read / written
Op = namedtuple("Op", "kind hoist ks stride up flags tr tw rr rw")


def _records(fn, *args):
    N = _N()
    cap = 512
    while True:
        recs, n = (N.PlanOp * cap)(), C.c_int(0)
        N.check(fn(*args, recs, cap, C.byref(n)))
        if n.value <= cap:
            break
        cap = n.value
    return [Op(r.kind, r.hoist_from, r.ks, r.stride, r.up, r.flags, frozenset(r.tread[:r.n_tread]), frozenset(r.twrite[:r.n_twrite]),
               tuple((q.lo, q.hi) for q in r.read[:r.n_read]), tuple((q.lo, q.hi) for q in r.write[:r.n_write]))
            for r in recs[:n.value]]


def unet_plan(model, B):
    return _records(_N().lib().adm_unet_plan_ops, model._ensure_handle(), B)


def vae_plan(vae, which, B):
    return _records(_N().lib().adm_vae_plan_ops, vae._ensure_handle(vae._hw()), which, B)


def hoisted(plan):
    return [j for j, op in enumerate(plan) if op.hoist >= 0]


# ----------------------------------------------------------------------------------------------------------------- the checker
def _meet(a, b):
    return any(lo1 < hi2 and lo2 < hi1 for lo1, hi1 in a for lo2, hi2 in b)


def hazards(plan):
    """Every way a side launch of `plan` could race the ops it runs beside; [] = none. For each j with hoist_from[j] = i >= 0: j is a plain
    1x1 stride-1 convolution (no GroupNorm or activation on its load path, no statistics epilogue, no GroupNorm offered to its finish pass,
    weights of its own); every tensor it reads was last written before i (or is the network input, which no op writes); no op k in [i, j)
    reads what j writes (a), writes what j writes (b) or writes what j reads (c) — by byte range and by tensor id (the network input and
    output appear by id only); and windows are disjoint (the fork / join events are shared: the next side launch comes after j has joined)."""
    N = _N()
    plain = N.PLAN_GN_LOAD | N.PLAN_ACT | N.PLAN_STATS | N.PLAN_PER_SAMPLE_W | N.PLAN_GN_FUSE
    found = []
    writers = {}
    for k, op in enumerate(plan):
        for t in op.tw:
            writers.setdefault(t, []).append(k)
    side = hoisted(plan)
    for j in side:
        op, i = plan[j], plan[j].hoist
        if not 0 <= i < j:
            found.append(f"op {j}: hoist point {i} is not in front of it")
            continue
        if op.kind != CONV or op.ks != 1 or op.stride != 1 or op.up or op.flags & plain:
            found.append(f"op {j}: not a plain 1x1 stride-1 convolution (kind {op.kind}, ks {op.ks}, stride {op.stride}, up {op.up}, "
                         f"flags {op.flags})")
        for t in sorted(op.tr):
            before = [k for k in writers.get(t, []) if k < j]
            if before and before[-1] >= i:
                found.append(f"op {j}: its input tensor {t} is produced by op {before[-1]}, at or after the hoist point {i}")
        for k in range(i, j):
            w = plan[k]
            if _meet(w.rr, op.rw) or w.tr & op.tw:
                found.append(f"(a) op {k} in the window [{i}, {j}) reads what op {j} writes")
            if _meet(w.rw, op.rw) or w.tw & op.tw:
                found.append(f"(b) op {k} in the window [{i}, {j}) writes what op {j} writes")
            if _meet(w.rw, op.rr) or w.tw & op.tr:
                found.append(f"(c) op {k} in the window [{i}, {j}) writes what op {j} reads")
    for j, j2 in zip(side, side[1:]):
        if plan[j2].hoist <= j:
            found.append(f"windows overlap: op {j2} is launched in front of op {plan[j2].hoist}, before op {j} has joined")
    return found


def check_plan(plan, what):
    """The invariants, plus what makes them mean something: the report is complete for every op, and something is hoisted."""
    for k, op in enumerate(plan):
        assert (op.tr or op.rr) and (op.tw or op.rw), (what, k, op)
        if op.kind == CONV:
            assert op.rr, (what, k, "a convolution reads its weights")
    bad = hazards(plan)
    assert not bad, (what, bad[:8])
    assert hoisted(plan), f"{what}: nothing is hoisted — the test would check nothing"


# ----------------------------------------------------------------------------------------------------------------- a. checker self-test
def _op(kind=CONV, hoist=-1, ks=3, flags=0, tr=(), tw=(), rr=(), rw=()):
    return Op(kind, hoist, ks, 1, 0, flags, frozenset(tr), frozenset(tw), tuple(rr), tuple(rw))


def _resnet(**repl):
    """A resnet as Net::resnet emits it, its conv_shortcut hoisted in front of norm1. Tensors: 1 = block input x [0, 100), 2 = h [100, 200),
    3 = shortcut output s [200, 300), 4 = block output [300, 400); GroupNorm scale / shift [1000, 1010) and [1010, 1020)."""
    ops = [
        _op(tr=[0], tw=[1], rr=[(900, 950)], rw=[(0, 100)]),                                   # 0 producer of x
        _op(kind=0, tr=[1], rr=[(0, 100)], rw=[(1000, 1010)]),                                 # 1 norm1
        _op(flags=1 | 2, tr=[1], tw=[2], rr=[(0, 100), (1000, 1010), (2000, 2100)], rw=[(100, 200)]),   # 2 conv1
        _op(kind=0, tr=[2], rr=[(100, 200)], rw=[(1010, 1020)]),                               # 3 norm2
        _op(hoist=1, ks=1, tr=[1], tw=[3], rr=[(0, 100), (2100, 2110)], rw=[(200, 300)]),     # 4 conv_shortcut
        _op(flags=1 | 2, tr=[2, 3], tw=[4], rr=[(100, 200), (200, 300), (1010, 1020)], rw=[(300, 400)]),   # 5 conv2 (+ residual s)
    ]
    for k, kw in repl.items():
        ops[int(k[1:])] = ops[int(k[1:])]._replace(**kw)
    return ops


def test_the_checker_passes_a_clean_plan_and_flags_every_hazard():
    assert hazards(_resnet()) == []
    # (a) conv1 reads bytes the shortcut writes (an arena buffer handed to both)
    got = hazards(_resnet(o2=dict(rr=((0, 100), (1000, 1010), (250, 260)))))
    assert any(h.startswith("(a) op 2") for h in got), got
    # (b) conv1's output buffer is the shortcut's
    got = hazards(_resnet(o2=dict(rw=((150, 250),))))
    assert any(h.startswith("(b) op 2") for h in got), got
    # (c) norm2 overwrites the block input while the shortcut may still be reading it — the hazard the in-line emulator cannot see
    got = hazards(_resnet(o3=dict(rw=((1010, 1020), (40, 48)))))
    assert got and all(h.startswith("(c) op 3") for h in got), got
    # ... and by tensor id alone (the network input / output have no byte ranges in the report)
    got = hazards(_resnet(o3=dict(tw=frozenset([1]))))
    assert any(h.startswith("(c) op 3") for h in got), got
    # a producer of an input at or after the hoist point
    got = hazards(_resnet(o4=dict(hoist=0)))
    assert any("produced by op 0, at or after the hoist point 0" in h for h in got), got
    # overlapping windows: a second side launch forked before the first has joined
    plan = _resnet() + [_op(kind=0, tr=[4], rr=[(300, 400)], rw=[(1020, 1030)]),
                        _op(hoist=3, ks=1, tr=[1], tw=[5], rr=[(0, 100), (2200, 2210)], rw=[(500, 600)])]
    assert hazards(plan[:6] + [plan[6], plan[7]._replace(hoist=5)]) == []
    assert hazards(plan) == ["windows overlap: op 7 is launched in front of op 3, before op 4 has joined"]
    # not a plain 1x1 convolution: GroupNorm on the load path / statistics epilogue / a 3x3
    for repl in (dict(flags=1), dict(flags=4), dict(ks=3)):
        got = hazards(_resnet(o4=repl))
        assert any("not a plain 1x1" in h for h in got), (repl, got)
    # a hoist point that is not in front of the op
    assert any("not in front" in h for h in hazards(_resnet(o4=dict(hoist=4))))


# ----------------------------------------------------------------------------------------------------------------- models
def _unet(cfg, seed=0):
    from audiodiffusion import UNet2DModel
    return UNet2DModel(**cfg).init_random(seed)


def _cond(cfg, seed=0):
    from audiodiffusion import UNet2DConditionModel
    return UNet2DConditionModel(**cfg).init_random(seed)


def _vae(cfg, seed=0):
    from audiodiffusion.vae import AutoencoderKL
    return AutoencoderKL(**cfg).init_random(seed)


def _hw(cfg):
    ss = cfg["sample_size"]
    return (ss, ss) if isinstance(ss, int) else tuple(ss)


UNET_CFGS = dict(tiny=tu.TINY, tiny3=tu.TINY3, wide=tu.WIDE, small_planes=tu.SMALL_PLANES, one_pixel=tu.ONE_PIXEL, w6net=tu.W6NET)
VAE_CFGS = dict(smallhead=tv.TINY, gemmattn=tv.TINY_GEMM_ATTN)


# ----------------------------------------------------------------------------------------------------------------- b. plan invariants
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(UNET_CFGS))
def test_unet_plans_keep_the_window_ops_off_the_side_launch(backend, name):
    """The tiny UNet2DModel configs of tests/test_unet.py at B = 1, 2, 4: every side launch is a plain 1x1 convolution whose inputs were
    written before its hoist point, and nothing in its window touches what it reads or writes."""
    select(backend)
    m = _unet(UNET_CFGS[name])
    with overlap(1):
        for B in (1, 2, 4):
            check_plan(unet_plan(m, B), f"{name} B={B}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", ["tiny", "tiny3"])
def test_conditional_unet_plans_keep_the_window_ops_off_the_side_launch(backend, name):
    select(backend)
    m = _cond(dict(tiny=tc.TINY, tiny3=tc.TINY3)[name])
    with overlap(1):
        for B in (1, 2, 4):
            check_plan(unet_plan(m, B), f"conditional {name} B={B}")


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("name", list(VAE_CFGS))
def test_vae_plans_keep_the_window_ops_off_the_side_launch(backend, name):
    select(backend)
    v = _vae(VAE_CFGS[name])
    with overlap(1):
        for which in (0, 1):
            for B in (1, 2):
                check_plan(vae_plan(v, which, B), f"vae {name} {('encoder', 'decoder')[which]} B={B}")


# ----------------------------------------------------------------------------------------------------------------- c. the option
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_option_re_plans_every_net_by_itself(backend):
    """"side_overlap" = 0: the next report (same model, same batch, nothing else changed) comes from a new plan without side launches; 1 brings
    them back; -1 gives the environment's default (ADM_SIDE_OVERLAP, unset = on). A UNet's captured loop runs on the re-made plan (the plan
    the loop used is the one the report shows: a current plan is not re-made by the report), and the VAE re-plans the same way."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel
    dev = select(backend)
    m, v = _unet(tu.TINY), _vae(tv.TINY)
    with overlap(1):
        on = unet_plan(m, 2)
        assert hoisted(on) and unet_plan(m, 2) == on                   # planned once: the same report (same buffers) while nothing changes
        assert hoisted(vae_plan(v, 1, 1))
        set_overlap(0)
        off = unet_plan(m, 2)
        assert not hoisted(off) and len(off) == len(on)
        assert not hoisted(vae_plan(v, 1, 1))
        set_overlap(1)
        assert hoisted(unet_plan(m, 2)) == hoisted(on)
        assert hoisted(vae_plan(v, 1, 1))
        set_overlap(-1)
        assert bool(hoisted(unet_plan(m, 2))) == env_default()
        assert bool(hoisted(vae_plan(v, 0, 1))) == env_default()
        # the captured loop: sample under each setting, then ask for the plan it ran on
        pipe = AudioDiffusionPipeline(None, m, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1), DDIMScheduler()).to(dev)
        pipe.set_progress_bar_config(disable=True)
        noise = torch.randn(2, 1, 16, 16, generator=torch.Generator().manual_seed(0)).to(dev)
        for val in (1, 0, 1):
            set_overlap(val)
            pipe(batch_size=2, steps=2, noise=noise.clone(), audio=False, return_float=True)
            assert bool(hoisted(unet_plan(m, 2))) == bool(val), val


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_rejected_value_is_neither_remembered_nor_re_plans(backend):
    """adm_set_option validates before it records: "side_overlap" = 2 raises, the option keeps its value (0 here — a remembered 2 would switch
    the side launches on) and the dispatch epoch stays where it was (no re-plan: the same report, buffers included)."""
    select(backend)
    m = _unet(tu.TINY)
    with overlap(0):
        before = unet_plan(m, 2)
        assert not hoisted(before)
        with pytest.raises(RuntimeError, match="side_overlap"):
            set_overlap(2)
        after = unet_plan(m, 2)
        assert after == before
        set_overlap(1)                                                 # (the option still works after the rejection)
        assert hoisted(unet_plan(m, 2))


# ----------------------------------------------------------------------------------------------------------------- d. bits, tiny models
def _both(fn):
    """fn() with the side launches on and off (the option set explicitly either way): the results, in that order."""
    out = []
    for v in (1, 0):
        with overlap(v):
            out.append(fn())
    return out


@pytest.mark.parametrize("backend", BACKENDS)
def test_tiny_results_are_bit_identical_with_and_without_the_side_stream(backend):
    """The hoisted order moves no arithmetic: the tiny UNet forward (per-sample timesteps), a 3-step DDIM sampling through adm_sample_loop,
    the tiny conditional forward and the tiny VAE encode / decode are torch.equal with the overlap on and off."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel
    dev = select(backend)
    g = torch.Generator().manual_seed(7)
    m = _unet(tu.TINY)
    x = torch.randn(3, 1, 16, 16, generator=g).to(dev)
    ts = torch.tensor([3, 480, 997])
    with overlap(1):
        assert hoisted(unet_plan(m, 3))
    a, b = _both(lambda: m(x, ts)["sample"].cpu())
    assert torch.equal(a, b)

    pipe = AudioDiffusionPipeline(None, m, Mel(x_res=16, y_res=16, hop_length=64, n_fft=256, n_iter=1), DDIMScheduler()).to(dev)
    pipe.set_progress_bar_config(disable=True)
    noise = torch.randn(2, 1, 16, 16, generator=g).to(dev)
    a, b = _both(lambda: pipe(batch_size=2, steps=3, noise=noise.clone(), audio=False, return_float=True)[1].cpu())
    assert torch.equal(a, b)

    cm = _cond(tc.TINY)
    xc = torch.randn(2, 1, 16, 16, generator=g).to(dev)
    enc = torch.randn(2, 1, tc.TINY["cross_attention_dim"], generator=g).to(dev)
    with overlap(1):
        assert hoisted(unet_plan(cm, 2))
    a, b = _both(lambda: cm(xc, torch.tensor([11, 900]), enc)["sample"].cpu())
    assert torch.equal(a, b)

    v = _vae(tv.TINY)
    xi = torch.randn(2, 1, 32, 32, generator=g).to(dev)
    z = torch.randn(2, 1, 16, 16, generator=g).to(dev)
    a, b = _both(lambda: (v.encode(xi).latent_dist.mode().cpu(), v.decode(z)["sample"].cpu()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ----------------------------------------------------------------------------------------------------------------- device: the shipped plans
CFG256 = dict(sample_size=(256, 256), in_channels=1, out_channels=1, layers_per_block=2,
              block_out_channels=(128, 128, 256, 256, 512, 512),
              down_block_types=("DownBlock2D",) * 4 + ("AttnDownBlock2D", "DownBlock2D"),
              up_block_types=("UpBlock2D", "AttnUpBlock2D") + ("UpBlock2D",) * 4)
LATENT = dict(CFG256, sample_size=(32, 32))                      # config 4's UNet (tests/test_full_size.py)
VAE4 = dict(sample_size=(256, 256), in_channels=1, out_channels=1, latent_channels=1, layers_per_block=2,
            block_out_channels=(128, 256, 512, 512), down_block_types=("DownEncoderBlock2D",) * 4,
            up_block_types=("UpDecoderBlock2D",) * 4)
FACADE = {"wino6": 256, "single_sample": 1}                      # what audiodiffusion.AudioDiffusion sets on its own model

# Side launches per shipped plan, counted from the plan reports on the MI355X. They follow from the graphs: the 1x1 convolutions that
# qualify are the resnets' conv_shortcut (the attention / transformer 1x1s read the op right in front of them), every one of them is hoisted
# in front of its norm1 while its output has at most 4 Mi elements. 256x256 model: 20 shortcuts (2 down, 18 up); per sample the up levels
# give 32 Ki (8x8) .. 8 Mi (256x256) elements, so B = 1: 17 (all but the 256x256 level), B = 4: 14 (not 128x128 / 256x256), B = 32: 7
# (the 8x8 / 16x16 up levels and the 16x16 down shortcut). The latent UNet's planes are small: all 20 at B = 1 and 16. The config-4 VAE at
# B = 1: encoder 2 (128 -> 256 at 128x128: exactly 4 Mi, 256 -> 512 at 64x64), decoder 1 (512 -> 256 at 128x128; the 256x256 one is too
# large). The per-model rules change kernels, not these counts: a 1x1 shortcut never has a statistics epilogue.
SHIPPED = {
    ("unet256", "default", 1): 17, ("unet256", "default", 4): 14, ("unet256", "default", 32): 7,
    ("unet256", "facade", 1): 17, ("unet256", "facade", 4): 14, ("unet256", "facade", 32): 7,
    ("latent", "default", 1): 20, ("latent", "default", 16): 20,
    ("vae4-encoder", "default", 1): 2, ("vae4-decoder", "default", 1): 1,
}


@pytest.fixture(scope="module")
def models():
    """The shipped architectures with init_random weights, built once for the device tests (and only when one of them runs)."""
    from audiodiffusion import UNet2DModel
    select("hip")
    d = _unet(CFG256, 0)
    f = UNet2DModel(**CFG256).load_state_dict(d.state_dict())
    for k, val in FACADE.items():
        f.set_option(k, val)
    return {"default": d, "facade": f, "latent": _unet(LATENT, 4), "vae4": _vae(VAE4, 5)}


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(SHIPPED), ids=["-".join(map(str, k)) for k in SHIPPED])
def test_the_shipped_plans_keep_the_window_ops_off_the_side_launch(models, key):
    name, rules, B = key
    with overlap(1):
        if name == "unet256":
            plan = unet_plan(models[rules], B)
        elif name == "latent":
            plan = unet_plan(models["latent"], B)
        else:
            plan = vae_plan(models["vae4"], 0 if name.endswith("encoder") else 1, B)
    check_plan(plan, key)
    assert len(hoisted(plan)) == SHIPPED[key], (key, len(hoisted(plan)))


# ----------------------------------------------------------------------------------------------------------------- e. bits, device
@pytest.mark.gpu
@pytest.mark.parametrize("rules", ["default", "facade"])
def test_unet256_forward_is_bit_identical_with_and_without_the_side_stream(models, rules):
    m = models[rules]
    g = torch.Generator().manual_seed(21)
    for B, ts in ((1, [613]), (4, [0, 250, 640, 999])):
        x = torch.randn(B, 1, 256, 256, generator=g).cuda()
        a, b = _both(lambda: m(x, torch.tensor(ts))["sample"].cpu())
        assert torch.equal(a, b), (rules, B, float((a - b).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("rules,B", [("facade", 1), ("default", 4)])
def test_unet256_captured_sampling_is_bit_identical_with_and_without_the_side_stream(models, rules, B):
    """5 DDIM steps through the captured hipGraph (fork / join events and the side launch captured as a branch): on, off, on again — the
    option re-plans the model, which drops the captured loop, so each run is a fresh capture under its own setting."""
    from audiodiffusion import AudioDiffusionPipeline, DDIMScheduler, Mel
    pipe = AudioDiffusionPipeline(None, models[rules], Mel(), DDIMScheduler()).to(torch.device("cuda:0"))
    pipe.set_progress_bar_config(disable=True)
    noise = torch.randn(B, 1, 256, 256, generator=torch.Generator().manual_seed(22)).cuda()
    out = []
    for v in (1, 0, 1):
        with overlap(v):
            out.append(pipe(batch_size=B, steps=5, noise=noise.clone(), audio=False, return_float=True)[1].cpu())
            assert bool(hoisted(unet_plan(models[rules], B))) == bool(v)      # the plan the loop ran on
    assert torch.equal(out[0], out[2]) and torch.equal(out[0], out[1]), [float((o - out[0]).abs().max()) for o in out]


@pytest.mark.gpu
def test_vae4_decode_and_encode_are_bit_identical_with_and_without_the_side_stream(models):
    v = models["vae4"]
    g = torch.Generator().manual_seed(23)
    z = torch.randn(1, 1, 32, 32, generator=g).cuda()
    x = torch.randn(1, 1, 256, 256, generator=g).cuda()
    a, b = _both(lambda: (v.decode(z)["sample"].cpu(), v.encode(x).latent_dist.mode().cpu()))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# The window in which the side launch and a main-stream convolution both split K (each stream then has its own split-K slab buffer): the
# latent UNet's down_blocks.4.resnets.0 at B = 1 — norm1 (op 38), conv1 (op 39: 3x3 256 -> 512 on the 2x2 plane, generic split-K kernel,
# whose finish pass leaves norm2's scale / shift), norm2 (op 40), beside conv_shortcut (op 41: 1x1 256 -> 512, split-K generic kernel).
# (The 8x8 up level of the 256x256 model does not qualify: a 1x1 on an 8x8 plane runs the unsplit pipelined kernel.) The profile has one
# record per op after the time-embedding projection's, so record 1 + k is op k.
SPLIT_K = {116, 117, 119, 316, 317, 319, 326, 327, 329, 2316, 2317, 4317}    # variants of the split-K launches (k_conv_mfma.hip, k_conv_wino.hip)
WINDOW = (38, 41)


@pytest.mark.gpu
def test_split_k_beside_split_k_is_bit_identical_with_and_without_the_side_stream(models):
    N = _N()
    m = models["latent"]
    x = torch.randn(1, 1, 32, 32, generator=torch.Generator().manual_seed(24)).cuda()
    with overlap(1):
        plan = unet_plan(m, 1)
        recs, n = (N.OpProfile * 1024)(), C.c_int(0)
        out = torch.empty_like(x)
        N.check(N.lib().adm_unet_profile(m._ensure_handle(), N.ptr(x), 500.0, N.ptr(out), 1, recs, 1024, C.byref(n), N.stream_for(x)))
    assert n.value == len(plan) + 1
    var = [recs[1 + k].variant for k in range(len(plan))]
    i, j = WINDOW
    assert plan[j].hoist == i and plan[j].ks == 1, plan[j]
    assert var[j] in SPLIT_K, var[j]
    assert any(plan[k].kind == CONV and var[k] in SPLIT_K for k in range(i, j)), var[i:j]
    a, b = _both(lambda: m(x, torch.tensor([500]))["sample"].cpu())
    assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(a, out.cpu())                                   # (the profile's in-order eager forward: the same bits)
