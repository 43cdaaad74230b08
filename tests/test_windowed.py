"""Windowed sampling (include/adm.h "Windowed sampling"; adm_version() >= 117): one wide sample denoised jointly through overlapping
model-sized windows — `adm_window_gather`, `adm_window_blend` (csrc/k_window.hip), the three window fields of `adm_sample_loop_args`
(csrc/unet_exec.hip) and the `frames` / `window_stride` / `circular` keywords of the pipeline.

A. the two kernels against numpy restatements of the definition, bit for bit, and their refusals
B. loop identities, bit for bit: against the ordinary loop where the two must agree, and against the same steps composed from the
   public pieces (`ops.window_gather`, the model, `ops.window_blend`, `scheduler.step` on the wide tensors)
C. seamlessness: on the circle, rolling the initial noise by one stride rolls the result by one stride, bit for bit
D. against the oracle UNet and scheduler through a torch restatement of the windowed loop kept here
E. plumbing: widths, audio length, the errors, the facade, `longform.generate_long`, and the zero fields of an ordinary call

The shapes are the smallest at which the indexing can go wrong: W = 16 (the tiny models of tests/test_dpmsolver.py) and every
placement of PLACEMENTS, with B in {1, 2}, C in {1, 2}, H in {1, 4}; B = 2 and C = 2 are what expose a wrong row or channel stride.
"""
import numpy as np
import pytest
import torch

import test_dpmsolver as td
from native_backend import BACKENDS, select, spy_sample_loop
from oracle import mel as omel
from oracle import schedulers as osched
from oracle.unet import UNet2DModel as OracleUNet

W = 16
#             Wt  s   circular        nW  cover
PLACEMENTS = [(16, 16, False),      # 1   1
              (48, 16, False),      # 3   1
              (32, 8, False),       # 3   1-2
              (28, 12, False),      # 2   1-2
              (24, 4, False),       # 3   1-3
              (32, 8, True),        # 4   2
              (24, 12, True),       # 2   1-2
              (32, 4, True),        # 8   4
              (20, 4, True)]        # 5   4
PIDS = [f"{wt}-{s}-{'circular' if c else 'open'}" for wt, s, c in PLACEMENTS]


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _cols(Wt, Wm, s, wrap):
    """(nW, Wm) columns of the wide sample that each window covers: the placement table of the definition."""
    nW = Wt // s if wrap else (Wt - Wm) // s + 1
    cols = np.arange(nW)[:, None] * s + np.arange(Wm)[None, :]
    return cols % Wt if wrap else cols


def _np_gather(x, Wm, s, wrap):
    B, Cc, H, Wt = x.shape
    cols = _cols(Wt, Wm, s, wrap)
    win = x[:, :, :, cols]                                        # (B, C, H, nW, Wm)
    return np.ascontiguousarray(win.transpose(0, 3, 1, 2, 4)).reshape(B * len(cols), Cc, H, Wm)


def _np_blend(win, Wt, s, wrap):
    """The definition, sequentially in fp32: ascending window index, the sum starts from the first window's value, every addition is
    an fp32 addition, one fp32 division by the cover count. -> (mean, cover count per column)"""
    BW, Cc, H, Wm = win.shape
    cols = _cols(Wt, Wm, s, wrap)
    nW = len(cols)
    win = win.reshape(BW // nW, nW, Cc, H, Wm)
    acc = np.zeros((BW // nW, Cc, H, Wt), np.float32)
    count = np.zeros(Wt, np.int64)
    for w in range(nW):
        first = count[cols[w]] == 0
        o = win[:, w]
        acc[..., cols[w][first]] = o[..., first]
        acc[..., cols[w][~first]] = (acc[..., cols[w][~first]] + o[..., ~first]).astype(np.float32)
        count[cols[w]] += 1
    assert count.min() >= 1
    return (acc / count.astype(np.float32)).astype(np.float32), count


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ================================================================ A. the kernels
def _check_kernels(dev, shape, Wm, s, wrap, seed):
    from audiodiffusion import ops
    x = _randn(shape, seed)
    Wt = shape[3]
    win = ops.window_gather(x.to(dev), Wm, s, wrap)
    want = _np_gather(x.numpy(), Wm, s, wrap)
    assert tuple(win.shape) == want.shape and np.array_equal(_bits(win.cpu().numpy()), _bits(want)), (shape, s, wrap)
    # the blend of independent window values (what the model's outputs are), not of a gather
    o = _randn(want.shape, seed + 1)
    mean = ops.window_blend(o.to(dev), Wt, s, wrap)
    ref, count = _np_blend(o.numpy(), Wt, s, wrap)
    assert tuple(mean.shape) == ref.shape == tuple(shape) and np.array_equal(_bits(mean.cpu().numpy()), _bits(ref)), (shape, s, wrap)
    # blend(gather(x)) == x wherever the cover is 1, 2 or 4 ((x + x + x) / 3 is not x)
    back = ops.window_blend(win, Wt, s, wrap).cpu().numpy()
    exact = np.isin(count, (1, 2, 4))
    assert exact.any() and np.array_equal(_bits(back[..., exact]), _bits(x.numpy()[..., exact])), (shape, s, wrap)
    return count


@pytest.mark.parametrize("Wt,s,wrap", PLACEMENTS, ids=PIDS)
@pytest.mark.parametrize("backend", BACKENDS)
def test_gather_and_blend_are_the_definition_bit_for_bit(backend, Wt, s, wrap):
    dev = select(backend)
    covers = set()
    for B in (1, 2):
        for Cc in (1, 2):
            for H in (1, 4):
                covers |= set(_check_kernels(dev, (B, Cc, H, Wt), W, s, wrap, 7 + B + 2 * Cc + H).tolist())
    want = {(16, 16, False): {1}, (48, 16, False): {1}, (32, 8, False): {1, 2}, (28, 12, False): {1, 2}, (24, 4, False): {1, 2, 3},
            (32, 8, True): {2}, (24, 12, True): {1, 2}, (32, 4, True): {4}, (20, 4, True): {4}}[(Wt, s, wrap)]
    assert covers == want          # the table of the issue: this case exercises the covers it is there for


@pytest.mark.parametrize("shape,Wm,s,wrap", [((1, 1, 256, 1024), 256, 128, False), ((3, 1, 256, 3072), 256, 128, True)],
                         ids=["1x1x256x1024-open", "3x1x256x3072-circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_gather_and_blend_at_size(backend, shape, Wm, s, wrap):
    """The grid-stride loop. The second case has more float4 than the capped grid has lanes (2048 blocks of 256) in both kernels:
    589824 in the wide tensor, 24 windows per sample on top of that in the gather."""
    dev = select(backend)
    _check_kernels(dev, shape, Wm, s, wrap, 3)


@pytest.mark.parametrize("backend", BACKENDS)
def test_kernel_refusals_carry_the_name_of_the_argument(backend):
    dev = select(backend)
    from audiodiffusion import _native as N
    lib = N.lib()
    assert lib.adm_version() >= 117
    a, b = torch.zeros(4096, device=dev), torch.zeros(4096, device=dev)
    ok = dict(B=1, C=1, H=1, total_w=32, W=16, stride=8, wrap=0)
    cases = [(dict(total_w=34), "total_w"), (dict(total_w=12), "total_w"), (dict(total_w=36), "total_w"),          # % 4, < W, (Wt - W) % s
             (dict(total_w=40, stride=16, wrap=1), "total_w"),                                                    # circular: Wt % s
             (dict(stride=6), "stride"), (dict(stride=0), "stride"), (dict(stride=-8), "stride"), (dict(stride=20, total_w=36), "stride"),
             (dict(wrap=2), "wrap"), (dict(wrap=-1), "wrap"), (dict(W=18), "W"), (dict(B=0), "B"), (dict(C=0), "C"),
             (dict(B=1 << 30, total_w=48), "int")]                                                               # B * nW past int
    for fn in (lib.adm_window_gather, lib.adm_window_blend):
        for bad, word in cases:
            k = dict(ok, **bad)
            rc = fn(N.ptr(a), N.ptr(b), k["B"], k["C"], k["H"], k["total_w"], k["W"], k["stride"], k["wrap"], None)
            assert rc != 0 and word in lib.adm_last_error().decode(), (bad, lib.adm_last_error())
        for pa, pb in ((None, N.ptr(b)), (N.ptr(a), None)):
            assert fn(pa, pb, *[ok[k] for k in ("B", "C", "H", "total_w", "W", "stride", "wrap")], None) != 0
            assert "null" in lib.adm_last_error().decode()
        assert fn(N.ptr(a), N.ptr(b), *[ok[k] for k in ("B", "C", "H", "total_w", "W", "stride", "wrap")], None) == 0


# ================================================================ B. loop identities
def _pipe(sched, cond=False):
    """This package's pipeline over the tiny weights of tests/test_dpmsolver.py, and the oracle UNet that holds the same weights."""
    from audiodiffusion import AudioDiffusionPipeline, Mel, UNet2DConditionModel, UNet2DModel
    torch.manual_seed(0)
    if cond:
        from oracle.unet_condition import UNet2DConditionModel as OracleCond
        ref_unet = OracleCond(**td.COND).eval()
        unet = UNet2DConditionModel(**td.COND).load_state_dict(ref_unet.state_dict())
    else:
        ref_unet = OracleUNet(**td.TINY).eval()
        unet = UNet2DModel(**td.TINY).load_state_dict(ref_unet.state_dict())
    mine = AudioDiffusionPipeline(None, unet, Mel(**td.MEL), sched)
    mine.set_progress_bar_config(disable=True)
    return ref_unet, mine


def _den(mine, x, eta=0.0, **kw):
    return mine._denoise(x, 0, eta, None, None, 0, 0, **kw)


def _scheduler(kind, **cfg):
    import audiodiffusion as ad
    return {"ddim": ad.DDIMScheduler, "ddpm": ad.DDPMScheduler, "dpm": ad.DPMSolverMultistepScheduler,
            "unipc": ad.UniPCMultistepScheduler}[kind](**cfg)


@pytest.mark.parametrize("backend", BACKENDS)
def test_frames_equal_to_the_model_width_is_the_ordinary_loop(backend):
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    mine.scheduler.set_timesteps(3)
    x0 = _randn((2, 1, 16, 16), 9).to(dev)
    plain, u8 = _den(mine, x0)
    for s in (16, 8):                                   # open, one window: a copy, a forward, a division by 1.0f
        wide, u8w = _den(mine, x0, window_stride=s)
        assert torch.equal(plain, wide) and torch.equal(u8, u8w)


@pytest.mark.parametrize("kind", ["ddim", "dpm", "unipc"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_disjoint_windows_are_the_ordinary_loop_on_the_windows_as_a_batch(backend, kind):
    """Open, stride == W, frames = 3 W, B = 2: nothing overlaps, so the wide result is the ordinary loop run on the six windows stacked
    as a batch of 6. The multistep history and the UniPC state have the wide shape in one run and the windows' in the other."""
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = _pipe(_scheduler(kind))
    mine.scheduler.set_timesteps(4)
    x0 = _randn((2, 1, 16, 48), 5).to(dev)
    wide, u8 = _den(mine, x0, window_stride=16)
    stacked, u8s = _den(mine, ops.window_gather(x0, 16, 16))
    assert tuple(wide.shape) == (2, 1, 16, 48) and tuple(stacked.shape) == (6, 1, 16, 16)
    assert torch.equal(ops.window_gather(wide, 16, 16), stacked)
    assert tuple(u8.shape) == (2, 16, 48, 1)
    assert torch.equal(u8.reshape(2, 16, 3, 16).permute(0, 2, 1, 3).reshape(6, 16, 16, 1), u8s)


def _composed(mine, x0, s, wrap, enc=None, neg=None, **step_kw):
    """The windowed loop, step by step from the public pieces. step_kw: keywords of scheduler.step; a list holds one value per step."""
    from audiodiffusion import ops
    sched, y, Wt = mine.scheduler, x0, x0.shape[3]
    nW = len(_cols(Wt, W, s, wrap))
    for k, t in enumerate(sched.timesteps):
        win = ops.window_gather(y, W, s, wrap)
        kw = {n: (v[k] if isinstance(v, list) else v) for n, v in step_kw.items()}
        if enc is None:
            o = ops.window_blend(mine.unet(win, t)["sample"], Wt, s, wrap)
        else:
            o = ops.window_blend(mine.unet(win, t, enc.repeat_interleave(nW, 0))["sample"], Wt, s, wrap)
            if neg is not None:
                kw["model_output_uncond"] = ops.window_blend(mine.unet(win, t, neg.repeat_interleave(nW, 0))["sample"], Wt, s, wrap)
        y = sched.step(o, t, y, **kw).prev_sample
    return y


TH = dict(thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=4.0)
COMPOSED = ["ddim-clamp", "ddpm-step-noise", "ddpm-device-noise", "ddpm-device-noise-row-offset", "dpm", "unipc-v-thresholded",
            "guided", "guided-rescaled"]


@pytest.mark.parametrize("case", COMPOSED)
@pytest.mark.parametrize("wrap", [False, True], ids=["open", "circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_the_native_loop_is_the_steps_composed_from_the_public_pieces(backend, wrap, case):
    dev = select(backend)
    n, s, B, Wt = 3, 8, 2, 32
    x0 = _randn((B, 1, 16, Wt), 21).to(dev)
    den_kw, step_kw, enc, neg, cond = {}, {}, None, None, case.startswith("guided")
    if case == "ddim-clamp":
        sched = _scheduler("ddim")
        assert sched.config.clip_sample
    elif case.startswith("ddpm"):
        sched = _scheduler("ddpm")
        if case == "ddpm-step-noise":
            sched.set_timesteps(n)
            noisy = [r["k_noise"] != 0.0 for r in sched.coef_rows(0.0)]           # (the last row, t = 0, adds no noise)
            sn = [_randn((B, 1, 16, Wt), 30 + i).to(dev) for i in range(n)]
            den_kw, step_kw = dict(step_noise=sn), dict(variance_noise=[v if noisy[i] else None for i, v in enumerate(sn)])
            assert noisy == [True, True, False]
        else:
            off = 5 if case.endswith("row-offset") else 0
            den_kw = dict(device_noise_seed=77, device_noise_row_offset=off)
            step_kw = dict(device_noise_seed=77, device_noise_row_offset=off)
    elif case == "dpm":
        sched = _scheduler("dpm")
    elif case == "unipc-v-thresholded":
        sched = _scheduler("unipc", prediction_type="v_prediction", **TH)
    else:
        sched = _scheduler("ddim")
        enc, neg = _randn((B, 1, 12), 40).to(dev), (0.5 * _randn((B, 1, 12), 41)).to(dev)
        phi = 0.7 if case == "guided-rescaled" else None
        den_kw = dict(encoding=enc, negative_encoding=neg, guidance_scale=3.0, guidance_rescale=phi)
        step_kw = dict(guidance_scale=3.0, guidance_rescale=phi)
    _, mine = _pipe(sched, cond=cond)
    sched.set_timesteps(n)
    whole, _ = _den(mine, x0, window_stride=s, circular=wrap, **den_kw)
    sched.set_timesteps(n)
    y = _composed(mine, x0, s, wrap, enc=enc, neg=neg, **step_kw)
    assert torch.equal(whole, y)
    assert float((whole - x0).abs().max()) > 1e-2


@pytest.mark.parametrize("backend", BACKENDS)
def test_graph_replay_second_call_and_batch_independence(backend):
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    mine.scheduler.set_timesteps(3)
    x0 = _randn((2, 1, 16, 32), 13).to(dev)
    kw = dict(window_stride=8, circular=True)
    whole, u8 = _den(mine, x0, **kw)
    if backend != "emu":             # (the emulator has no graph: both settings are the same code there)
        eager, u8e = _den(mine, x0, use_graph=False, **kw)
        assert torch.equal(whole, eager) and torch.equal(u8, u8e)
    again, u8a = _den(mine, x0, **kw)
    assert torch.equal(whole, again) and torch.equal(u8, u8a)
    one, u81 = _den(mine, x0[1:2].contiguous(), **kw)
    assert torch.equal(whole[1:2], one) and torch.equal(u8[1:2], u81)


@pytest.mark.parametrize("backend", BACKENDS)
def test_windowed_and_ordinary_loops_alternate_on_one_handle(backend):
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    mine.scheduler.set_timesteps(3)
    xw, xo =_randn((2, 1, 16, 32), 14).to(dev), _randn((2, 1, 16, 16), 15).to(dev)
    w1, o1 = _den(mine, xw, window_stride=8)[0], _den(mine, xo)[0]
    handle = mine.unet._handle
    c1 = _den(mine, xw, window_stride=8, circular=True)[0]
    w2, o2, c2 = _den(mine, xw, window_stride=8)[0], _den(mine, xo)[0], _den(mine, xw, window_stride=8, circular=True)[0]
    assert mine.unet._handle == handle and tuple(mine.unet._hw()) == (16, 16)       # the model kept its own width throughout
    assert torch.equal(w1, w2) and torch.equal(o1, o2) and torch.equal(c1, c2) and not torch.equal(w1, c1)


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_windowed_run_is_one_native_call(backend, monkeypatch):
    dev = select(backend)
    for kind, kw in (("unipc", {}), ("ddpm", dict(device_noise_seed=5))):
        _, mine = _pipe(_scheduler(kind))
        calls = spy_sample_loop(monkeypatch)
        images = mine(batch_size=2, steps=4, frames=32, window_stride=8, circular=True, audio=False, return_dict=False, **kw)[0]
        monkeypatch.undo()
        assert [c["symbol"] for c in calls] == ["adm_sample_loop_ex"]
        c = calls[0]
        assert (c["window_total_w"], c["window_stride"], c["window_wrap"], c["B"], c["n_steps"]) == (32, 8, 1, 2, 4)
        assert (c["unipc_host"] is not None) == (kind == "unipc") and c["noise_source"] == (1 if kind == "ddpm" else 0)
        assert len(images) == 2 and images[0].size == (32, 16)
    assert dev is not None


# ================================================================ C. seamlessness
@pytest.mark.parametrize("backend", BACKENDS)
def test_on_the_circle_a_roll_of_the_noise_is_a_roll_of_the_result(backend):
    """Not a restatement of the definition. Circular, stride W/2 (cover 2), DDIM with eta 0: rolling the initial wide noise by one
    stride along the time axis turns window w into window w + 1 and swaps the order of the two terms of every sum; a + b is
    commutative, so the result is the rolled result bit for bit, and the seam is a column like any other."""
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    mine.scheduler.set_timesteps(3)
    x0 = _randn((2, 1, 16, 32), 17).to(dev)
    kw = dict(window_stride=8, circular=True)
    a, u8a = _den(mine, x0, **kw)
    b, u8b = _den(mine, torch.roll(x0, 8, dims=3).contiguous(), **kw)
    assert torch.equal(torch.roll(a, 8, dims=3), b) and torch.equal(torch.roll(u8a, 8, dims=2), u8b)
    open_, _ = _den(mine, x0, window_stride=8)          # the open placement has edges: it is another sample
    assert not torch.equal(open_, a)


# ================================================================ D. against the oracle
def _oracle_windowed(ref_unet, x, s, wrap, steps):
    """A torch restatement of the windowed loop on the oracle UNet and the oracle DDIM scheduler."""
    sched = osched.DDIMScheduler()
    sched.set_timesteps(steps)
    B, Cc, H, Wt = x.shape
    cols = torch.from_numpy(_cols(Wt, W, s, wrap))
    nW = len(cols)
    count = torch.zeros(Wt)
    for w in range(nW):
        count[cols[w]] += 1
    with torch.no_grad():
        for t in sched.timesteps:
            win = x[:, :, :, cols].permute(0, 3, 1, 2, 4).reshape(B * nW, Cc, H, W)
            o = ref_unet(win, t)["sample"].reshape(B, nW, Cc, H, W)
            acc = torch.zeros_like(x)
            for w in range(nW):
                acc[..., cols[w]] += o[:, w]
            x = sched.step(acc / count, t, x)["prev_sample"]
    return x


def _u8(x):
    return ((x / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy() * 255).round().astype("uint8")


@pytest.mark.parametrize("wrap", [False, True], ids=["open", "circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_sampling_matches_the_oracle(backend, wrap):
    """The bars of section D of tests/test_dpmsolver.py (from tests/test_pipeline.py): max|d| <= 1e-3 on the floats, images within 1 LSB."""
    dev = select(backend)
    ref_unet, mine = _pipe(_scheduler("ddim"))
    noise = _randn((2, 1, 16, 32), 42)
    rf = _oracle_windowed(ref_unet, noise.clone(), 8, wrap, 4)
    mi, mf = mine(batch_size=2, steps=4, noise=noise.clone().to(dev), frames=32, window_stride=8, circular=wrap, audio=False,
                  return_float=True)
    err = float((mf.cpu() - rf).abs().max())
    a, b = np.stack([np.asarray(i).astype(int) for i in mi]), _u8(rf)[..., 0].astype(int)
    print(f"WINDOWED oracle wrap={wrap} max|d|={err:.3e} lsb={np.abs(a - b).max()}")
    assert err <= 1e-3
    assert a.shape == b.shape == (2, 16, 32) and np.abs(a - b).max() <= 1


@pytest.mark.parametrize("backend", BACKENDS)
def test_wide_audio_matches_the_oracle_codec(backend):
    """The wide image goes through a Mel with x_res = frames; compared with the oracle codec on the same image and start phase at the
    bar every injected-phase codec comparison of the suite uses (tests/test_mel.py, tests/test_golden.py, tests/test_full_size.py):
    max|d| <= 1e-3 max|ref|. (tests/test_pipeline.py itself compares no audio.)"""
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    frames = 32
    phase = np.random.default_rng(0).random((1, 1 + td.MEL["n_fft"] // 2, frames))
    images, (sr, audios) = mine(batch_size=1, steps=2, noise=_randn((1, 1, 16, frames), 3).to(dev), frames=frames, circular=True,
                                return_dict=False, init_phase=phase)
    want = omel.Mel(**dict(td.MEL, x_res=frames)).image_to_audio(images[0], init_phase=phase[0])
    assert sr == td.MEL["sample_rate"] and audios[0].shape == want.shape == (td.MEL["hop_length"] * (frames - 1),)
    rel = float(np.abs(audios[0] - want).max() / np.abs(want).max())
    print(f"WINDOWED audio rel err={rel:.3e}")
    assert rel <= 1e-3
    assert mine.mel.x_res == 16                      # the pipeline's own Mel is not touched


# ================================================================ E. plumbing
@pytest.mark.parametrize("backend", BACKENDS)
def test_output_widths_audio_length_and_device_noise_latent(backend):
    from audiodiffusion import ops
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    out = mine(batch_size=2, steps=2, frames=48, generator=torch.Generator().manual_seed(1))       # default stride W // 2, open
    assert [i.size for i in out.images] == [(48, 16)] * 2 and out.audios.shape == (2, 1, td.MEL["hop_length"] * 47)
    kw = dict(batch_size=2, steps=2, frames=32, circular=True, audio=False, return_float=True)
    _, a = mine(device_noise_seed=11, device_noise_row_offset=3, **kw)
    latent = ops.randn((2, 1, 16, 32), 11, row_offset=3, noise_stream=1, device=dev)                # drawn at the wide shape
    _, b = mine(noise=latent, **kw)
    assert tuple(a.shape) == (2, 1, 16, 32) and torch.equal(a, b)


@pytest.mark.parametrize("backend", BACKENDS)
def test_every_refusal_names_its_keyword(backend, monkeypatch):
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    calls = spy_sample_loop(monkeypatch)
    kw = dict(steps=2, audio=False)
    for bad, word in [(dict(frames=30), "frames"), (dict(frames=12), "frames"), (dict(frames=36), "frames"),
                      (dict(frames=40, window_stride=16, circular=True), "frames"), (dict(frames=32, window_stride=6), "window_stride"),
                      (dict(frames=32, window_stride=0), "window_stride"), (dict(frames=36, window_stride=20), "window_stride"),
                      (dict(frames=32, circular=2), "circular"), (dict(window_stride=8), "window_stride"), (dict(circular=True), "circular"),
                      (dict(frames=32, raw_audio=np.zeros(2000, np.float32)), "raw_audio"), (dict(frames=32, audio_file="x.wav"), "audio_file"),
                      (dict(frames=32, mask_start_secs=0.1), "mask_start_secs"), (dict(frames=32, mask_end_secs=0.1), "mask_end_secs"),
                      (dict(frames=32, noise=torch.zeros(1, 1, 16, 16, device=dev)), "noise")]:
        with pytest.raises(ValueError, match=word):
            mine(**kw, **bad)
    mine.vqvae = object()
    with pytest.raises(NotImplementedError, match="vqvae"):
        mine(frames=32, **kw)
    assert calls == []               # all of it before any work
    monkeypatch.undo()
    # the C-ABI's own refusals, each by name
    from audiodiffusion import _native as N
    mine.vqvae = None
    mine(batch_size=1, **kw)         # a finalized handle
    lib, h = N.lib(), mine.unet._handle
    x = torch.zeros(1, 1, 16, 32, device=dev)
    coef = (N.SchedCoef * 1)(N.SchedCoef(0.5, 0.5, 1.0, 1.0, 0.0, 0.0, 0.0, 10.0))

    def refused(word, **f):
        a = N.SampleLoopArgs(x=N.ptr(x), B=1, coef_host=coef, n_steps=1, use_graph=0, max_value=1.0, guidance_scale=1.0, **f)
        assert lib.adm_sample_loop_ex(h, a, None) != 0 and word in lib.adm_last_error().decode(), (f, lib.adm_last_error())
    refused("mask", window_total_w=32, window_stride=8, mask=N.ptr(x))
    refused("window_total_w", window_total_w=30, window_stride=8)
    refused("window_total_w", window_total_w=36, window_stride=8)
    refused("window_total_w", window_total_w=40, window_stride=16, window_wrap=1)
    refused("window_total_w", window_total_w=12, window_stride=4)
    refused("window_stride", window_total_w=32, window_stride=6)
    refused("window_stride", window_total_w=32, window_stride=0)
    refused("window_stride", window_total_w=36, window_stride=20)
    refused("window_wrap", window_total_w=32, window_stride=8, window_wrap=2)
    refused("mode", window_total_w=32, window_stride=8, mode=7)            # the checks that were there stay as they are
    refused("prediction", window_total_w=32, window_stride=8, prediction=5)
    refused("noise_source", window_total_w=32, window_stride=8, noise_source=3)


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_ordinary_call_hands_the_loop_zero_window_fields(backend, monkeypatch):
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    calls = spy_sample_loop(monkeypatch)
    mine(batch_size=1, steps=2, audio=False, noise=_randn((1, 1, 16, 16), 1).to(dev))
    assert len(calls) == 1 and (calls[0]["window_total_w"], calls[0]["window_stride"], calls[0]["window_wrap"]) == (0, 0, 0)


@pytest.mark.parametrize("backend", BACKENDS)
def test_front_end_and_generate_long_pass_the_keywords_through(backend, tmp_path):
    from audiodiffusion import AudioDiffusion, longform
    dev = select(backend)
    _, mine = _pipe(_scheduler("ddim"))
    mine.save_pretrained(str(tmp_path / "pipe"))
    front = AudioDiffusion(str(tmp_path / "pipe"), cuda=backend != "emu", progress_bar=None)
    front.pipe.set_progress_bar_config(disable=True)
    seen, real = {}, front.pipe._denoise

    def spy(*a, **kw):
        seen.update(kw)
        return real(*a, **kw)
    front.pipe._denoise = spy
    img, (sr, audio) = front.generate_spectrogram_and_audio(steps=2, frames=32, window_stride=4, circular=True)
    assert (seen["window_stride"], seen["circular"]) == (4, True) and img.size == (32, 16) and audio.shape == (64 * 31,)
    img, _ = front.generate_spectrogram_and_audio(steps=2)
    assert (seen["window_stride"], seen["circular"]) == (None, False) and img.size == (16, 16)
    # generate_long: one column is hop_length / sample_rate = 0.016 s, W = 16 columns = 0.256 s
    assert longform.long_placement(mine, 0.5, 0.128) == (32, 8)                     # 31.25 columns -> 16 + 2*8; overlap 8 columns
    assert longform.long_placement(mine, 0.5, 0.128, circular=True) == (32, 8)
    assert longform.long_placement(mine, 0.6, 0.07) == (40, 12)                     # 37.5 columns -> 16 + 2*12; overlap 4.375 -> stride 12
    assert longform.long_placement(mine, 0.6, 0.07, circular=True) == (48, 12)      # ... -> 4*12
    assert longform.long_placement(mine, 0.1, 0.0) == (16, 16)                      # never narrower than the model
    assert longform.long_placement(mine, 0.4, 1.0) == (28, 4)                       # the stride floor: 25 columns -> 16 + 3*4
    seen.clear()
    mine._denoise, real = spy, mine._denoise
    (images, (sr, audios)), used = longform.generate_long(mine, 0.6, 0.07, circular=True, steps=2, batch_size=2, return_dict=False)
    assert used["frames"] == 48 and used["window_stride"] == 12 and abs(used["seconds"] - 0.768) < 1e-9 and abs(used["overlap_secs"] - 0.064) < 1e-9
    assert (seen["window_stride"], seen["circular"]) == (12, True) and [i.size for i in images] == [(48, 16)] * 2
    assert audios[0].shape == (64 * 47,) and dev is not None
