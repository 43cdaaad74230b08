"""What keys the captured step of the sampling loop (include/adm.h, "what keys the captured step"; adm_version() >= 122), on the emulator
and, under `-m gpu`, on the MI355X.

`adm_unet_loop_captures` counts the captures of a handle, so a replay and a re-capture can be told apart. Every test is a chain of loop
calls on ONE handle and asserts, per call, by how much the counter went up. The expected increments are the contract of the header's
paragraph, not a measurement:

  +0  the same arguments; new CONTENTS at the same addresses; new values in a *_host table of the same n_steps; another seed / row_offset;
      any value in a field of a feature that is off; a use_graph=0 call in between;
  +1  any other difference -- and +1 again on the way back, because a handle holds one captured step.

On the MI355X every captured call is also compared, bit for bit, with the same arguments run with use_graph=0 on a second handle over the
same weights: a replay of a stale graph would return success and the wrong bits. (The emulator runs every step eagerly, so there the
counter is the whole check.)

Shapes: the conditional 16 x 16 tiny model of tests/test_sched_dispatch.py, and for the window fields the unconditional 16-wide tiny model
sampled 32 wide; B = 1, two steps. Every tensor is allocated once, at the largest size a test uses, and refilled in place before each
call: an address changes only where a test hands the loop another tensor.
"""
import ctypes as C

import pytest
import torch

import test_dpmsolver as td
import test_guidance as tg
from native_backend import BACKENDS, select
from test_sched_dispatch import _coef, _randn

THRESH, MULTISTEP = 1, 2
N_STEPS, H, W, WIDE = 2, 16, 16, 32


class _Rig:
    """A handle whose captures are counted and, on the MI355X, a second handle over the same weights that runs every loop eagerly."""

    def __init__(self, dev, handle, eager_handle, shapes):
        from audiodiffusion import _native as N
        self.N, self.lib, self.dev, self.h = N, N.lib(), dev, handle
        self.eager = eager_handle if dev.type == "cuda" else None
        self.t, self.master = {}, {}
        for name, shape in shapes.items():
            u8 = name.startswith(("u8", "keep"))
            self.t[name] = torch.zeros(shape, dtype=torch.uint8 if u8 else torch.float32, device=dev)
        self.contents(0)

    def contents(self, salt):
        """New contents for every tensor, at the same addresses."""
        for seed, (name, t) in enumerate(self.t.items()):
            if name.startswith("keep"):
                self.master[name] = (_randn(t.shape, 100 * salt + seed) > 0).to(torch.uint8)
            elif name.startswith("u8"):
                self.master[name] = torch.zeros(t.shape, dtype=torch.uint8)
            else:
                self.master[name] = (1.0 + 0.25 * salt) * _randn(t.shape, 100 * salt + seed)

    def on_both(self, fn):
        for h in (self.h, self.eager):
            if h is not None:
                self.N.check(fn(h))

    def _run(self, h, fields, use_graph):
        N = self.N
        for name, t in self.t.items():
            t.copy_(self.master[name])
        a = N.SampleLoopArgs(use_graph=use_graph)
        for k, v in fields.items():
            setattr(a, k, N.ptr(v) if isinstance(v, torch.Tensor) else v)
        N.check(self.lib.adm_sample_loop_ex(h, a, N.stream_for(fields["x"])))
        if self.dev.type == "cuda":
            torch.cuda.synchronize()
        out = [fields["x"].clone()] + ([fields["u8_out"].clone()] if fields.get("u8_out") is not None else [])
        assert bool(torch.isfinite(out[0]).all()) and not torch.equal(out[0].cpu(), self.master_of(fields["x"]))
        return out

    def master_of(self, tensor):
        return next(self.master[name] for name, t in self.t.items() if t is tensor)

    def call(self, fields, use_graph=1):
        """One loop on the counted handle -> by how much its capture counter went up."""
        before = self.lib.adm_unet_loop_captures(self.h)
        got = self._run(self.h, fields, use_graph)
        captured = self.lib.adm_unet_loop_captures(self.h) - before
        if self.eager is not None and use_graph:
            want = self._run(self.eager, fields, 0)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), "the captured loop differs from the eager one"
            assert self.lib.adm_unet_loop_captures(self.eager) == 0
        return captured

    def there_and_back(self, base, changes):
        """From `base` (the step the handle holds): each change captures, and so does the way back."""
        for change in changes:
            assert self.call({**base, **change}) == 1, change
            assert self.call(base) == 1, ("back from", change)


def _conditional(dev):
    """-> (rig, P): the conditional tiny model; P is the plain loop with staged noise, a mask and the u8 image."""
    from audiodiffusion import _native as N
    _, mine = tg._build("ddpm")
    _, other = tg._build("ddpm")
    image, noise = (2, 1, H, W), (N_STEPS + 1, 2, 1, H, W)
    rig = _Rig(dev, mine.unet._ensure_handle(), other.unet._ensure_handle(), {
        "x": image, "x_alt": image, "noise": noise, "noise_alt": noise, "mask": (2, N_STEPS + 1, H, W), "mask_alt": (2, N_STEPS + 1, H, W),
        "u8": (2, H, W, 1), "enc": (2, 1, 12), "enc_alt": (2, 1, 12), "neg": (2, 1, 12), "neg_alt": (2, 1, 12),
        "known": image, "known_alt": image, "known_noise": image, "known_noise_alt": image, "keep": (2, H, W), "keep_alt": (2, H, W)})
    rig.models = (mine, other)                       # the handles' owners
    rig.on_both(lambda h: N.lib().adm_unet_set_encoding(h, N.ptr(rig.t["enc"]), 1))
    mine.scheduler.set_timesteps(N_STEPS + 1)
    rig.rows = mine.scheduler.coef_rows()
    assert all(r["k_noise"] != 0.0 for r in rig.rows[:N_STEPS])
    t = rig.t
    P = dict(x=t["x"], B=1, coef_host=_coef(rig.rows), n_steps=N_STEPS, step_noise=t["noise"], mask=t["mask"], mask_start=1, mask_end=1,
             u8_out=t["u8"], max_value=1.0, guidance_scale=1.0)
    return rig, P


def _known_coef(scale=1.0):
    return (C.c_float * (2 * (N_STEPS + 1)))(*[scale * v for v in (0.9, 0.4, 0.95, 0.3, 1.0, 0.0)])


def _inpainting(rig, P):
    t = rig.t
    return dict(P, mask=None, mask_start=0, mask_end=0, keep=t["keep"], known=t["known"], known_noise=t["known_noise"],
                known_coef_host=_known_coef())


@pytest.mark.parametrize("backend", BACKENDS)
def test_data_behind_the_same_addresses_replays(backend):
    from audiodiffusion import _native as N
    dev = select(backend)
    assert N.lib().adm_version() >= 122 and N.lib().adm_unet_loop_captures(None) == 0
    rig, P = _conditional(dev)
    assert N.lib().adm_unet_loop_captures(rig.h) == 0
    assert rig.call(P) == 1                                               # the first call
    assert rig.call(P) == 0                                               # the same arguments again
    rig.contents(1)                                                       # new x, noise, mask (and encoding) at the same addresses ...
    other_rows = [dict(r, k_noise=0.5 * r["k_noise"], k_eps=0.75 * r["k_eps"]) for r in rig.rows]
    assert rig.call(dict(P, coef_host=_coef(other_rows))) == 0            # ... and new values in coef_host
    device_noise = dict(P, step_noise=None, noise_source=1, seed=0x1234_5678_9ABC_DEF0, row_offset=5)
    assert rig.call(device_noise) == 1
    assert rig.call(dict(device_noise, seed=77, row_offset=0)) == 0       # the seed and the row offset are data in the handle's block
    K = _inpainting(rig, device_noise)
    assert rig.call(K) == 1
    rig.contents(2)                                                       # new keep, known and known_noise at the same addresses ...
    assert rig.call(dict(K, known_coef_host=_known_coef(0.5))) == 0       # ... and new values in known_coef_host
    assert N.lib().adm_unet_loop_captures(rig.h) == 3


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_field_of_a_feature_that_is_off_is_not_in_the_key(backend):
    dev = select(backend)
    rig, P = _conditional(dev)
    t = rig.t
    khist = (C.c_float * N_STEPS)(0.0, 0.5)
    assert rig.call(dict(P, mode=MULTISTEP, k_hist_host=khist)) == 1       # (the handle has a k_hist table from here on)
    assert rig.call(P) == 1
    ignored = [dict(lo=5), dict(hi=7), dict(w=0.5), dict(max_value=3.0),                        # mode 0: no selection
               dict(guidance_scale=7.0),                                                        # encoding_uncond NULL
               dict(window_stride=8, window_wrap=1),                                            # window_total_w 0
               dict(known=t["known"], known_noise=t["known_noise"], known_coef_host=_known_coef(), known_batched=1, keep_batched=1),   # keep NULL
               dict(k_hist_host=khist)]                                                         # mode 0: not the multistep step
    assert [change for change in ignored if rig.call({**P, **change}) != 0] == []
    assert rig.call(P) == 0


def _keyed(rig, P):
    """group -> (the loop the handle holds, the changes that each make it another step)."""
    from audiodiffusion import _native as N
    from audiodiffusion import ops
    t = rig.t
    lo, hi, w = ops.threshold_ranks(H * W, 0.9)
    khist = (C.c_float * N_STEPS)(0.0, 0.5)
    # (c_x, c_m1, c_m2, c_t, p_m1): row 0 starts a run and reads no state; row 1 reads `last` and m_0, and no m_(-1): c_m2 == 0
    unipc = (N.SchedUnipcCoef * N_STEPS)(N.SchedUnipcCoef(1.0, 0.0, 0.0, 0.0, 0.0), N.SchedUnipcCoef(0.9, 0.2, 0.0, 0.05, 0.1))
    T = dict(P, mode=THRESH, lo=lo, hi=hi, w=w, max_value=4.0)
    return {
        "tensors": (P, [dict(x=t["x_alt"]), dict(step_noise=t["noise_alt"]), dict(step_noise=None), dict(mask=t["mask_alt"]),
                        dict(mask_start=0), dict(u8_out=None)]),
        "scalars": (P, [dict(n_steps=N_STEPS + 1), dict(prediction=2), T, dict(mode=MULTISTEP, k_hist_host=khist), dict(B=2)]),
        "thresholded": (T, [dict(lo=lo - 2, hi=hi - 2), dict(w=0.125 if w != 0.125 else 0.25), dict(max_value=3.0)]),
        "unipc": (dict(P, step_noise=None), [dict(unipc_host=unipc)]),                          # (the UniPC step has no noise rows)
        "guided": (dict(P, encoding_uncond=t["neg"], guidance_scale=2.5),
                   [dict(encoding_uncond=None), dict(encoding_uncond=t["neg_alt"]), dict(guidance_scale=3.0)]),
        "inpainting": (_inpainting(rig, P), [dict(keep=None), dict(keep=t["keep_alt"]), dict(known=t["known_alt"]),
                                             dict(known_noise=t["known_noise_alt"]), dict(known_batched=1), dict(keep_batched=1)]),
    }


@pytest.mark.parametrize("group", ["tensors", "scalars", "thresholded", "unipc", "guided", "inpainting"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_every_keyed_field_captures_and_captures_again_on_the_way_back(backend, group):
    dev = select(backend)
    rig, P = _conditional(dev)
    base, changes = _keyed(rig, P)[group]
    assert rig.call(base) == 1
    rig.there_and_back(base, changes)
    if group == "guided":
        for phi in (0.5, 0.7, 0.0):                                       # guidance_rescale 0 -> 0.5 -> 0.7, and back to 0
            assert rig.call(dict(base, guidance_rescale=phi)) == 1, phi
    assert rig.call(base) == 0


@pytest.mark.parametrize("backend", BACKENDS)
def test_what_the_handle_holds_is_in_the_key(backend):
    """The encoding set on the handle, its plan, and the stream: the arguments are the same in every call."""
    from audiodiffusion import _native as N
    dev = select(backend)
    rig, P = _conditional(dev)
    t, lib = rig.t, N.lib()
    assert rig.call(P) == 1
    for enc in ("enc_alt", "enc"):
        rig.on_both(lambda h: lib.adm_unet_set_encoding(h, N.ptr(t[enc]), 1))
        assert rig.call(P) == 1, enc
    for value in (1, 0):                                                  # a per-model option: the plan is dropped, and the step with it
        rig.on_both(lambda h: lib.adm_unet_set_option(h, b"single_sample", value))
        assert rig.call(P) == 1, value
    assert rig.call(P) == 0
    if dev.type == "cuda":                                                # the stream the step was captured on
        second = torch.cuda.Stream()
        with torch.cuda.stream(second):
            assert rig.call(P, use_graph=0) == 0                          # (a stream's split-K scratch cannot grow inside a capture: its
            assert rig.call(P) == 1                                       #  first loop is an eager one)
        assert rig.call(P) == 1
        assert rig.call(P) == 0
        N.check(lib.adm_release_stream(second.cuda_stream))               # no graph of this handle holds the stream's scratch any more


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_window_fields_are_keyed_when_windows_are_on(backend):
    from audiodiffusion import UNet2DModel
    dev = select(backend)
    torch.manual_seed(0)
    weights = td.OracleUNet(**td.TINY).state_dict()
    models = [UNet2DModel(**td.TINY).load_state_dict(weights) for _ in range(2)]
    rig = _Rig(dev, models[0]._ensure_handle(), models[1]._ensure_handle(),
               {"x": (1, 1, H, WIDE), "noise": (N_STEPS, 1, 1, H, WIDE), "u8": (1, H, WIDE, 1)})
    rows = [dict(tg.ROWS[i], timestep=float(t)) for i, t in ((0, 500), (1, 10))]
    assert all(r["k_noise"] != 0.0 for r in rows)
    t = rig.t
    P = dict(x=t["x"], B=1, coef_host=_coef(rows), n_steps=N_STEPS, step_noise=t["noise"], u8_out=t["u8"], max_value=1.0, guidance_scale=1.0)
    Wd = dict(P, window_total_w=WIDE, window_stride=W)                    # two disjoint windows
    assert rig.call(P) == 1                                               # the ordinary loop on the first 16 columns' worth of x
    rig.there_and_back(P, [Wd])
    assert rig.call(Wd) == 1 and rig.call(Wd) == 0
    rig.there_and_back(Wd, [dict(window_stride=8),                        # three windows: another plan as well
                            dict(window_wrap=1)])                         # two windows either way: the same plan, another step


@pytest.mark.parametrize("backend", BACKENDS)
def test_an_eager_loop_between_two_captured_ones_leaves_the_step_alone(backend):
    dev = select(backend)
    rig, P = _conditional(dev)
    assert rig.call(P) == 1
    assert rig.call(dict(P, prediction=2), use_graph=0) == 0              # another loop altogether, run eagerly on the same handle
    assert rig.call(P, use_graph=0) == 0
    assert rig.call(P) == 0
