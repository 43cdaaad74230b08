"""The long-form procedures on top of the generalised DDIM inversion (tests/test_inversion.py has the step, the loop and `encode`):
`longform.interpolate` with an encoding and with images wider than the model, and `longform.invert_audio` -- on the emulator and, under
`-m gpu`, on the MI355X."""
import numpy as np
import pytest
import torch

import test_guidance as tg
import test_inversion as ti
from native_backend import BACKENDS, select


def _spy_encode_loop(monkeypatch):
    """-> a list that gains, per `adm_encode_loop_ex` call, the fields of the adm_sample_loop_args it received."""
    from audiodiffusion import _native
    real, calls = _native.lib(), []

    def record(handle, args, stream):
        calls.append({name: getattr(args, name) for name, _ in args._fields_ if name.startswith(("B", "n_steps", "window_", "prediction"))})
        return real.adm_encode_loop_ex(handle, args, stream)

    class Spy:
        def __getattr__(self, name):
            return record if name == "adm_encode_loop_ex" else getattr(real, name)
    monkeypatch.setattr(_native, "lib", lambda: Spy())
    return calls


@pytest.mark.parametrize("backend", BACKENDS)
def test_interpolate_with_an_encoding(backend, monkeypatch):
    dev = select(backend)
    from audiodiffusion.longform import interpolate
    _, mine = tg._build("ddim")
    mine.to(dev)
    a, b = ti._images(2, 16, 16, 1)
    enc = ti._randn((1, 1, 12), 2).to(dev)
    calls = _spy_encode_loop(monkeypatch)
    alphas = [0.0, 0.5, 1.0]
    images, (sr, audios) = interpolate(mine, a, b, alphas, steps=3, encode_steps=3, audio=False, level="matched", encoding=enc)
    assert len(images) == len(alphas) and all(i.size == (16, 16) for i in images)
    assert len(calls) == 1 and calls[0]["B"] == 2 and calls[0]["window_total_w"] == 0
    # the encoding reaches the inversions and the sampling: another encoding gives other images
    other, _ = interpolate(mine, a, b, alphas, steps=3, encode_steps=3, audio=False, level="matched", encoding=-enc)
    assert any(np.asarray(x).tolist() != np.asarray(y).tolist() for x, y in zip(images, other))
    with pytest.raises(ValueError, match="encoding"):
        interpolate(mine, a, b, alphas, steps=3, encode_steps=3, audio=False)
    with pytest.raises(ValueError, match="ONE encoding"):
        interpolate(mine, a, b, alphas, steps=3, encode_steps=3, audio=False, encoding=ti._randn((2, 1, 12), 3).to(dev))


@pytest.mark.parametrize("circular", [False, True], ids=["open", "circular"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_interpolate_between_wide_images(backend, circular, monkeypatch):
    dev = select(backend)
    from audiodiffusion.longform import interpolate
    _, mine = ti._tiny("v_prediction")
    mine.to(dev)
    a, b = ti._images(2, 16, 32, 4)
    calls = _spy_encode_loop(monkeypatch)
    alphas = [0.25, 0.75]
    images, (sr, audios) = interpolate(mine, a, b, alphas, steps=2, encode_steps=2, audio=False, level="matched", window_stride=8,
                                          circular=circular)
    assert len(images) == len(alphas) and all(i.size == (32, 16) for i in images)
    assert len(calls) == 1 and (calls[0]["window_total_w"], calls[0]["window_stride"], calls[0]["window_wrap"]) == (32, 8, int(circular))
    assert calls[0]["prediction"] == 2 and tuple(mine.unet._hw()) == (16, 16)


@pytest.mark.parametrize("backend", BACKENDS)
def test_invert_audio_of_a_two_slice_clip_is_one_windowed_call(backend, monkeypatch):
    dev = select(backend)
    from audiodiffusion.longform import invert_audio
    _, mine = ti._tiny()
    mine.to(dev)
    rng = np.random.default_rng(0)
    clip = (0.2 * rng.standard_normal(2 * 16 * 64)).astype(np.float32)        # two slices of x_res * hop_length samples
    calls = _spy_encode_loop(monkeypatch)
    noise, image = invert_audio(mine, clip, steps=2, level="matched")
    assert image.size == (32, 16) and tuple(noise.shape) == (1, 1, 16, 32) and bool(torch.isfinite(noise).all())
    assert len(calls) == 1 and (calls[0]["B"], calls[0]["window_total_w"], calls[0]["window_stride"]) == (1, 32, 8)
    assert mine.mel.x_res == 16, "the pipeline's own Mel is not touched"
    noise1, image1 = invert_audio(mine, clip[:16 * 64], steps=2)                  # one slice: the model's width, the ordinary loop
    assert image1.size == (16, 16) and tuple(noise1.shape) == (1, 1, 16, 16)
    assert len(calls) == 2 and calls[1]["window_total_w"] == 0
