"""Long-form and interpolation procedures of `notebooks/test_model.ipynb`, as library calls on the native pipeline.

The reference has these only as notebook cells that call `AudioDiffusion` once per clip; here each is one function whose
heavy parts are batched on the device:

* `interpolate`    — cells 32-37 / 41-46: DDIM-invert two spectrograms (ONE batched `encode`), spherical interpolation for a
                     whole grid of weights (`ops.slerp_grid`, one launch pair), ONE batched sampling of all of them.
* `invert_audio`   — not in the notebook: audio -> the noise behind it (`encode`), a clip longer than one slice in ONE windowed call.
* `outpaint`       — cell 16: extend a clip segment by segment; every new segment is generated with its first
                     `overlap_secs` pinned to the tail of the previous one (`mask_start_secs`): the per-step mask overwrite
                     is part of the captured denoising graph (csrc/k_sched.hip `sched_step_kernel`, every instantiation), not a Python loop.
* `generate_long`  — not in the notebook: a clip longer than the model, or a seamless loop, sampled JOINTLY through overlapping
                     windows in one batched pipeline call (`frames` / `window_stride` / `circular`), where `outpaint` is causal and
                     runs the whole pipeline once per segment.
* `inpaint`        — not in the notebook: regenerate given time spans of a clip and keep the rest of its spectrogram exactly
                     (`keep_mask`: the known region is re-noised inside the step kernel, include/adm.h "Region in-painting").
* `continue_track` — not in the notebook: the one-call counterpart of `outpaint`: ONE windowed call over a wide sample whose
                     first columns are pinned to the input.
* `remix_track`    — cell 20: re-generate a whole track in overlapping slices from `start_step`, re-inserting (peak-
                     normalised) the tail of what was generated into the head of the next slice.

Extra keyword hooks (`noise`, `step_noise`, `init_phases`) exist so that the parity tests can feed the oracle pipeline and
this one identical draws; with their defaults the functions behave as the notebook cells do.
"""
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import ops


def slerp_grid(x0: torch.Tensor, x1: torch.Tensor, alphas: Sequence[float]) -> torch.Tensor:
    """`AudioDiffusionPipeline.slerp(x0, x1, alpha)` (`pipeline_audio_diffusion.py:244-258`) for every alpha at once:
    (len(alphas),) + x0.shape."""
    return ops.slerp_grid(x0, x1, alphas)


@torch.no_grad()
def interpolate(pipe, image_a: Image.Image, image_b: Image.Image, alphas: Sequence[float], steps: int = None,
                encode_steps: int = 50, generator: torch.Generator = None, audio: bool = True, init_phases=None, *,
                level: str = None, encoding: torch.Tensor = None, window_stride: int = None, circular: bool = False):
    """Returns (images, (sample_rate, audios)) with one entry per alpha (notebook cells 32-37). `level`, `encoding`, `window_stride`,
    `circular`: as `AudioDiffusionPipeline.encode`. The encoding ((1, S, D) or (S, D): one condition for the whole grid) serves both
    inversions and the sampling; images wider than the model are inverted and sampled through the windowed loop at one placement."""
    noise = pipe.encode([image_a, image_b], steps=encode_steps, level=level, encoding=encoding, window_stride=window_stride,
                        circular=circular)                                 # both inversions in one batched loop
    grid = slerp_grid(noise[0], noise[1], alphas)                          # (A, C, H, W)
    call = {}
    if encoding is not None:
        enc = encoding[None] if encoding.dim() == 2 else encoding
        if enc.shape[0] != 1:
            raise ValueError(f"interpolate takes ONE encoding, (1, S, D) or (S, D), for both images and every alpha, not {tuple(encoding.shape)}")
        call["encoding"] = enc.expand(len(alphas), -1, -1)
    if noise.shape[3] > pipe.unet._hw()[1]:   # wide: the sampler takes the same placement
        call.update(frames=int(noise.shape[3]), window_stride=window_stride, circular=circular)
    return pipe(batch_size=len(alphas), noise=grid, steps=steps, generator=generator, return_dict=False, audio=audio,
                init_phase=init_phases, **call)


@torch.no_grad()
def invert_audio(pipe, raw_audio: np.ndarray, **encode_kwargs):
    """DDIM-invert a clip: `raw_audio` becomes ONE spectrogram image and goes through `pipe.encode(**encode_kwargs)`. A clip of at most
    one slice gives the model-width image of the pipeline's own Mel; a longer one gives an image as wide as the clip (hop_length samples
    per column, rounded down to whole cells of 4 columns of the tensor being inverted), made by a Mel of the pipeline's config with
    x_res = that width (`_wide_mel`), so the whole clip inverts in ONE windowed call (`window_stride`, `circular` of `encode` place the
    windows and the width must fit them). Returns (the recovered noise, the image)."""
    mel = pipe.mel
    cell = 4 * _cell(pipe)
    cols = len(raw_audio) // mel.hop_length // cell * cell
    if cols > mel.x_res:
        mel = pipe._wide_mel(cols)
    mel.load_audio(raw_audio=raw_audio)
    image = mel.audio_slice_to_image(0)
    return pipe.encode([image], **encode_kwargs), image


def _one(pipe, **kw):
    images, (sr, audios) = pipe(batch_size=1, return_dict=False, **kw)
    return images[0], sr, audios[0]


@torch.no_grad()
def outpaint(pipe, raw_audio: np.ndarray, n_segments: int, overlap_secs: float, start_step: int = 0, steps: int = None,
             generator: torch.Generator = None, step_generator: torch.Generator = None, eta: float = 0,
             noise: Optional[List[torch.Tensor]] = None, step_noise=None, init_phases=None
             ) -> Tuple[np.ndarray, List[Image.Image]]:
    """Notebook cell 16. Returns (track, images): `raw_audio` followed by `n_segments` generated continuations."""
    sr = pipe.mel.get_sample_rate()
    ov = int(overlap_secs * sr)
    track, audio, images = raw_audio, raw_audio, []
    for i in range(n_segments):
        image, sr, audio2 = _one(pipe, raw_audio=audio[-ov:], start_step=start_step, steps=steps, generator=generator,
                                 step_generator=step_generator, eta=eta, mask_start_secs=overlap_secs,
                                 noise=None if noise is None else noise[i].clone(),
                                 step_noise=None if step_noise is None else step_noise[i],
                                 init_phase=None if init_phases is None else init_phases[i])
        images.append(image)
        track = np.concatenate([track, audio2[ov:]])
        audio = audio2
    return track, images


def _cell(pipe) -> int:
    """Image columns per column of the tensor the pipeline denoises: 1, or f = 2^(VAE blocks - 1) for a latent pipeline, whose `frames`,
    `window_stride` and `keep_mask` count latent cells."""
    return pipe._vae_factor() if getattr(pipe, "vqvae", None) is not None else 1


def long_placement(pipe, seconds: float, overlap_secs: float, circular: bool = False) -> Tuple[int, int]:
    """`seconds` of audio and `overlap_secs` of overlap between neighbouring windows, as the (frames, window_stride) of windowed sampling
    (include/adm.h "Windowed sampling") for this pipeline's model width W and Mel settings; one column is hop_length / sample_rate
    seconds. Rounded to the placement rules: the stride W - overlap to the nearest multiple of 4 in [4, W]; the number of windows up, so
    that the clip is at least `seconds` long (frames = W + k*stride open, k*stride >= W circular). With a `vqvae` both are in latent
    columns (f image columns each, so one is f * hop_length / sample_rate seconds) and W is the latent UNet's width."""
    cols_per_sec = pipe.mel.get_sample_rate() / pipe.mel.hop_length / _cell(pipe)
    W = pipe.unet._hw()[1]
    stride = int(round((W - overlap_secs * cols_per_sec) / 4)) * 4
    stride = min(max(stride, 4), W)
    want = max(int(np.ceil(seconds * cols_per_sec)), W)
    if circular:
        return -(-want // stride) * stride, stride
    return W + -(-(want - W) // stride) * stride, stride


@torch.no_grad()
def generate_long(pipe, seconds: float, overlap_secs: float, circular: bool = False, **call):
    """A clip of about `seconds`, longer than the model was trained on, sampled jointly through model-sized windows that overlap by about
    `overlap_secs` — ONE batched pipeline call (`frames`, `window_stride`, `circular` of `AudioDiffusionPipeline.__call__`) where
    `outpaint` runs the whole pipeline once per segment. `circular=True`: the spectrogram tiles with no seam (the Griffin-Lim phase
    does not). Returns (result of the pipeline call, dict(frames, window_stride, seconds, overlap_secs)): the values as rounded to the
    placement rules (`long_placement`), in columns and back in seconds. `call`: further keywords of the pipeline call."""
    frames, stride = long_placement(pipe, seconds, overlap_secs, circular)
    secs_per_col = _cell(pipe) * pipe.mel.hop_length / pipe.mel.get_sample_rate()
    used = dict(frames=frames, window_stride=stride, seconds=frames * secs_per_col,
                overlap_secs=(pipe.unet._hw()[1] - stride) * secs_per_col)
    return pipe(frames=frames, window_stride=stride, circular=circular, **call), used


def span_keep_mask(pipe, spans_secs: Sequence[Tuple[float, float]], width: int = None) -> np.ndarray:
    """The (H, W) uint8 keep mask that regenerates the time spans `spans_secs` [(from, to), ...] and keeps everything else: seconds
    become columns by the pipeline's own rule for `mask_start_secs` (pixels_per_second = W * sample_rate / x_res / hop_length,
    truncated), each span covering columns [int(from * pps), int(to * pps)). `width`: the mask's width (default: the model's W).
    With a `vqvae` the mask has the latent's resolution (`width` in latent columns): the spans are laid out in image columns as above
    (f per latent column) and a latent column is kept only if all f image columns under it are kept."""
    H, W = pipe.unet._hw()
    f = _cell(pipe)
    pps = f * W * pipe.mel.get_sample_rate() / pipe.mel.x_res / pipe.mel.hop_length
    keep = np.ones((H, f * (W if width is None else int(width))), dtype=np.uint8)
    for a, b in spans_secs:
        if not 0 <= a <= b:
            raise ValueError(f"spans_secs: a span is (from, to) with 0 <= from <= to, not {(a, b)}")
        keep[:, int(a * pps):int(b * pps)] = 0
    return keep if f == 1 else np.ascontiguousarray(keep.reshape(H, -1, f).min(axis=2))


@torch.no_grad()
def inpaint(pipe, raw_audio: np.ndarray, spans_secs: Sequence[Tuple[float, float]], **call):
    """Regenerate the time spans `spans_secs` [(from, to), ...] of one slice of `raw_audio` and keep the rest of its spectrogram
    exactly (`keep_mask` of `AudioDiffusionPipeline.__call__` with the default `known_level="previous"`): ONE pipeline call, the
    known region re-noised inside the step kernel. Returns (result of the pipeline call, the (H, W) keep mask). `call`: further
    keywords of the pipeline call (`slice`, `steps`, `batch_size`, `noise`, ...)."""
    keep = span_keep_mask(pipe, spans_secs)
    return pipe(raw_audio=raw_audio, keep_mask=keep, **call), keep


@torch.no_grad()
def continue_track(pipe, raw_audio: np.ndarray, seconds: float, overlap_secs: float, **call):
    """Continue `raw_audio` to a clip of about `seconds` in ONE windowed pipeline call: the wide sample of `long_placement(pipe,
    seconds, overlap_secs)` is denoised jointly through overlapping windows, the columns the input covers (hop_length samples each, from
    column 0; with a `vqvae` f * hop_length samples per latent column, and only columns the input covers whole) are kept and the rest is
    generated. The one-call counterpart of `outpaint`, which runs the whole pipeline once per
    segment at batch 1. Returns (result of the pipeline call, dict(frames, window_stride, kept_columns, seconds)). `call`: further
    keywords of the pipeline call."""
    frames, stride = long_placement(pipe, seconds, overlap_secs)
    kept = min(frames, int(len(raw_audio) / (_cell(pipe) * pipe.mel.hop_length)))
    keep = np.zeros((pipe.unet._hw()[0], frames), dtype=np.uint8)
    keep[:, :kept] = 1
    used = dict(frames=frames, window_stride=stride, kept_columns=kept,
                seconds=frames * _cell(pipe) * pipe.mel.hop_length / pipe.mel.get_sample_rate())
    return pipe(raw_audio=raw_audio, keep_mask=keep, frames=frames, window_stride=stride, **call), used


@torch.no_grad()
def remix_track(pipe, track_audio: np.ndarray, overlap_secs: float, start_step: int, seed: int = None, steps: int = None,
                eta: float = 0, noise: Optional[torch.Tensor] = None, step_noise=None, init_phases=None
                ) -> Tuple[np.ndarray, List[Image.Image]]:
    """Notebook cell 20. The generator is re-seeded to the same seed before every slice, as the cell does (`noise` overrides
    the draw: the same tensor for every slice). Returns (track, images)."""
    mel = pipe.mel
    sr = mel.get_sample_rate()
    ov = int(overlap_secs * sr)
    slice_size = mel.x_res * mel.hop_length
    stride = slice_size - ov
    generator = torch.Generator(device=pipe.device)
    seed = generator.seed() if seed is None else seed
    track, images, audio2, not_first = np.array([]), [], None, 0
    for sample in range(len(track_audio) // stride):
        generator.manual_seed(seed)
        audio = np.array(track_audio[sample * stride:sample * stride + slice_size])
        if not_first:
            # Normalize and re-insert generated audio
            audio[:ov] = audio2[-ov:] * np.max(audio[:ov]) / np.max(audio2[-ov:])
        image, sr, audio2 = _one(pipe, raw_audio=audio, start_step=start_step, steps=steps, generator=generator, eta=eta,
                                 mask_start_secs=overlap_secs * not_first,
                                 noise=None if noise is None else noise.clone(),
                                 step_noise=step_noise,
                                 init_phase=None if init_phases is None else init_phases[sample])
        images.append(image)
        track = np.concatenate([track, audio2[ov * not_first:]])
        not_first = 1
    return track, images
