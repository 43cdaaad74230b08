"""AudioDiffusionPipeline drop-in (`audiodiffusion/pipeline_audio_diffusion.py:39-258` of the reference).

Same constructor, `__call__` signature/defaults (`:72-87`), `encode` (`:208`), `slerp` (`:244`),
`get_default_steps` (`:63`) and return types. The denoising loop (`:159-185`), the scheduler step, the mask
overwrite and the uint8 dequantisation (`:192-194`) run as ONE native call (`adm_sample_loop_ex`: a captured
hipGraph of {UNet forward, fused scheduler epilogue} replayed per step, csrc/unet_exec.hip); the audio codec
runs in the Mel HIP kernels. `diffusers` is not required: a minimal `DiffusionPipeline`-compatible base
(`from_pretrained / save_pretrained / to / device / progress_bar / register_modules`) reads and writes the
diffusers on-disk layout (`model_index.json`, `unet/`, `scheduler/`, `mel/`).

Kept VERBATIM from the reference (GPL-3.0, see NOTICE.md at the repository root), because a drop-in must keep their quirks
bit for bit and `tests/test_reference_pin.py` pins them against the reference's own program text: the `__call__` signature
(`:72-87`), the audio-conditioned prologue (`:134-156`: slice -> image -> [-1, 1] tensor, the `images[0, 0] = add_noise(...)`
write-through into the aliased `noise`, the `(B, steps, H, W)` mask) and the image -> tensor lines of `encode` (`:221-226`).
Everything else in this file — the base class, the native loop call, dequantisation, batched image -> audio — is original.
"""
import ctypes as C
import json
import os
from math import acos, sin
from typing import List, Tuple, Union

import numpy as np
import torch
from PIL import Image

from . import _native as N
from . import ops
from .mel import Mel
from .schedulers import DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler, UniPCMultistepScheduler, randn_tensor
from .unet import UNet2DConditionModel, UNet2DModel
from .vae import AutoencoderKL


class PipelineOutput(dict):
    """BaseOutput-like: attribute and key access to `audios` / `images`."""
    __getattr__ = dict.__getitem__


_CLASSES = {"AutoencoderKL": AutoencoderKL, "UNet2DModel": UNet2DModel, "UNet2DConditionModel": UNet2DConditionModel,
            "DDIMScheduler": DDIMScheduler, "DDPMScheduler": DDPMScheduler,
            "DPMSolverMultistepScheduler": DPMSolverMultistepScheduler, "UniPCMultistepScheduler": UniPCMultistepScheduler, "Mel": Mel}


class DiffusionPipeline:
    """The subset of diffusers.DiffusionPipeline the reference relies on (`__init__.py:30-32`, `train_unet.py:303`)."""
    config_name = "model_index.json"
    _optional_components: List[str] = []

    def __init__(self):
        self._modules = {}
        self._progress_bar_config = {}
        self._device = N.default_device()

    def __setattr__(self, name, value):
        if name in self.__dict__.get("_modules", ()):   # `pipe.scheduler = other`: the registered component follows (save_pretrained)
            self._modules[name] = value
        super().__setattr__(name, value)

    def register_modules(self, **kwargs):
        for k, v in kwargs.items():
            self._modules[k] = v
            setattr(self, k, v)

    @property
    def device(self):
        return self._device

    def to(self, device=None, *a, **k):
        if device is not None:
            d = torch.device(device)
            if d.type == "cuda" and d.index is None:
                d = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
            if N.is_device_build() and d.type != "cuda":
                raise RuntimeError("this pipeline runs on the MI355X only (HIP kernels, no CPU path)")
            self._device = d
        return self

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    def progress_bar(self, iterable=None, total=None):
        cfg = dict(self._progress_bar_config)
        if cfg.get("disable"):
            return iterable
        try:
            from tqdm.auto import tqdm
            return tqdm(iterable, total=total, **cfg)
        except Exception:
            return iterable

    @classmethod
    def from_pretrained(cls, path, **kwargs):
        if not os.path.isdir(path):
            raise EnvironmentError(f"{path} is not a local directory (there is no hub access; pass a diffusers-layout directory)")
        with open(os.path.join(path, cls.config_name)) as f:
            index = json.load(f)
        comps = {}
        for name, spec in index.items():
            if name.startswith("_"):
                continue
            lib, klass = spec
            if klass is None:
                comps[name] = None
                continue
            if klass not in _CLASSES:
                raise NotImplementedError(f"component {name}: class {klass} is not implemented on this path")
            comps[name] = _CLASSES[klass].from_pretrained(path, subfolder=name)
        for opt in cls._optional_components:
            comps.setdefault(opt, None)
        return cls(**comps)

    def save_pretrained(self, path, safe_serialization=True):
        os.makedirs(path, exist_ok=True)
        index = {"_class_name": type(self).__name__, "_diffusers_version": "0.24.0"}
        for name, m in self._modules.items():
            if m is None:
                index[name] = [None, None]
                continue
            lib = "audio_diffusion" if isinstance(m, Mel) else "diffusers"
            index[name] = [lib, type(m).__name__]
            sub = os.path.join(path, name)
            if isinstance(m, (UNet2DModel, AutoencoderKL)):
                m.save_pretrained(sub, safe_serialization=safe_serialization)
            else:
                m.save_pretrained(sub)
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(index, f, indent=2, sort_keys=True)


class AudioDiffusionPipeline(DiffusionPipeline):
    """
    Parameters (as the reference, `pipeline_audio_diffusion.py:39-61`):
        vqvae: AutoencoderKL for latent audio diffusion or None
        unet: UNet2DModel
        mel: Mel — transform audio <-> spectrogram
        scheduler: DDIMScheduler, DDPMScheduler, DPMSolverMultistepScheduler or UniPCMultistepScheduler
    """

    _optional_components = ["vqvae"]
    # per-call step-noise staging is bounded: the loop runs in chunks of this many steps
    _STEP_CHUNK = 100

    def __init__(self, vqvae, unet, mel, scheduler):
        super().__init__()
        self.register_modules(unet=unet, scheduler=scheduler, mel=mel, vqvae=vqvae)

    def get_default_steps(self) -> int:
        if isinstance(self.scheduler, (DPMSolverMultistepScheduler, UniPCMultistepScheduler)):
            return 20   # (the reference's rule would say 1000: pointless for a solver built for few steps)
        return 50 if isinstance(self.scheduler, DDIMScheduler) else 1000

    # ---- the native denoising loop (pipeline_audio_diffusion.py:159-185 + :192-194) ----------------------
    def _guided(self, guidance_scale, negative_encoding, encoding):
        """The rules of classifier-free guidance (`__call__`): True when the guided loop is to run."""
        if guidance_scale is not None and not np.isfinite(float(guidance_scale)):   # (before the rule below: nan > 1 is False)
            raise ValueError(f"guidance_scale={guidance_scale!r} must be finite")
        on = guidance_scale is not None and float(guidance_scale) > 1.0   # diffusers' rule: <= 1 is today's path, exactly
        if not on:
            if negative_encoding is not None:
                raise ValueError("negative_encoding is only used by classifier-free guidance: pass guidance_scale > 1 with it")
            return False
        if not isinstance(self.unet, UNet2DConditionModel):
            raise ValueError("guidance_scale > 1 needs a conditional model: this pipeline's unet is not a UNet2DConditionModel")
        if encoding is None:
            raise ValueError("guidance_scale > 1 needs an `encoding` to guide towards: none was given")
        return True

    @staticmethod
    def _negative_encoding(negative_encoding, enc, keep=None):
        """The unconditional branch's encoding, of the shape of `enc` (B, seq, dim): zeros by default, a leading 1 broadcasts.
        keep: the buffer this method made for an earlier guided call (never a caller's tensor). Its address is part of the captured graph's key, so where a new tensor would have
        to be made (zeros, a broadcast, a conversion) `keep` is refilled in place when shape and device still fit: consecutive calls
        then replay the captured graph instead of capturing again. A caller's own contiguous fp32 tensor is used as it is.
        -> (the encoding to use, the buffer to keep for the next call)"""
        fits = keep is not None and keep.shape == enc.shape and keep.device == enc.device and keep.dtype == torch.float32
        if negative_encoding is None:
            buf = keep.zero_() if fits else torch.zeros_like(enc)
            return buf, buf
        neg = negative_encoding.to(enc.device, torch.float32)
        if neg.dim() == 2:
            neg = neg[:, None, :]
        if neg.dim() == 3 and neg.shape[0] == 1 and tuple(neg.shape[1:]) == tuple(enc.shape[1:]):
            neg = neg.expand(enc.shape[0], -1, -1)
        if tuple(neg.shape) != tuple(enc.shape):
            raise ValueError(f"negative_encoding shape {tuple(negative_encoding.shape)} does not match the encoding's {tuple(enc.shape)} "
                             f"(a leading 1 is broadcast over the batch)")
        if neg is negative_encoding and neg.is_contiguous():
            return neg, keep
        buf = keep.copy_(neg) if fits else neg.contiguous().clone()
        return buf, buf

    @staticmethod
    def _device_noise(device_noise_seed, **excluded):
        """The rule of `device_noise_seed` (`__call__`): it replaces every other source of noise, so none may be given with it."""
        if device_noise_seed is None:
            return
        ops._seed64(device_noise_seed, "device_noise_seed")
        for name, given in excluded.items():
            if given is not None:
                raise ValueError(f"device_noise_seed draws the noise on the device from its own stream: it cannot be combined with `{name}`")

    def _window(self, frames, window_stride, circular, **excluded):
        """The rules of windowed sampling (`__call__`), before any work. -> None (`frames` is None: today's path), or
        (frames, window_stride, circular, windows per sample)."""
        if frames is None:
            if window_stride is not None:
                raise ValueError("window_stride places the windows of a wide sample: it needs `frames`")
            if circular:
                raise ValueError("circular places the windows of a wide sample on a circle: it needs `frames`")
            return None
        for name, given in excluded.items():
            if given:
                raise ValueError(f"`{name}` cannot be combined with `frames`: windowed sampling starts from noise and has no mask "
                                 f"(the mask's layout assumes the model's width)")
        if self.vqvae is not None and not hasattr(self.vqvae, "decode_tiled"):
            raise NotImplementedError("`frames` with a `vqvae` that has no `decode_tiled` is not implemented: the decoder's mid-block "
                                      "attention would see another sequence length than the one it was trained on")
        W = self.unet._hw()[1]
        stride = W // 2 if window_stride is None else window_stride
        nW = ops.window_count(frames, W, stride, circular, names=("frames", "window_stride", "circular"))
        return int(frames), int(stride), bool(circular), nW

    KNOWN_LEVELS = ("previous", "current")

    def _keep_mask(self, keep_mask, known_level, known, shape, has_audio, mask_start_secs, mask_end_secs):
        """The rules of region in-painting (`__call__`), before any work and any native call. `shape`: the (B, C, H, W) of the tensor
        being denoised. -> None (`keep_mask` is None: today's path), or (keep (1 or B, H, W) uint8 on the device, `known` as a
        (1 or B, C, H, W) fp32 device tensor or None when the audio input is the source)."""
        if known_level not in self.KNOWN_LEVELS:
            raise ValueError(f"known_level={known_level!r} must be one of {self.KNOWN_LEVELS}")
        if keep_mask is None:
            if known is not None:
                raise ValueError("`known` is the image that `keep_mask` keeps: it needs `keep_mask`")
            return None
        if mask_start_secs or mask_end_secs:
            raise ValueError("`keep_mask` cannot be combined with `mask_start_secs` / `mask_end_secs`: put the edge columns into the mask")
        if known is None and not has_audio:
            raise ValueError("`keep_mask` needs a source for the region it keeps: `audio_file`, `raw_audio` or `known`")
        if known is not None and has_audio:
            raise ValueError("`keep_mask` takes ONE source for the region it keeps: `known`, or `audio_file` / `raw_audio`, not both")
        B, Cc, H, W = shape
        keep = torch.as_tensor(np.asarray(keep_mask) if not torch.is_tensor(keep_mask) else keep_mask)
        if keep.dim() == 2:
            keep = keep[None]
        if keep.dim() != 3 or tuple(keep.shape[1:]) != (H, W) or keep.shape[0] not in (1, B):
            raise ValueError(f"keep_mask shape {tuple(keep.shape)} is not (H, W), (1, H, W) or (B, H, W) with (B, H, W) = {(B, H, W)}: "
                             f"its resolution is that of the tensor being denoised")
        # (a contiguous uint8 tensor on the device is used as it is, so its address — part of the captured graph's key — stays the caller's:
        # new contents in the same buffer replay the graph; the kernel reads "non-zero", not "one")
        if not (keep.dtype == torch.uint8 and keep.device == torch.device(self.device) and keep.is_contiguous()):
            keep = (keep != 0).to(torch.uint8).to(self.device).contiguous()
        if known is not None:
            if not torch.is_tensor(known) or known.dim() != 4 or tuple(known.shape[1:]) != (Cc, H, W) or known.shape[0] not in (1, B):
                got = tuple(known.shape) if torch.is_tensor(known) else type(known).__name__
                raise ValueError(f"known shape {got} is not (1 or B, C, H, W) with (B, C, H, W) = {shape}: a float tensor in model space")
            known = known.to(self.device, torch.float32).contiguous()
        return keep, known

    def _known_coef(self, start_step, n, known_level):
        """(ka, kb) for the `n` loop rows from `start_step`: `add_noise`'s coefficients (`_sa_sb`) of the level the overwrite uses.
        "current": row i at timesteps[i], the level the sample had before the step (the reference's mask). "previous": row i at
        timesteps[i + 1], the level it has after the step, and the last row of the schedule (1, 0): the known image itself."""
        ts = self.scheduler.timesteps
        first = start_step + (1 if known_level == "previous" else 0)
        idx = ts[first:start_step + n + (1 if known_level == "previous" else 0)]
        sa, sb = self.scheduler._sa_sb(idx, "cpu") if len(idx) else (torch.zeros(0), torch.zeros(0))
        rows = [(float(a), float(b)) for a, b in zip(sa.tolist(), sb.tolist())]
        if len(rows) < n:   # "previous" on the last row of the schedule
            rows.append((1.0, 0.0))
        assert len(rows) == n
        return rows

    def _vae_factor(self):
        """Image pixels per latent cell along an axis (1 without a `vqvae`): `frames` counts cells of the tensor being denoised."""
        return 1 if self.vqvae is None else 2 ** (len(self.vqvae.config.block_out_channels) - 1)

    def _encode_known(self, input_images, window, generator):
        """The audio input's image (1, H, W) in [-1, 1] -> the scaled latent (Cz, h, w) of a `vqvae` pipeline. With windowed sampling the
        image is wide and goes through the tiled encoder at the sampler's own placement, in pixels."""
        x = torch.unsqueeze(input_images, 0)
        if window is None:
            dist = self.vqvae.encode(x).latent_dist
        else:
            f = self._vae_factor()
            dist = self.vqvae.encode_tiled(x, f * self.unet._hw()[1], f * window[1], window[2]).latent_dist
        return 0.18215 * dist.sample(generator=generator)[0]

    def _wide_mel(self, frames):
        """A Mel of the pipeline's Mel config with x_res = frames (the codec requires the image width to equal x_res): a separate object,
        kept for the next call at the same width; the pipeline's own Mel is not touched."""
        cfg = dict(self.mel.config, x_res=int(frames))
        kept = getattr(self, "_wide_mel_kept", None)
        if kept is None or kept[0] != cfg:
            kept = (cfg, Mel.from_config(cfg))
            self._wide_mel_kept = kept
        kept[1].nnls_max_iter = self.mel.nnls_max_iter
        return kept[1]

    def _denoise(self, images, start_step, eta, step_generator, mask, mask_start, mask_end, step_noise=None,
                 use_graph=True, want_u8=True, encoding=None, stop_step=None, guidance_scale=None, negative_encoding=None,
                 device_noise_seed=None, device_noise_row_offset=0, guidance_rescale=0.0, window_stride=None, circular=False,
                 keep_mask=None, known=None, known_noise=None, known_level="previous"):
        """The denoising loop (`:159-185`) as ONE native call per chunk of steps. `stop_step` (tests only) ends the loop
        before that step index, so that a single step of a long schedule can be compared in isolation.
        Every combination is one `adm_sample_loop_args` (include/adm.h) and one `adm_sample_loop_ex` call per chunk.
        guidance_scale > 1: every step is two forwards (the encoding, the negative encoding) and one guided step kernel, inside the
        same native call; otherwise one forward per step. guidance_rescale in (0, 1] (needs the guided loop): one statistics kernel more
        per step, and the step uses the rescaled guided output (include/adm.h "guidance rescale").
        device_noise_seed: the noise of every noisy row is drawn inside the step kernel ("adm noise stream 1", include/adm.h) at (seed,
        device_noise_row_offset + b, the row's timestep): ONE native call whatever the number of steps, no staging tensor, no chunks,
        no synchronisation. A schedule without noisy rows (DDIM with eta == 0, the multistep solver) has nothing to draw.
        window_stride (not None: windowed sampling, include/adm.h "Windowed sampling"): `images` is the WIDE sample (B, C, H, frames),
        wider than the model, which keeps its own width; every step gathers the windows, runs the model on all B*nW of them as one
        batch, blends the outputs and steps once on the wide sample, inside the same native call. `circular` places the windows on a
        circle. The encodings of sample b serve its nW windows.
        keep_mask (not None: region in-painting, include/adm.h "Region in-painting"): a (H, W), (1, H, W) or (B, H, W) 0/1 mask at the
        resolution of `images`; after every step the elements it marks are overwritten, inside the step kernel, with
        ka*known + kb*known_noise at the level `known_level` names (`_known_coef`). known: (1 or B, C, H, W) in model space; known_noise:
        (B, C, H, W), one fixed draw for all steps. No tensor has a step axis; with windowed sampling the three are wide."""
        sched, unet = self.scheduler, self.unet
        self._device_noise(device_noise_seed, step_generator=step_generator, step_noise=step_noise)
        guided = self._guided(guidance_scale, negative_encoding, encoding)
        rescaled = ops.guidance_rescale_on(guidance_rescale, guided)
        multistep = isinstance(sched, DPMSolverMultistepScheduler)
        unipc = isinstance(sched, UniPCMultistepScheduler)   # its own step kernel: every prediction type, thresholded or not
        thresh = None if multistep else sched.threshold()
        pred = 0 if multistep else sched.prediction   # the C-ABI's `prediction`; the multistep step is epsilon only
        # (a multistep or UniPC run that starts late starts first order: its rows depend on where it starts, not only on the slice)
        rows = sched.loop_rows(start_step, stop_step) if multistep or unipc else sched.coef_rows(eta)[start_step:stop_step]
        n = len(rows)
        x = images.contiguous().clone()  # the reference never writes the loop state back into `noise`
        B, Cc, H, W = x.shape
        nW = 1
        if window_stride is not None:   # the model keeps its own width: x is wide, the windows have the model's shape
            if mask is not None:
                raise ValueError("windowed sampling has no mask (the mask's layout assumes the model's width)")
            if unet._hw()[0] != H:
                raise ValueError(f"a wide sample has the model's height {unet._hw()[0]}, not {H}")
            nW = ops.window_count(W, unet._hw()[1], window_stride, circular, names=("frames", "window_stride", "circular"))
        elif tuple(unet._hw()) != (H, W):
            unet.sample_size = (H, W)
        h = unet._ensure_handle()
        if isinstance(unet, UNet2DConditionModel):     # `self.unet(images, t, encoding)` (:160-161): constant over the loop
            if nW > 1 and encoding is not None:        # sample-major windows: the encoding of sample b for each of its nW windows
                encoding = encoding.repeat_interleave(nW, dim=0)
                if negative_encoding is not None and negative_encoding.shape[0] == B:
                    negative_encoding = negative_encoding.repeat_interleave(nW, dim=0)
            unet._set_encoding(h, encoding, B * nW, x.device)
        if guided:
            # kept alive, and reused by the next call: the captured graph holds the pointer
            unet._enc_uncond, unet._enc_uncond_buf = self._negative_encoding(negative_encoding, unet._enc,
                                                                             getattr(unet, "_enc_uncond_buf", None))
        u8 = torch.empty((B, H, W, Cc), dtype=torch.uint8, device=x.device) if want_u8 else None
        if Cc != 1 and want_u8:
            u8 = None  # NHWC permute for multi-channel images is done after the loop
        kept = None
        if keep_mask is not None:
            if mask is not None:
                raise ValueError("`keep_mask` and the staged mask exclude each other")
            if known is None or known_noise is None:
                raise ValueError("`keep_mask` needs `known` and `known_noise`")
            checked = self._keep_mask(keep_mask, known_level, known, (B, Cc, H, W), False, 0, 0)
            kept = (checked[1], known_noise.to(x.device, torch.float32).contiguous(), checked[0], self._known_coef(start_step, n, known_level))
            if tuple(kept[1].shape) != (B, Cc, H, W):
                raise ValueError(f"known_noise shape {tuple(kept[1].shape)} is not that of the sample, {(B, Cc, H, W)}")
        needs_noise = [r["k_noise"] != 0.0 for r in rows]
        philox = device_noise_seed is not None and any(needs_noise)
        chunk = n if philox or not any(needs_noise) else min(n, self._STEP_CHUNK)
        stage = None
        done = 0
        while done < n:
            m = min(chunk, n - done)
            sub = rows[done:done + m]
            coef = (N.SchedCoef * m)(*[N.SchedCoef(*[float(r[k]) for k in
                                       ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise", "timestep")])
                                       for r in sub])
            noise_ptr = None
            if not philox and any(needs_noise[done:done + m]):
                if stage is None or stage.shape[0] != m:
                    stage = torch.empty((m, B, Cc, H, W), dtype=torch.float32, device=x.device)
                for i in range(m):
                    if needs_noise[done + i]:
                        if step_noise is not None:
                            stage[i].copy_(step_noise[done + i])
                        else:  # same draw order as scheduler.step's randn_tensor calls in the reference loop
                            stage[i].copy_(randn_tensor((B, Cc, H, W), step_generator, x.device, torch.float32))
                noise_ptr = N.ptr(stage)
            last = done + m == n
            mask_ptr = None
            if mask is not None:
                # (B, n_total, H, W): this chunk starts at row `done`; the kernel indexes mask[:, step_in_chunk]
                mask_chunk = mask[:, done:done + m].contiguous()
                mask_ptr = N.ptr(mask_chunk)
            u8_ptr = N.ptr(u8) if (last and u8 is not None) else None
            # one entry point for every combination; device noise, the multistep history and the UniPC state all need all steps in this one call
            assert m == n or not (philox or multistep or unipc)
            args = N.SampleLoopArgs(x=N.ptr(x), B=B, coef_host=coef, n_steps=m, step_noise=noise_ptr, mask=mask_ptr,
                                    mask_start=int(mask_start), mask_end=int(mask_end), u8_out=u8_ptr, use_graph=int(use_graph),
                                    prediction=pred, max_value=1.0, guidance_scale=1.0)
            if multistep:
                args.mode, args.k_hist_host = N.SCHED_MULTISTEP, (C.c_float * m)(*[float(r["k_hist"]) for r in sub])
            if unipc:
                args.unipc_host = (N.SchedUnipcCoef * m)(*[N.SchedUnipcCoef(*[float(r[k]) for k in ops.UNIPC_FIELDS]) for r in sub])
            if not multistep and thresh is not None:   # dynamic thresholding: the statistic is over this tensor's C*H*W (the latent's, with a VAE)
                args.mode, args.max_value = N.SCHED_THRESH, thresh[1]
                args.lo, args.hi, args.w = ops.threshold_ranks(Cc * H * W, thresh[0])
            if guided:   # two forwards per step, the second on this encoding
                args.encoding_uncond, args.guidance_scale = N.ptr(unet._enc_uncond), float(guidance_scale)
            if rescaled:
                args.guidance_rescale = float(guidance_rescale)
            if philox:   # noise drawn in the step kernel: no staging tensor
                args.noise_source, args.row_offset = 1, int(device_noise_row_offset)
                args.seed = ops._seed64(device_noise_seed, "device_noise_seed")
            if window_stride is not None:   # x, the noise and the u8 image are `W` wide; B counts wide samples
                args.window_total_w, args.window_stride, args.window_wrap = W, int(window_stride), int(bool(circular))
            if kept is not None:   # the known-region overwrite: three tensors of x's shape class and this chunk's (ka, kb) rows
                args.known, args.known_noise, args.keep = N.ptr(kept[0]), N.ptr(kept[1]), N.ptr(kept[2])
                args.known_coef_host = (C.c_float * (2 * m))(*[v for row in kept[3][done:done + m] for v in row])
                args.known_batched, args.keep_batched = int(kept[0].shape[0] != 1), int(kept[2].shape[0] != 1)
            N.check(N.lib().adm_sample_loop_ex(h, args, N.stream_for(x)))
            if x.is_cuda and (noise_ptr is not None or mask_ptr is not None) and not last:
                torch.cuda.current_stream(x.device).synchronize()  # staging buffers are rewritten next chunk
            done += m
        return x, u8

    @torch.no_grad()
    def __call__(
        self,
        batch_size: int = 1,
        audio_file: str = None,
        raw_audio: np.ndarray = None,
        slice: int = 0,
        start_step: int = 0,
        steps: int = None,
        generator: torch.Generator = None,
        mask_start_secs: float = 0,
        mask_end_secs: float = 0,
        step_generator: torch.Generator = None,
        eta: float = 0,
        noise: torch.Tensor = None,
        encoding: torch.Tensor = None,
        return_dict=True,
        step_noise=None,
        audio=True,
        return_float=False,
        init_phase=None,
        guidance_scale=None,
        negative_encoding=None,
        device_noise_seed: int = None,
        device_noise_row_offset: int = 0,
        guidance_rescale: float = 0.0,
        frames: int = None,
        window_stride: int = None,
        circular: bool = False,
        keep_mask=None,
        known_level: str = "previous",
        known: torch.Tensor = None,
    ) -> Union[PipelineOutput, Tuple[List[Image.Image], Tuple[int, List[np.ndarray]]]]:
        """Generate random mel spectrogram from audio input and convert to audio (reference docstring `:89-112`).

        Extra keyword-only knobs (not in the reference; defaults reproduce it): `step_noise` injects the
        per-step scheduler noise (parity tests), `audio=False` skips the image->audio conversion,
        `return_float=True` additionally returns the final float images, `init_phase` (B, n_bins, frames) replaces the
        unseeded Griffin-Lim start phase librosa draws (`mel.py:165-167`).

        Classifier-free guidance (Ho & Salimans 2022), off by default: `guidance_scale` g and `negative_encoding`.
          * g None or <= 1.0 takes the unguided path exactly: one forward per step and the unguided entry points (diffusers' rule;
            u + 1*(c - u) is not c in floating point, so 1.0 never goes through the guided kernel).
          * g > 1 needs a UNet2DConditionModel and an `encoding`; otherwise ValueError naming what is missing. Every step then runs the
            model on the encoding (c) and on the negative encoding (u) and steps with u + g*(c - u), all inside the captured loop.
          * `negative_encoding` None means zeros of the encoding's shape (what `train_unet.py --encoding_dropout` trains the model
            to read as "no condition"); otherwise it must have the encoding's shape, a leading 1 being broadcast over the batch.
          * a `negative_encoding` without g > 1 is a ValueError.
          * `guidance_rescale` phi (Lin et al. 2023 §3.4; diffusers' keyword): None or 0 is the guided path above, exactly. phi in (0, 1]
            pulls the per-sample standard deviation of the guided output back towards that of the conditional one before every step,
            o' = phi*(o*std(c)/std(o)) + (1 - phi)*o, computed on the device inside the captured loop (include/adm.h "guidance
            rescale"). It needs active guidance (g > 1, a conditional model, an encoding): otherwise ValueError naming guidance_scale.
            A value outside [0, 1] is a ValueError naming guidance_rescale.

        Device noise, off by default: `device_noise_seed` (an int in [0, 2^64)). All noise then comes from "adm noise stream 1"
        (include/adm.h): a counter-based generator evaluated on the device, a pure function of (seed, global sample row, timestep,
        element). The initial latent, unless `noise` is given, is `ops.randn(..., noise_stream=1)`; every noisy step (DDPM, DDIM with
        eta > 0) draws inside the fused step kernel, and the loop is one native call without a noise tensor. Sample b is global row
        `device_noise_row_offset` + b, so a sample's bits depend on neither its batch nor its shard. It is NOT torch.randn's stream: the
        same seed gives other images than a torch generator. With `generator`, `step_generator` or `step_noise` it is a ValueError; with
        the multistep and UniPC schedulers (no noisy steps) the seed only picks the initial latent.

        Windowed sampling, off by default: `frames`, `window_stride`, `circular` (include/adm.h "Windowed sampling"). `frames` = Wt asks
        for spectrograms Wt columns wide, wider than the model's W: every step cuts the wide sample into model-sized windows `window_stride`
        (default W // 2) apart, runs the model on the windows of all samples as one batch, averages the model outputs where windows
        overlap and makes one scheduler step on the wide sample, all inside the captured loop. `circular=True` places the windows on a
        circle: the time axis has no edge and the spectrogram tiles with no seam at any column.
          * `frames=None` is the path without it, exactly. frames, window_stride and W are multiples of 4, window_stride <= W <= frames;
            open: frames - W is a multiple of window_stride; circular: frames is. Otherwise ValueError naming the keyword.
          * `noise`, if given, is (batch_size, C, H, frames); device noise draws the initial latent at that shape. Everything per sample
            (thresholding, guidance rescale, the device-noise counter) is per wide sample. `encoding` rows serve all windows of a sample.
          * `window_stride` or `circular` without `frames`, and `audio_file`, `raw_audio`, `mask_start_secs` or `mask_end_secs` with it:
            ValueError.
          * with a `vqvae` (latent audio diffusion) `frames`, `window_stride` and `noise` are in units of the tensor being denoised,
            latent cells of f = 2^(VAE blocks - 1) pixels, as `keep_mask` is. The wide latent is decoded by `vqvae.decode_tiled` at the
            sampler's own placement (windows of the UNet's width, `window_stride`, `circular`): all windows as one decoder batch, joined
            in pixel space by a cross-fade whose weights fall off towards each window's edges (include/adm.h "Tiled codec"), so the
            decoder's global attention never sees a wide latent. A `vqvae` object without `decode_tiled`: NotImplementedError.
          * images come back `frames` wide (f*frames with a `vqvae`); audio is decoded through a separate Mel of this pipeline's Mel
            config with x_res = that width and is hop_length * (width - 1) samples long. The Griffin-Lim phase of a circular image is NOT
            made circular: the seamless object is the spectrogram.

        Region in-painting, off by default: `keep_mask`, `known_level`, `known` (include/adm.h "Region in-painting"). `keep_mask` is a
        bool or 0/1 tensor or array (H, W), (1, H, W) or (B, H, W) at the resolution of the tensor being denoised (image pixels; latent
        cells with a `vqvae`; `frames` wide with windowed sampling); non-zero means "this element stays the input's". Any region: a span
        in the middle of a clip, a frequency band, single pixels; any channel count (the mask is broadcast over the channels).
          * `keep_mask=None` is the path without it, exactly.
          * the known image comes from `audio_file` / `raw_audio` (+ `slice`), converted as for `mask_start_secs` (with a `vqvae`:
            encoded and scaled by 0.18215; with `frames`: through a Mel of this pipeline's config with x_res = the image width, and
            with both through `vqvae.encode_tiled` at the sampler's placement, ONE posterior draw at the wide shape), or from `known`,
            a float tensor (1 or B, C, H, W) already in model space ([-1, 1] images, or scaled latents). One of them is needed, not both.
          * after every step the kept elements are overwritten with ka*known + kb*noise INSIDE the step kernel: no (B, steps, H, W) mask
            tensor is built, nothing is staged per step, and the run is the same native call(s) as without the mask.
          * `known_level="previous"` (default): the overwrite uses the level the sample has AFTER the step (timesteps[i + 1]) and the last
            step uses (1, 0), so the kept region of the result is the input exactly. `"current"` is the reference's rule (the level of
            timesteps[i]): with edge columns it gives the images of `mask_start_secs` / `mask_end_secs` byte for byte, the noise of the
            last timestep included.
          * the noise is the initial latent, as in the reference: ONE fixed draw for all steps, not a fresh draw per step (copied before
            `start_step` writes into the latent; with `device_noise_seed` it is the latent that seed draws).
          * `start_step > 0`: every sample (not only [0, 0] as with `mask_start_secs`) starts from add_noise(known, noise,
            timesteps[start_step - 1]).
          * with `mask_start_secs` / `mask_end_secs`, without a source, with a mask or a `known` of another shape, or with another
            `known_level`: ValueError naming the keyword. `frames` with a `vqvae` that cannot decode tiles stays NotImplementedError."""
        ops.guidance_rescale_on(guidance_rescale, self._guided(guidance_scale, negative_encoding, encoding))   # the ValueErrors, before any work
        self._device_noise(device_noise_seed, generator=generator, step_generator=step_generator, step_noise=step_noise)
        # For backwards compatibility
        if type(self.unet.sample_size) == int:
            self.unet.sample_size = (self.unet.sample_size, self.unet.sample_size)
        has_audio = audio_file is not None or raw_audio is not None
        if known_level not in self.KNOWN_LEVELS:
            raise ValueError(f"known_level={known_level!r} must be one of {self.KNOWN_LEVELS}")
        if keep_mask is not None and (mask_start_secs or mask_end_secs):   # (before `frames` refuses the same two for its own reason)
            raise ValueError("`keep_mask` cannot be combined with `mask_start_secs` / `mask_end_secs`: put the edge columns into the mask")
        # (an audio input with `frames` is the known image of a keep mask; without one it stays refused)
        window = self._window(frames, window_stride, circular, audio_file=audio_file if keep_mask is None else None,
                              raw_audio=raw_audio is not None and keep_mask is None,
                              mask_start_secs=mask_start_secs, mask_end_secs=mask_end_secs)
        steps = steps or self.get_default_steps()
        self.scheduler.set_timesteps(steps)
        step_generator = step_generator or generator
        shape = (batch_size, self.unet.in_channels, self.unet.sample_size[0], self.unet.sample_size[1] if window is None else window[0])
        kept = self._keep_mask(keep_mask, known_level, known, shape, has_audio, mask_start_secs, mask_end_secs)
        if window is not None and noise is not None and tuple(noise.shape) != shape:
            raise ValueError(f"noise shape {tuple(noise.shape)} is not (batch_size, C, H, frames) = {shape}")
        if noise is None and device_noise_seed is not None:
            noise = ops.randn(shape, device_noise_seed, row_offset=device_noise_row_offset, t=0, noise_stream=1, device=self.device)
        if noise is None:
            # the reference's torch.randn(..., generator=generator, device=self.device) (:120-128); going through
            # randn_tensor additionally accepts a CPU generator on the GPU build (drawn on the host, then moved)
            noise = randn_tensor(shape, generator, self.device, torch.float32)
        images = noise
        mask = None
        mask_start = mask_end = 0

        known_noise = None
        if kept is not None:
            # region in-painting: the known image in model space, the latent copied as the ONE noise draw before anything writes into
            # it, and no (B, steps, H, W) mask: the step kernel forms add_noise(known, noise, level) where keep_mask says so
            known = kept[1]
            if known is None:
                mel = self.mel if window is None else self._wide_mel(self._vae_factor() * window[0])
                mel.load_audio(audio_file, raw_audio)
                input_image = mel.audio_slice_to_image(slice)
                input_image = np.frombuffer(input_image.tobytes(), dtype="uint8").reshape((input_image.height, input_image.width))
                input_image = (input_image / 255) * 2 - 1
                input_images = torch.tensor(input_image[np.newaxis, :, :], dtype=torch.float).to(self.device)
                if self.vqvae is not None:
                    input_images = self._encode_known(input_images, window, generator)
                known = input_images[None].contiguous()
                if tuple(known.shape[1:]) != shape[1:]:
                    raise ValueError(f"the audio input gives a known image of shape {tuple(known.shape[1:])}, the sample is {shape[1:]}: "
                                     f"pass `known` at the sample's shape")
            known_noise = noise.to(self.device, torch.float32).contiguous().clone()
            if start_step > 0:
                sa, sb = self.scheduler._sa_sb(self.scheduler.timesteps[start_step - 1].repeat(batch_size), self.device)
                images = ops.add_noise(known.expand(shape).contiguous(), known_noise, sa, sb, per_sample=True)
        elif audio_file is not None or raw_audio is not None:
            self.mel.load_audio(audio_file, raw_audio)
            input_image = self.mel.audio_slice_to_image(slice)
            input_image = np.frombuffer(input_image.tobytes(), dtype="uint8").reshape(
                (input_image.height, input_image.width)
            )
            input_image = (input_image / 255) * 2 - 1
            input_images = torch.tensor(input_image[np.newaxis, :, :], dtype=torch.float).to(self.device)

            if self.vqvae is not None:
                input_images = self.vqvae.encode(torch.unsqueeze(input_images, 0)).latent_dist.sample(
                    generator=generator
                )[0]
                input_images = 0.18215 * input_images

            if start_step > 0:
                images[0, 0] = self.scheduler.add_noise(input_images, noise, self.scheduler.timesteps[start_step - 1])

            pixels_per_second = (
                self.unet.sample_size[1] * self.mel.get_sample_rate() / self.mel.x_res / self.mel.hop_length
            )
            mask_start = int(mask_start_secs * pixels_per_second)
            mask_end = int(mask_end_secs * pixels_per_second)
            mask = self.scheduler.add_noise(input_images, noise, self.scheduler.timesteps[start_step:].clone())

        use_mask = mask if (mask is not None and (mask_start > 0 or mask_end > 0)) else None
        images, u8 = self._denoise(images, start_step, eta, step_generator, use_mask, mask_start, mask_end,
                                   step_noise=step_noise, want_u8=self.vqvae is None, encoding=encoding,
                                   guidance_scale=guidance_scale, negative_encoding=negative_encoding,
                                   device_noise_seed=device_noise_seed, device_noise_row_offset=device_noise_row_offset,
                                   guidance_rescale=guidance_rescale, window_stride=None if window is None else window[1],
                                   circular=window is not None and window[2], keep_mask=None if kept is None else kept[0],
                                   known=known if kept is not None else None, known_noise=known_noise, known_level=known_level)

        if self.vqvae is not None and window is not None:
            # the wide latent never reaches the decoder as it is: windows of the UNet's width at the sampler's own placement, decoded as
            # one batch and cross-faded in pixel space (include/adm.h "Tiled codec"); the bytes come from the cross-fade kernel
            tiled = self.vqvae.decode_tiled(images, self.unet._hw()[1], window[1], window[2], _in_scale=1 / 0.18215, want_u8=True)
            images, u8 = tiled["sample"], tiled["u8"].permute(0, 2, 3, 1).contiguous()
        elif self.vqvae is not None:
            # 0.18215 was scaling factor used in training to ensure unit variance (pipeline:187-190); the 1/0.18215
            # multiply is folded into the decoder launch
            images = self.vqvae.decode(images, _in_scale=1 / 0.18215)["sample"]
            u8 = ops.dequant_u8(images).permute(0, 2, 3, 1).contiguous()
        final_float = images

        if u8 is None:  # multi-channel: dequantise then NHWC (pipeline:192-194)
            u8 = ops.dequant_u8(images).permute(0, 2, 3, 1).contiguous()
        arr = u8.cpu().numpy()
        images = list(
            map(lambda _: Image.fromarray(_[:, :, 0]), arr)
            if arr.shape[3] == 1
            else map(lambda _: Image.fromarray(_, mode="RGB").convert("L"), arr)
        )

        # the reference maps image_to_audio over the images one by one on a host core (:201); here the whole batch goes
        # through the Mel kernels in one launch sequence
        audios = []
        if audio:
            # (the codec requires the image width to equal x_res; with a `vqvae` the image is f times as wide as the latent)
            mel = self.mel if window is None else self._wide_mel(self._vae_factor() * window[0])
            audios = list(mel.images_to_audios(images, init_phase=init_phase))
        if return_float:
            return images, final_float
        if not return_dict:
            return images, (self.mel.get_sample_rate(), audios)
        return PipelineOutput(audios=np.array(audios)[:, np.newaxis, :] if audio else np.zeros((0, 1, 0)), images=images)

    def _encode_encoding(self, encoding, B):
        """The rules of `encode(encoding=...)`, before any work: required for a conditional model, refused for an unconditional one,
        (B, S, D) or (1, S, D) broadcast over the batch. -> None, or the (B, S, D) fp32 tensor."""
        if not isinstance(self.unet, UNet2DConditionModel):
            if encoding is not None:
                raise ValueError("`encoding` conditions a UNet2DConditionModel: this pipeline's unet is unconditional")
            return None
        if encoding is None:
            raise ValueError("encode() with a UNet2DConditionModel needs the `encoding` the images are to be inverted under: none was given")
        D = self.unet.config.cross_attention_dim
        enc = encoding[:, None, :] if torch.is_tensor(encoding) and encoding.dim() == 2 else encoding
        if not torch.is_tensor(enc) or enc.dim() != 3 or enc.shape[0] not in (1, B) or enc.shape[2] != D:
            got = tuple(encoding.shape) if torch.is_tensor(encoding) else type(encoding).__name__
            raise ValueError(f"encoding shape {got} is not (B, S, D) or (1, S, D) with B = {B}, D = {D}")
        return enc.to(self.device, torch.float32).expand(B, -1, -1)

    @torch.no_grad()
    def encode(self, images: List[Image.Image], steps: int = 50, *, level: str = None, encoding: torch.Tensor = None,
               window_stride: int = None, circular: bool = False, generator: torch.Generator = None) -> torch.Tensor:
        """Reverse step process: recover noisy image from generated image (`pipeline_audio_diffusion.py:207-242`).

        `encode(images, steps)` is the reference's procedure. Not in the reference (defaults reproduce it), for every model family the
        sampler runs; the result has the shape and scale `pipe(noise=...)` takes for this pipeline:
          * `prediction_type` "sample" / "v_prediction": the same native loop with the inversion step of that type. These two have no
            default `level`: without one the call raises the NotImplementedError it always raised, which asks for the rule by name.
          * `level`: None is "reference" for an epsilon model. "reference" gives the model the TARGET timestep of each step, as the reference does; "matched" gives it the
            timestep of the level the sample is at (textbook DDIM inversion; `DDIMScheduler.encode_rows`). On a zero-terminal-SNR
            schedule use "matched": the last "reference" row is finite but degenerate.
          * `encoding` (B, S, D), or (1, S, D) broadcast: required for a UNet2DConditionModel, a ValueError for an unconditional model.
            Guidance is not offered: guided inversion is a different, unstable procedure.
          * with a `vqvae` the images go through `vqvae.encode` and `* 0.18215` and the latent is inverted: the posterior's `.mode()`
            with `generator=None` (inversion is then deterministic), `.sample(generator=generator)` otherwise, the rule of `__call__`.
          * images wider than the model, in cells of the tensor being inverted (image columns; f = 2^(VAE blocks - 1) of them with a
            `vqvae`), are inverted through the windowed loop (include/adm.h "Windowed sampling"): `window_stride` (default W // 2) and
            `circular` place the windows by the rules and with the messages of `__call__(frames=...)`; with a `vqvae` the wide image goes
            through `vqvae.encode_tiled` at that placement. `window_stride` or `circular` with a model-width image: ValueError.
        Every rule is checked before any native call."""
        # Only works with DDIM as this method is deterministic
        assert isinstance(self.scheduler, DDIMScheduler)
        level = self.scheduler._encode_level(level)
        self.scheduler.set_timesteps(steps)
        rows = self.scheduler.encode_rows(level)
        sample = np.array(
            [np.frombuffer(image.tobytes(), dtype="uint8").reshape((1, image.height, image.width)) for image in images]
        )
        sample = (sample / 255) * 2 - 1
        f = self._vae_factor()
        B, _, H, W = sample.shape
        if H % f or W % f:
            raise ValueError(f"images of {H} x {W} pixels are not whole latent cells of {f} x {f} pixels")
        H, W = H // f, W // f   # in cells of the tensor being inverted
        enc = self._encode_encoding(encoding, B)
        mh, mw = self.unet._hw()
        window = self._window(W if W > mw else None, window_stride, circular)
        if window is not None and H != mh:
            raise ValueError(f"a wide sample has the model's height {mh}, not {H}")
        sample = torch.Tensor(sample).to(self.device).contiguous()
        if self.vqvae is not None:
            if window is None:
                dist = self.vqvae.encode(sample).latent_dist
            else:
                dist = self.vqvae.encode_tiled(sample, f * mw, f * window[1], window[2]).latent_dist
            sample = (0.18215 * (dist.mode() if generator is None else dist.sample(generator=generator))).contiguous()
        coef = (N.SchedCoef * len(rows))(*[N.SchedCoef(*[float(r[k]) for k in
                                           ("sqrt_beta", "sqrt_alpha", "clip", "k_x0", "k_x", "k_eps", "k_noise", "timestep")])
                                           for r in rows])
        B, _, H, W = sample.shape
        nW = 1 if window is None else window[3]
        if window is None and (mh, mw) != (H, W):
            self.unet.sample_size = (H, W)
        h = self.unet._ensure_handle()
        if enc is not None:   # set on the handle as `__call__` does: the rows of sample b serve its nW windows, sample-major
            self.unet._set_encoding(h, enc.repeat_interleave(nW, dim=0) if nW > 1 else enc, B * nW, sample.device)
        args = N.SampleLoopArgs(x=N.ptr(sample), B=B, coef_host=coef, n_steps=len(rows), use_graph=1, prediction=self.scheduler.prediction)
        if window is not None:
            args.window_total_w, args.window_stride, args.window_wrap = W, window[1], int(window[2])
        N.check(N.lib().adm_encode_loop_ex(h, args, N.stream_for(sample)))
        return sample

    @staticmethod
    def slerp(x0: torch.Tensor, x1: torch.Tensor, alpha: float) -> torch.Tensor:
        """Spherical Linear intERPolation (`pipeline_audio_diffusion.py:244-258`)."""
        theta = acos(torch.dot(torch.flatten(x0), torch.flatten(x1)) / torch.norm(x0) / torch.norm(x1))
        return sin((1 - alpha) * theta) * x0 / sin(theta) + sin(alpha * theta) * x1 / sin(theta)
