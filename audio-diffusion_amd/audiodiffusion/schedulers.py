"""DDPMScheduler / DDIMScheduler / DPMSolverMultistepScheduler / UniPCMultistepScheduler drop-ins (duck-typed members the reference pipeline calls).

Reference call sites: `audiodiffusion/pipeline_audio_diffusion.py:115,150,157,166-179,221-234`,
`scripts/train_unet.py:161-164,250`. Host side (this file): the beta/alpha tables and the per-step scalar
coefficients, computed in the same 0-d fp32 tensor arithmetic diffusers==0.24.0 uses. Device side: ONE fused
HIP kernel per step (`adm_sched_step_ex`, csrc/k_sched.hip) instead of ~12 eager elementwise kernels plus D2H
scalar reads. `coef_rows()` exports the whole coefficient table so the native sampling loop
(`adm_sample_loop_ex`) can replay a captured hipGraph for every step. `DPMSolverMultistepScheduler` (second-order multistep,
not used by the reference itself) goes through the same two entry points with `mode` 2 (the multistep instantiation of the
kernel): one more coefficient per step and a per-element history of the previous x0 prediction.
`thresholding=True` (DDPM / DDIM) replaces the static clamp of x0 by the dynamic one: a per-sample percentile selected on the
device (`sched_threshold_kernel`) in front of the step kernel, in `step()` and inside the captured loop (`mode` 1).
`prediction_type` "sample" / "v_prediction" (DDPM / DDIM): the model output is the clean sample or the velocity sa*eps - sb*x0 instead
of the noise. The coefficient rows do not change; the step and selection kernels turn (x, output) into (x0, eps) by the type
(the structs' `prediction`; the table is in include/adm.h), and `get_velocity` /
`ops.noise_and_velocity` give the training target. With them come `timestep_spacing` "linspace" / "trailing" and
`rescale_betas_zero_snr` (Lin et al. 2023), whose last training timestep has alphas_cumprod == 0: only the two new types can start
there, an epsilon scheduler refuses such a schedule. The multistep scheduler stays epsilon-only.
`UniPCMultistepScheduler` (UniPC, Zhao et al. 2023) is the few-step solver for everything above: the three prediction types, zero-SNR
schedules, thresholding, guidance and its rescale, through its own fused step kernel (csrc/k_unipc.hip; `adm_sched_step_ex` with
`unipc_table`, `adm_sample_loop_ex` with `unipc_host`). `unipc_rows` computes its coefficient rows from a list of noise levels; the
definition is in include/adm.h ("UniPC").
Classifier-free guidance: `step(..., model_output_uncond=u, guidance_scale=g)` of the three schedulers takes the conditional output as
`model_output` and steps with u + g*(model_output - u), combined inside the one fused kernel (the struct's `eps_uncond`; the
thresholded and the multistep paths included). Both keywords or neither; the `<= 1 means off` rule belongs to the pipeline.
Guidance rescale (Lin et al. 2023 §3.4): `step(..., guidance_rescale=phi)` with the two keywords above rescales that combined output per
sample towards the standard deviation of the conditional one before it is used (include/adm.h "guidance rescale"); None or 0 is off.
Device noise: `step(..., device_noise_seed=s, device_noise_row_offset=r)` (DDPM, DDIM with eta > 0) draws the step's noise inside the fused
kernel from "adm noise stream 1" (include/adm.h) at (seed s, global row r + b, the step's timestep) instead of `randn_tensor`
(the struct's `noise_source` 1). Not together with `generator` or `variance_noise`.
"""
import json
import math
import os

import numpy as np
import torch

from . import ops


class FrozenConfig(dict):
    """dict with attribute access, like diffusers' FrozenDict."""
    __getattr__ = dict.__getitem__


class SchedulerOutput(dict):
    __getattr__ = dict.__getitem__


def randn_tensor(shape, generator=None, device=None, dtype=torch.float32):
    """diffusers.utils.torch_utils.randn_tensor: a CPU generator draws on the CPU and the result is moved."""
    device = torch.device(device or "cpu")
    gen_dev = generator.device.type if generator is not None else device.type
    if gen_dev == "cpu" and device.type != "cpu":
        return torch.randn(shape, generator=generator, device="cpu", dtype=dtype).to(device)
    return torch.randn(shape, generator=generator, device=device, dtype=dtype)


def _betas(n, beta_start, beta_end, schedule):
    if schedule == "linear":
        return torch.linspace(beta_start, beta_end, n, dtype=torch.float32)
    if schedule == "scaled_linear":
        return torch.linspace(beta_start**0.5, beta_end**0.5, n, dtype=torch.float32) ** 2
    if schedule == "squaredcos_cap_v2":
        f = lambda t: math.cos((t + 0.008) / 1.008 * math.pi / 2) ** 2  # noqa: E731
        return torch.tensor([min(1 - f((i + 1) / n) / f(i / n), 0.999) for i in range(n)], dtype=torch.float32)
    raise NotImplementedError(f"{schedule} is not implemented")


def _rescale_zero_snr(betas):
    """[3P-recall] diffusers' `rescale_zero_terminal_snr` (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are
    Flawed", algorithm 1), in the same fp32 tensor arithmetic: shift sqrt(alphas_cumprod) so that its last entry is 0, rescale so that
    its first entry is kept, square, and take ratios back to betas. The last beta is exactly 1 (alphas_cumprod[-1] == 0)."""
    alphas_bar_sqrt = torch.cumprod(1.0 - betas, dim=0).sqrt()
    first, last = alphas_bar_sqrt[0].clone(), alphas_bar_sqrt[-1].clone()
    alphas_bar_sqrt = alphas_bar_sqrt - last
    alphas_bar_sqrt = alphas_bar_sqrt * (first / (first - last))
    alphas_bar = alphas_bar_sqrt ** 2
    alphas = torch.cat([alphas_bar[0:1], alphas_bar[1:] / alphas_bar[:-1]])
    return 1 - alphas


class _SchedulerBase:
    config_name = "scheduler_config.json"
    _class_name = "SchedulerMixin"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear",
                     trained_betas=None, clip_sample=True, clip_sample_range=1.0, prediction_type="epsilon",
                     timestep_spacing="leading", steps_offset=0, thresholding=False,
                     dynamic_thresholding_ratio=0.995, sample_max_value=1.0, rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        cfg = dict(self._defaults)
        unknown = {k: v for k, v in kwargs.items() if k not in cfg and not k.startswith("_")}
        cfg.update({k: v for k, v in kwargs.items() if not k.startswith("_")})
        self._unknown = unknown
        self._check_config(cfg)
        self.config = FrozenConfig(cfg)
        if cfg["trained_betas"] is not None:
            self.betas = torch.tensor(cfg["trained_betas"], dtype=torch.float32)
        else:
            self.betas = _betas(cfg["num_train_timesteps"], cfg["beta_start"], cfg["beta_end"], cfg["beta_schedule"])
        if cfg.get("rescale_betas_zero_snr"):
            self.betas = _rescale_zero_snr(self.betas)
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.one = torch.tensor(1.0)
        self.init_noise_sigma = 1.0
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, cfg["num_train_timesteps"])[::-1].copy())
        self._table = None  # (device, eta) -> device coefficient table

    def _check_config(self, cfg):
        if cfg["prediction_type"] not in ops.PREDICTION_TYPES:
            raise ValueError(f"prediction_type={cfg['prediction_type']!r} must be one of {', '.join(map(repr, ops.PREDICTION_TYPES))}")
        if cfg["timestep_spacing"] not in ("leading", "linspace", "trailing"):
            raise NotImplementedError(f"timestep_spacing={cfg['timestep_spacing']!r} is not implemented (implemented: 'leading', "
                                      f"'linspace', 'trailing')")
        # dynamic thresholding (Imagen §2.3; diffusers' `_threshold_sample` [3P-recall]): checked whether or not it is switched on
        if not 0.0 <= float(cfg["dynamic_thresholding_ratio"]) <= 1.0:
            raise ValueError(f"dynamic_thresholding_ratio={cfg['dynamic_thresholding_ratio']!r} must be in [0, 1]")
        if not float(cfg["sample_max_value"]) >= 1.0:
            raise ValueError(f"sample_max_value={cfg['sample_max_value']!r} must be >= 1")

    # ---- config (de)serialisation: scheduler/scheduler_config.json of the diffusers layout -------------
    @classmethod
    def from_config(cls, cfg):
        return cls(**{k: v for k, v in dict(cfg).items() if not k.startswith("_")})

    @classmethod
    def from_pretrained(cls, path, subfolder=None):
        p = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(p, cls.config_name)) as f:
            return cls.from_config(json.load(f))

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        d = {"_class_name": self._class_name, "_diffusers_version": "0.24.0"}
        d.update(self.config)
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(d, f, indent=2, sort_keys=True)

    # ---- reference members -----------------------------------------------------------------------------
    def set_timesteps(self, num_inference_steps, device=None):
        n_train = self.config.num_train_timesteps
        if num_inference_steps > n_train:
            raise ValueError("num_inference_steps cannot exceed num_train_timesteps")
        spacing = self.config.timestep_spacing
        if spacing == "linspace":      # [3P-recall] the two other spacings of diffusers' DDIM / DDPM schedulers
            ts = np.linspace(0, n_train - 1, num_inference_steps).round()[::-1].copy().astype(np.int64)
        elif spacing == "trailing":    # starts at T - 1: the zero-SNR timestep of a rescaled schedule
            ts = (np.round(np.arange(n_train, 0, -n_train / num_inference_steps)) - 1).astype(np.int64)
        else:
            step_ratio = n_train // num_inference_steps
            ts = (np.arange(0, num_inference_steps) * step_ratio).round()[::-1].copy().astype(np.int64)
            ts += self.config.steps_offset
        if spacing != "leading" and (np.diff(ts) >= 0).any():
            # (diffusers lets them repeat; here `_index_of` would resolve every repeat to its first row, so eager steps and the loop
            #  would part ways)
            raise ValueError(f"{num_inference_steps} steps with timestep_spacing={spacing!r} over {n_train} training timesteps give "
                             f"repeated timesteps; use fewer steps")
        self._refuse_epsilon_at_zero_snr(ts)
        self.num_inference_steps = num_inference_steps
        self.timesteps = torch.from_numpy(ts)
        self._table = None

    @property
    def prediction(self):
        """The C-ABI's integer for `prediction_type`: 0 epsilon, 1 sample, 2 v_prediction."""
        return ops.PREDICTION_TYPES[self.config.prediction_type]

    def _refuse_epsilon_at_zero_snr(self, timesteps):
        """x0 = (x - sb*eps) / sa divides by sa = 0 on a zero-SNR row (`rescale_betas_zero_snr` with a spacing that reaches T - 1).
        The mirror image for a sample model: eps = (x - sa*x0) / sb divides by sb = 0 on a row with alphas_cumprod == 1, which only
        `trained_betas` with leading zeros can make."""
        if self.config.prediction_type == "sample":
            for t in np.asarray(timesteps).tolist():
                if float(self.alphas_cumprod[t]) == 1.0:
                    raise ValueError(f"prediction_type='sample' cannot step from timestep {t}, where alphas_cumprod == 1 (no noise): "
                                     f"eps = (x - sqrt_alpha*x0) / sqrt_beta divides by zero; drop the zero betas or that timestep")
        if self.config.prediction_type != "epsilon":
            return
        for t in np.asarray(timesteps).tolist():
            if float(self.alphas_cumprod[t]) == 0.0:
                raise ValueError(f"prediction_type='epsilon' cannot step from timestep {t}, where alphas_cumprod == 0 (zero terminal "
                                 f"SNR): x0 = (x - sqrt_beta*eps) / sqrt_alpha divides by zero; use prediction_type='v_prediction' or "
                                 f"'sample', or a timestep_spacing that does not reach it")

    def scale_model_input(self, sample, timestep=None):
        return sample

    def add_noise(self, original_samples, noise, timesteps):
        """sqrt(acp[t])*x0 + sqrt(1-acp[t])*noise with diffusers' broadcasting; the two shapes the reference
        uses (pipeline:150,157; train_unet.py:250) run in the fused HIP kernel."""
        ac = self.alphas_cumprod
        ts = torch.as_tensor(timesteps).cpu().long()
        sa = (ac[ts] ** 0.5).flatten().to(noise.device).contiguous()
        sb = ((1 - ac[ts]) ** 0.5).flatten().to(noise.device).contiguous()
        x0 = original_samples.contiguous()
        nz = noise.contiguous()
        if nz.dim() == 4 and x0.shape == nz.shape and sa.numel() == nz.shape[0]:
            return ops.add_noise(x0, nz, sa, sb, per_sample=True)
        if nz.dim() == 4 and x0.dim() == 3 and nz.shape[1] == 1 and x0.shape[0] == 1 and ts.dim() == 1:
            return ops.add_noise(x0, nz, sa, sb, per_sample=False)  # (B, n_steps, H, W) mask (pipeline:157)
        if ts.dim() == 0 and x0.shape[-2:] == nz.shape[-2:] and nz.dim() == 4:
            # pipeline:150: (1,H,W) x (B,1,H,W) with one timestep -> (B,1,H,W)
            return ops.add_noise(x0.reshape(1, *x0.shape[-2:]).contiguous(), nz, sa, sb, per_sample=False)
        raise NotImplementedError("add_noise: unsupported broadcast pattern for the fused kernel")

    def _sa_sb(self, timesteps, device):
        ac = self.alphas_cumprod
        ts = torch.as_tensor(timesteps).cpu().long()
        return (ac[ts] ** 0.5).flatten().to(device).contiguous(), ((1 - ac[ts]) ** 0.5).flatten().to(device).contiguous()

    def add_noise_and_velocity(self, original_samples, noise, timesteps):
        """(add_noise, get_velocity) of the per-sample 4-D case from ONE kernel: what a v_prediction training step needs."""
        x0, nz = original_samples.contiguous(), noise.contiguous()
        sa, sb = self._sa_sb(timesteps, nz.device)
        if not (nz.dim() == 4 and x0.shape == nz.shape and sa.numel() == nz.shape[0]):
            raise NotImplementedError("get_velocity: only (B,C,H,W) samples and noise with one timestep per sample run in the fused kernel")
        return ops.noise_and_velocity(x0, nz, sa, sb)

    def get_velocity(self, sample, noise, timesteps):
        """sqrt(acp[t])*noise - sqrt(1-acp[t])*sample, the regression target of a v_prediction model (diffusers' name) [3P-recall]."""
        return self.add_noise_and_velocity(sample, noise, timesteps)[1]

    def _index_of(self, timestep):
        t = int(timestep)
        idx = (self.timesteps == t).nonzero()
        if idx.numel() == 0:
            raise ValueError(f"timestep {t} is not in the current schedule")
        return int(idx[0])

    def coef_table(self, device, eta=0.0):
        return self._cached(device, eta)[1]

    def _cached(self, device, eta):
        key = (str(device), float(eta))
        if self._table is None or self._table[0] != key:
            rows = self.coef_rows(eta)
            self._table = (key, ops.sched_coef_table(rows, device), rows)
        return self._table

    def _prev_acp(self, t):
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps
        return self.alphas_cumprod[prev_t] if prev_t >= 0 else self._final_alpha()

    def _clip(self):
        return float(self.config.clip_sample_range) if self.config.clip_sample else -1.0

    def threshold(self):
        """None, or (dynamic_thresholding_ratio, sample_max_value) when `thresholding` is on: x0 of every step is then clamped to
        s = clamp(quantile(|x0|, ratio), 1, sample_max_value) per sample and divided by s, INSTEAD of the static `clip_sample`
        clamp (diffusers' `if thresholding ... elif clip_sample`). With sample_max_value = 1 that is exactly the static clamp to 1."""
        if not self.config.thresholding:
            return None
        return float(self.config.dynamic_thresholding_ratio), float(self.config.sample_max_value)

    def _known(self, known, i, device):
        """`step(known=...)`: None, or (known, known_noise, keep, ka, kb): the known-region overwrite of this one step (include/adm.h
        "Region in-painting"): where keep (1 or B, H, W) is non-zero the result is ka*known + kb*known_noise. -> the tuple
        `ops.sched_step(known=...)` takes: the three tensors and a table that holds (ka, kb) on row `i`."""
        if known is None:
            return None
        kn, kz, keep, ka, kb = known
        table = torch.zeros((i + 1, 2), dtype=torch.float32)
        table[i, 0], table[i, 1] = float(ka), float(kb)
        keep = (torch.as_tensor(keep) != 0).to(torch.uint8).to(device).contiguous()
        return kn.contiguous(), kz.contiguous(), keep[None] if keep.dim() == 2 else keep, table.to(device)

    def _step(self, model_output, timestep, sample, eta, generator, variance_noise, model_output_uncond=None, guidance_scale=None,
              device_noise_seed=None, device_noise_row_offset=0, guidance_rescale=None, known=None):
        if device_noise_seed is not None:
            for name, given in (("generator", generator), ("variance_noise", variance_noise)):
                if given is not None:
                    raise ValueError(f"device_noise_seed draws the step noise inside the kernel: it cannot be combined with `{name}`")
        i = self._index_of(timestep)
        _, table, rows = self._cached(sample.device, eta)
        need_noise = rows[i]["k_noise"] != 0.0
        if need_noise and variance_noise is None and device_noise_seed is None:
            variance_noise = randn_tensor(model_output.shape, generator, model_output.device, model_output.dtype)
        prev = ops.sched_step(sample.contiguous(), model_output.contiguous(), table, i,
                              noise=variance_noise.contiguous() if variance_noise is not None else None,
                              threshold=self.threshold(), prediction=self.prediction,
                              uncond=model_output_uncond.contiguous() if model_output_uncond is not None else None,
                              guidance_scale=guidance_scale, noise_seed=device_noise_seed, noise_row_offset=device_noise_row_offset,
                              guidance_rescale=guidance_rescale, known=self._known(known, i, sample.device))
        return SchedulerOutput(prev_sample=prev)


class DDPMScheduler(_SchedulerBase):
    _class_name = "DDPMScheduler"
    _defaults = dict(_SchedulerBase._defaults, variance_type="fixed_small", clip_sample=True)

    def __init__(self, **kw):
        super().__init__(**kw)
        if self.config.variance_type != "fixed_small":
            raise NotImplementedError("only variance_type='fixed_small' is implemented")

    def _final_alpha(self):
        return self.one

    def coef_rows(self, eta=0.0):
        self._refuse_epsilon_at_zero_snr(self.timesteps)
        rows = []
        for t in self.timesteps.tolist():
            a_t = self.alphas_cumprod[t]
            a_prev = self._prev_acp(t)
            b_t = 1 - a_t
            b_prev = 1 - a_prev
            cur_a = a_t / a_prev
            cur_b = 1 - cur_a
            k_noise = 0.0
            if t > 0:
                var = torch.clamp((1 - a_prev) / (1 - a_t) * cur_b, min=1e-20)
                k_noise = float(var ** 0.5)
            rows.append(dict(sqrt_beta=float(b_t ** 0.5), sqrt_alpha=float(a_t ** 0.5), clip=self._clip(),
                             k_x0=float((a_prev ** 0.5 * cur_b) / b_t), k_x=float(cur_a ** 0.5 * b_prev / b_t),
                             k_eps=0.0, k_noise=k_noise, timestep=float(t)))
        return rows

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, variance_noise=None, *,
             model_output_uncond=None, guidance_scale=None, device_noise_seed=None, device_noise_row_offset=0, guidance_rescale=None,
             known=None):
        return self._step(model_output, timestep, sample, 0.0, generator, variance_noise, model_output_uncond, guidance_scale,
                          device_noise_seed, device_noise_row_offset, guidance_rescale, known)


class DDIMScheduler(_SchedulerBase):
    _class_name = "DDIMScheduler"
    _defaults = dict(_SchedulerBase._defaults, set_alpha_to_one=True, clip_sample=True)

    def __init__(self, **kw):
        super().__init__(**kw)
        self.final_alpha_cumprod = torch.tensor(1.0) if self.config.set_alpha_to_one else self.alphas_cumprod[0]

    def _final_alpha(self):
        return self.final_alpha_cumprod

    def coef_rows(self, eta=0.0):
        self._refuse_epsilon_at_zero_snr(self.timesteps)
        rows = []
        for t in self.timesteps.tolist():
            a_t = self.alphas_cumprod[t]
            a_prev = self._prev_acp(t)
            b_t = 1 - a_t
            b_prev = 1 - a_prev
            variance = (b_prev / b_t) * (1 - a_t / a_prev)
            std = eta * variance ** 0.5
            rows.append(dict(sqrt_beta=float(b_t ** 0.5), sqrt_alpha=float(a_t ** 0.5), clip=self._clip(),
                             k_x0=float(a_prev ** 0.5), k_x=0.0, k_eps=float((1 - a_prev - std ** 2) ** 0.5),
                             k_noise=float(std) if eta > 0 else 0.0, timestep=float(t)))
        return rows

    ENCODE_LEVELS = ("reference", "matched")

    def _encode_level(self, level):
        """`level=None`: "reference" for an epsilon model, the call as it always was; the other two prediction types have no default and
        keep the NotImplementedError they always gave, which now asks for the rule by name."""
        if level is None:
            if self.config.prediction_type != "epsilon":
                raise NotImplementedError(f"encode() has no default `level` for prediction_type={self.config.prediction_type!r}: the "
                                          f"reference's rule uses the model output at a mismatched noise level. Pass level='matched' "
                                          f"(the model is given the sample's own timestep) or level='reference' (the reference's rule)")
            return "reference"
        if level not in self.ENCODE_LEVELS:
            raise ValueError(f"level={level!r} must be one of {self.ENCODE_LEVELS}")
        return level

    def encode_rows(self, level=None):
        """Rows of the DDIM inversion update in loop order (ascending timesteps; include/adm.h "DDIM inversion" names the fields). With
        s = `_prev_acp(t)` the level the sample has, t the target level, c the level of the timestep the model is given and e the noise
        prediction formed from the model output at c (the table of `coef_rows`' prediction types):
            x' = (x - sqrt(1 - s)*e) * s^-0.5 * t^0.5 + sqrt(1 - t)*e
        level="reference": the reference's rule (`pipeline_audio_diffusion.py:228-240`): the model is given the TARGET timestep t and
            c = t, although the sample sits at s: a first-order error. For an epsilon model these are the reference's rows, bit for bit.
        level="matched": textbook DDIM inversion: the model is given the sample's own timestep max(t - T // N, 0) and c is
            alphas_cumprod there. On the first row s may be `final_alpha_cumprod` = 1: x0 = x exactly, and nothing divides by zero.
        level=None (default): "reference" for an epsilon model; a NotImplementedError naming `prediction_type` for the other two, as before
            they were built: for them the rule is to be named.
        All three prediction types, every `timestep_spacing` and `rescale_betas_zero_snr` are accepted (an epsilon model on a zero-SNR
        row stays refused, as in sampling). On a zero-terminal-SNR schedule the last "reference" row is finite but degenerate: the
        model is evaluated where its output says nothing about the noise (e = x for a sample or v model, so x' = x): use "matched"."""
        level = self._encode_level(level)
        ts = torch.flip(self.timesteps, (0,)).tolist()
        ratio = self.config.num_train_timesteps // self.num_inference_steps
        given = ts if level == "reference" else [max(t - ratio, 0) for t in ts]
        self._refuse_epsilon_at_zero_snr(ts)
        if self.config.prediction_type == "sample":     # (its e divides by sqrt(1 - c))
            self._refuse_epsilon_at_zero_snr(given)
        eps = self.config.prediction_type == "epsilon"  # reads no conversion pair: its rows keep the zeros they had
        rows = []
        for t, tc in zip(ts, given):
            a_t = self.alphas_cumprod[t]
            a_prev = self._prev_acp(t)
            a_c = self.alphas_cumprod[tc]
            b_t = 1 - a_t
            rows.append(dict(sqrt_beta=float((1 - a_prev) ** 0.5), sqrt_alpha=float(a_prev ** (-0.5)), clip=-1.0,
                             k_x0=float(a_t ** 0.5), k_x=0.0 if eps else float(a_c ** 0.5), k_eps=float(b_t ** 0.5),
                             k_noise=0.0 if eps else float((1 - a_c) ** 0.5), timestep=float(tc)))
        return rows

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True, *, model_output_uncond=None, guidance_scale=None, device_noise_seed=None,
             device_noise_row_offset=0, guidance_rescale=None, known=None):
        if use_clipped_model_output:
            raise NotImplementedError("use_clipped_model_output is not implemented (the reference never sets it)")
        return self._step(model_output, timestep, sample, float(eta), generator, variance_noise, model_output_uncond, guidance_scale,
                          device_noise_seed, device_noise_row_offset, guidance_rescale, known)


def _f32(v):
    """One rounding of a float64 host scalar to the fp32 the kernel reads."""
    return float(np.float32(v))


def _solver_timesteps(cfg, N):
    """The N timesteps of the few-step solvers (DPM-Solver++ multistep, UniPC) for `timestep_spacing` linspace / leading / trailing, with
    their ValueErrors: every row must move to a strictly lower noise level."""
    T = cfg.num_train_timesteps
    if N < 1 or N > T:
        raise ValueError("num_inference_steps must be in [1, num_train_timesteps]")
    spacing = cfg.timestep_spacing
    if spacing == "linspace":
        ts = np.linspace(0, T - 1, N + 1).round()[::-1][:-1]
    elif spacing == "leading":
        ts = (np.arange(0, N + 1) * (T // (N + 1))).round()[::-1][:-1] + cfg.steps_offset
    else:
        ts = np.arange(T, 0, -T / N).round() - 1
    ts = ts.copy().astype(np.int64)
    # every row must move to a lower noise level (h > 0): the second-order rows divide by h
    if ts.max() >= T or ts.min() < 0 or (np.diff(ts) >= 0).any():
        raise ValueError(f"{N} steps with timestep_spacing={spacing!r} over {T} training timesteps give repeated or out-of-range "
                         f"timesteps; use fewer steps")
    if cfg.final_sigmas_type == "sigma_min" and ts[-1] == 0:
        raise ValueError(f"{N} steps with timestep_spacing={spacing!r} reach timestep 0 before the final row, which "
                         f"final_sigmas_type='sigma_min' ends at; use fewer steps or final_sigmas_type='zero'")
    return ts


class DPMSolverMultistepScheduler(_SchedulerBase):
    """DPM-Solver++ multistep (Lu et al. 2022, "2M"): a first- or second-order data-prediction solver of the
    probability-flow ODE, for sampling an epsilon-model trained on the DDPM schedule in 15-25 steps.

    [3P-recall] Config names, defaults, timestep spacings and the update follow diffusers'
    `DPMSolverMultistepScheduler` as recalled; diffusers is not installed where this was written, so the arithmetic is
    unpinned (like the other third-party arithmetic of this package). What is anchored independently (tests/test_dpmsolver.py):
    order 1 is the DDIM update, and on an analytic Gaussian model the second-order rows converge faster than the first-order
    ones to the exact solution of the ODE.

    The update is linear in (x, x0 of this step, x0 of the previous step):
        x' = k_x*x + k_x0*m0 + k_hist*m1,   m0 = (x - sqrt_beta*eps) / sqrt_alpha
    so a step is one fused kernel (`adm_sched_step_ex`, `mode` 2) with the eight `adm_sched_coef` fields, one extra per-step
    coefficient `k_hist` and a per-element history buffer. Scalars are computed in float64 on the host and rounded to fp32
    once. Built: `solver_order` 1 and 2, `algorithm_type="dpmsolver++"`, `solver_type` midpoint / heun, the three timestep
    spacings, `final_sigmas_type` zero / sigma_min, `lower_order_final`, `euler_at_final`. Everything else raises
    NotImplementedError naming the key (the SDE variants need per-step noise and a history that survives the pipeline's
    noise-staging chunks). `thresholding=True` raises as well: the selection kernel of the DDIM / DDPM schedulers
    (`sched_threshold_kernel`) is what a thresholded multistep step would reuse: one more instantiation of `sched_step_kernel`, which is not built."""
    _class_name = "DPMSolverMultistepScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, algorithm_type="dpmsolver++", solver_type="midpoint", lower_order_final=True,
                     euler_at_final=False, use_karras_sigmas=False, use_lu_lambdas=False, final_sigmas_type="zero",
                     lambda_min_clipped=-float("inf"), variance_type=None, timestep_spacing="linspace", steps_offset=0)

    def __init__(self, **kwargs):
        # keys of another scheduler's config (`from_config(pipe.scheduler.config)`) are dropped, as diffusers does
        if kwargs.get("rescale_betas_zero_snr"):   # not dropped with the other foreign keys: it changes the schedule
            raise NotImplementedError("rescale_betas_zero_snr=True is not implemented for DPMSolverMultistepScheduler (epsilon only: "
                                      "sigma is infinite at the zero-SNR timestep)")
        known = {k: v for k, v in kwargs.items() if k in self._defaults}
        super().__init__(**known)
        self._unknown = {k: v for k, v in kwargs.items() if k not in self._defaults and not k.startswith("_")}
        self._reset_multistep()

    prediction = 0   # epsilon only (`_check_config`)

    def _check_config(self, cfg):
        def only(key, allowed):
            if cfg[key] not in allowed:
                raise NotImplementedError(f"{key}={cfg[key]!r} is not implemented (implemented: {', '.join(map(repr, allowed))})")
        only("solver_order", (1, 2))
        only("prediction_type", ("epsilon",))
        only("algorithm_type", ("dpmsolver++",))
        only("solver_type", ("midpoint", "heun"))
        only("timestep_spacing", ("linspace", "leading", "trailing"))
        only("final_sigmas_type", ("zero", "sigma_min"))
        # (a DDPM config carries "fixed_small" / "fixed_large": the variance of ITS noise term, which this solver does not have; the
        #  learned kinds mean a model with extra variance channels, which the loop does not split off)
        only("variance_type", (None, "fixed_small", "fixed_small_log", "fixed_large", "fixed_large_log"))
        for key in ("thresholding", "use_karras_sigmas", "use_lu_lambdas"):
            if cfg[key]:
                raise NotImplementedError(f"{key}={cfg[key]!r} is not implemented")
        if cfg["lambda_min_clipped"] != -float("inf"):
            raise NotImplementedError(f"lambda_min_clipped={cfg['lambda_min_clipped']!r} is not implemented (only -inf)")

    def _reset_multistep(self):
        self._hist = None          # x0 prediction of the previous eager step (device tensor, rewritten in place by the kernel)
        self._last_index = None    # row of the previous eager step; the next row continues the run, any other starts a new one
        self._run_start = 0
        self._ms_tables = {}       # (device, first row of the run) -> (coef table, k_hist table) on the device

    def set_timesteps(self, num_inference_steps, device=None):
        N = int(num_inference_steps)
        ts = _solver_timesteps(self.config, N)
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(ts)
        self._table = None
        self._reset_multistep()

    # ---- coefficient rows -------------------------------------------------------------------------------
    def _levels(self):
        """float64 (alpha_i, s_i, lambda_i) for i = 0..N; level N is the end of the run (sigma 0, or sigma of timestep 0)."""
        acp = self.alphas_cumprod.double().numpy()
        t = self.timesteps.numpy()
        sig = list(np.sqrt((1 - acp[t]) / acp[t]))
        sig.append(0.0 if self.config.final_sigmas_type == "zero" else float(np.sqrt((1 - acp[0]) / acp[0])))
        out = []
        for sg in sig:
            a = 1.0 / math.sqrt(sg * sg + 1.0)
            s_ = sg * a
            out.append((a, s_, math.log(a) - math.log(s_) if s_ > 0 else math.inf))
        return out

    def _run_rows(self, run_start):
        """All N rows of the table of a run that STARTS at row `run_start`: that row is first order (there is no previous x0
        prediction yet), the rows after it are as in the full schedule (and so are the rows before it, which such a run never
        reads). Each row: the eight `adm_sched_coef` fields and `k_hist`."""
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        cfg, N = self.config, self.num_inference_steps
        lv = self._levels()
        ts = self.timesteps.tolist()
        rows = []
        for i in range(N):
            (a0, s0, l0), (a1, s1, l1) = lv[i], lv[i + 1]
            last = i == N - 1
            first_order = (cfg.solver_order == 1 or i == run_start or i == 0 or
                           (last and (cfg.euler_at_final or (cfg.lower_order_final and N < 15) or
                                      cfg.final_sigmas_type == "zero")))
            if math.isinf(l1):            # sigma_N = 0: h = inf, e^-h = 0, written out rather than left to inf arithmetic
                k_x, c, first_order = 0.0, 1.0, True
            else:
                h = l1 - l0
                k_x, c = s1 / s0, a1 * (1.0 - math.exp(-h))
            if first_order:
                k_x0, k_hist = c, 0.0
            else:
                r = (l0 - lv[i - 1][2]) / h
                if cfg.solver_type == "midpoint":
                    k_x0, k_hist = c * (1.0 + 1.0 / (2.0 * r)), -c / (2.0 * r)
                else:
                    g = a1 * ((math.exp(-h) - 1.0) / h + 1.0)
                    k_x0, k_hist = c + g / r, -g / r
            rows.append(dict(sqrt_beta=_f32(s0), sqrt_alpha=_f32(a0), clip=-1.0, k_x0=_f32(k_x0), k_x=_f32(k_x), k_eps=0.0,
                             k_noise=0.0, timestep=float(ts[i]), k_hist=_f32(k_hist)))
        return rows

    def loop_rows(self, start_step=0, stop_step=None):
        """Rows [start_step:stop_step] of a run that starts at `start_step` (first order there): what the native loop is given."""
        return self._run_rows(start_step)[start_step:stop_step]

    def coef_rows(self, eta=0.0):
        """The whole schedule from its first row. `eta` is accepted for the callers that pass it to every scheduler and is ignored:
        the solver is deterministic (no row has a noise term)."""
        return self._run_rows(0)

    # ---- eager step ---------------------------------------------------------------------------------------
    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True, *,
             model_output_uncond=None, guidance_scale=None, guidance_rescale=None, known=None):
        """One fused kernel (with model_output_uncond and guidance_scale: the guided one, whose history is x0 of the guided output). First order on the first call after `set_timesteps` (and whenever the call does not continue the
        previous one: another row than the next, another shape or device); the scheduler holds the history tensor."""
        i = self._index_of(timestep)
        fresh = (self._hist is None or self._hist.shape != sample.shape or self._hist.device != sample.device)
        if fresh or self._last_index is None or i != self._last_index + 1:
            self._run_start = i
        if fresh:
            self._hist = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
        key = (str(sample.device), self._run_start)
        if key not in self._ms_tables:
            rows = self._run_rows(self._run_start)
            self._ms_tables = {key: (ops.sched_coef_table(rows, sample.device),
                                     torch.tensor([r["k_hist"] for r in rows], dtype=torch.float32).to(sample.device))}
        table, khist = self._ms_tables[key]
        prev = ops.sched_multistep(sample.contiguous(), model_output.contiguous(), table, khist, self._hist, i,
                                   uncond=model_output_uncond.contiguous() if model_output_uncond is not None else None,
                                   guidance_scale=guidance_scale, guidance_rescale=guidance_rescale,
                                   known=self._known(known, i, sample.device))
        self._last_index = i
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


# ---- UniPC (include/adm.h "UniPC" has THE definition; the names below are its names) -------------------------------------------------
def _unipc_phi_b(h, solver_type, K):
    """(phi, B, [b_1 .. b_K]) of a step h > 0; h = +inf (the previous level at zero SNR): phi = B = -1 and no vector."""
    if math.isinf(h):
        return -1.0, -1.0, []
    hh = -h
    phi = math.expm1(hh)
    B = phi if solver_type == "bh2" else hh
    g, f, b = phi / hh - 1.0, 1.0, []
    for k in range(1, K + 1):
        b.append(g * f / B)
        f *= k + 1
        g = g / hh - 1.0 / f
    return phi, B, b


def unipc_rows(levels, solver_order=2, solver_type="bh2", run_start=0, lower_order_final=True, disable_corrector=()):
    """The N coefficient rows of a UniPC run over `levels` = [(alpha_i, sigma_i, lambda_i) for i in 0..N] (float64) that STARTS at row
    `run_start`: a pure function of the level list, so that any grid can be given (the scheduler passes its own; the convergence tests
    an analytic one). Each row: the eight `adm_sched_coef` fields (timestep = the row index; the scheduler overwrites it) and the five
    `adm_unipc_coef` fields, computed in float64 and rounded to fp32 once. Rows before `run_start` are as in a run from row 0 (such a
    run never reads them)."""
    if solver_type not in ("bh1", "bh2"):
        raise NotImplementedError(f"solver_type={solver_type!r} is not implemented (implemented: 'bh1', 'bh2')")
    if solver_order not in (1, 2):
        raise NotImplementedError(f"solver_order={solver_order!r} is not implemented (implemented: 1, 2)")
    N = len(levels) - 1
    off = set(int(i) for i in disable_corrector)
    rows, p_prev = [], None
    for i in range(N):
        (a0, s0, l0), (a1, s1, l1) = levels[i], levels[i + 1]
        start = run_start if i >= run_start else 0
        p = min(solver_order, i - start + 1, N - i if lower_order_final else solver_order)
        if p == 2 and math.isinf(levels[i - 1][2]):     # a zero-SNR level is never history
            p = 1
        # the corrector of the move i-1 -> i, of the order of that move's predictor
        c_x = c_m1 = c_m2 = c_t = 0.0
        if i > start and (i - 1) not in off:
            am, sm, lm = levels[i - 1]
            q = 1 if math.isinf(lm) else p_prev
            h = l0 - lm
            phi, B, b = _unipc_phi_b(h, solver_type, q)
            c_x = s0 / sm
            if q == 1:
                rho_last = 0.5
            else:
                r1 = (levels[i - 2][2] - lm) / h
                rho_1 = (b[0] - b[1]) / (1.0 - r1)      # [[1, 1], [r1, 1]] rho = b
                rho_last = b[0] - rho_1
                c_m2 = -a0 * B * rho_1 / r1
            c_t = -a0 * B * rho_last
            c_m1 = -a0 * phi - c_t - c_m2
        # the predictor of the move i -> i+1
        p_m1 = 0.0
        if math.isinf(l1):                # sigma = 0: x' = m_i, written out
            k_x, k_x0 = 0.0, 1.0
        elif math.isinf(l0):              # from zero SNR (alpha_i = 0, sigma_i = 1): phi = B = -1
            k_x, k_x0 = s1, a1
        else:
            h = l1 - l0
            phi, B, _ = _unipc_phi_b(h, solver_type, 0)
            k_x, k_x0 = s1 / s0, -a1 * phi
            if p == 2:
                r1 = (levels[i - 1][2] - l0) / h
                p_m1 = -a1 * B * 0.5 / r1
                k_x0 -= p_m1
        rows.append(dict(sqrt_beta=_f32(s0), sqrt_alpha=_f32(a0), clip=-1.0, k_x0=_f32(k_x0), k_x=_f32(k_x), k_eps=0.0, k_noise=0.0,
                         timestep=float(i), c_x=_f32(c_x), c_m1=_f32(c_m1), c_m2=_f32(c_m2), c_t=_f32(c_t), p_m1=_f32(p_m1)))
        p_prev = p
    return rows


class UniPCMultistepScheduler(_SchedulerBase):
    """UniPC (Zhao et al. 2023): a multistep predictor of order 1 or 2 in data-prediction form plus a corrector that re-does each move
    once the model has been evaluated at its end, raising the order of accuracy by one at no extra model evaluation. For 10-20 step
    sampling of epsilon, sample and v_prediction models, zero-terminal-SNR schedules and dynamically thresholded ones included, which
    `DPMSolverMultistepScheduler` refuses.

    [3P-recall] Config names and defaults follow diffusers' `UniPCMultistepScheduler` as recalled; the arithmetic is defined in
    include/adm.h ("UniPC") and anchored independently in tests/test_unipc.py (order 1 without correctors is DDIM, order 2 without
    correctors is DPM-Solver++ 2M midpoint, and the observed convergence orders on an analytic Gaussian model).

    A step is one fused kernel (`adm_sched_step_ex` with `unipc_table`, csrc/k_unipc.hip): the row's `adm_sched_coef`, its
    `adm_unipc_coef` and three per-element state buffers (the corrected sample of the previous row, two data predictions). Built:
    `solver_order` 1 and 2, `solver_type` bh1 / bh2, `predict_x0=True`, the three prediction types, `thresholding`, `lower_order_final`,
    `disable_corrector`, the three timestep spacings, `final_sigmas_type` zero / sigma_min, `rescale_betas_zero_snr`. Everything else
    raises NotImplementedError naming the key. Keys of another scheduler's config are dropped."""
    _class_name = "UniPCMultistepScheduler"
    _defaults = dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule="linear", trained_betas=None,
                     solver_order=2, prediction_type="epsilon", thresholding=False, dynamic_thresholding_ratio=0.995,
                     sample_max_value=1.0, predict_x0=True, solver_type="bh2", lower_order_final=True, disable_corrector=(),
                     solver_p=None, use_karras_sigmas=False, timestep_spacing="linspace", steps_offset=0, final_sigmas_type="zero",
                     rescale_betas_zero_snr=False)

    def __init__(self, **kwargs):
        known = {k: v for k, v in kwargs.items() if k in self._defaults}
        if "disable_corrector" in known:
            known["disable_corrector"] = [int(i) for i in (known["disable_corrector"] or ())]
        else:
            known["disable_corrector"] = []
        super().__init__(**known)
        self._unknown = {k: v for k, v in kwargs.items() if k not in self._defaults and not k.startswith("_")}
        self._reset_run()

    def _check_config(self, cfg):
        super()._check_config(cfg)

        def only(key, allowed):
            if cfg[key] not in allowed:
                raise NotImplementedError(f"{key}={cfg[key]!r} is not implemented (implemented: {', '.join(map(repr, allowed))})")
        only("solver_order", (1, 2))
        only("solver_type", ("bh1", "bh2"))
        only("predict_x0", (True,))
        only("solver_p", (None,))
        only("final_sigmas_type", ("zero", "sigma_min"))
        if cfg["use_karras_sigmas"]:
            raise NotImplementedError(f"use_karras_sigmas={cfg['use_karras_sigmas']!r} is not implemented")

    def _reset_run(self):
        self._hist = None          # (2,B,C,H,W): the data predictions of the two previous eager steps (rewritten in place by the kernel)
        self._last = None          # (B,C,H,W): the corrected sample of the previous eager step
        self._last_index = None    # row of the previous eager step; the next row continues the run, any other starts a new one
        self._run_start = 0
        self._run_tables = {}      # (device, first row of the run) -> (coef table, unipc table) on the device

    def set_timesteps(self, num_inference_steps, device=None):
        N = int(num_inference_steps)
        ts = _solver_timesteps(self.config, N)
        self._refuse_epsilon_at_zero_snr(ts)
        self.num_inference_steps = N
        self.timesteps = torch.from_numpy(ts)
        self._table = None
        self._reset_run()

    # ---- coefficient rows -------------------------------------------------------------------------------
    def _levels(self):
        """float64 (alpha_i, sigma_i, lambda_i) for i = 0..N; level N is the end of the run (sigma 0, or the sigma of timestep 0). A
        timestep with alphas_cumprod == 0 (zero terminal SNR) is (0, 1, -inf)."""
        acp = self.alphas_cumprod.double().numpy()
        out = []
        for t in self.timesteps.tolist() + ([] if self.config.final_sigmas_type == "zero" else [0]):
            if acp[t] == 0.0:
                out.append((0.0, 1.0, -math.inf))
                continue
            sg = math.sqrt((1 - acp[t]) / acp[t])
            a = 1.0 / math.sqrt(sg * sg + 1.0)
            s_ = sg * a
            out.append((a, s_, math.log(a) - math.log(s_)))
        if self.config.final_sigmas_type == "zero":
            out.append((1.0, 0.0, math.inf))
        return out

    def _run_rows(self, run_start):
        if self.num_inference_steps is None:
            raise ValueError("call set_timesteps first")
        self._refuse_epsilon_at_zero_snr(self.timesteps)
        cfg = self.config
        rows = unipc_rows(self._levels(), cfg.solver_order, cfg.solver_type, run_start, cfg.lower_order_final, cfg.disable_corrector)
        for r, t in zip(rows, self.timesteps.tolist()):
            r["timestep"] = float(t)
        return rows

    def loop_rows(self, start_step=0, stop_step=None):
        """Rows [start_step:stop_step] of a run that starts at `start_step` (no corrector and first order there): what the native loop
        is given."""
        return self._run_rows(start_step)[start_step:stop_step]

    def coef_rows(self, eta=0.0):
        """The whole schedule from its first row. `eta` is accepted for the callers that pass it to every scheduler and is ignored: the
        solver is deterministic (no row has a noise term)."""
        return self._run_rows(0)

    # ---- eager step ---------------------------------------------------------------------------------------
    def step(self, model_output, timestep, sample, generator=None, variance_noise=None, return_dict=True, *,
             model_output_uncond=None, guidance_scale=None, guidance_rescale=None, known=None):
        """One fused kernel. The scheduler holds the state (`last`, the two-slot history); the first call after `set_timesteps`, and any
        call that does not continue the previous one (another row than the next, another shape or device), starts a new run: no
        corrector and a first-order predictor there."""
        i = self._index_of(timestep)
        fresh = (self._last is None or self._last.shape != sample.shape or self._last.device != sample.device)
        if fresh or self._last_index is None or i != self._last_index + 1:
            self._run_start = i
        if fresh:
            self._last = torch.empty(sample.shape, dtype=torch.float32, device=sample.device)
            self._hist = torch.empty((2,) + tuple(sample.shape), dtype=torch.float32, device=sample.device)
        key = (str(sample.device), self._run_start)
        if key not in self._run_tables:
            rows = self._run_rows(self._run_start)
            self._run_tables = {key: (ops.sched_coef_table(rows, sample.device), ops.sched_unipc_table(rows, sample.device))}
        table, utable = self._run_tables[key]
        prev = ops.sched_unipc(sample.contiguous(), model_output.contiguous(), table, utable, self._hist, self._last, i,
                               uncond=model_output_uncond.contiguous() if model_output_uncond is not None else None,
                               guidance_scale=guidance_scale, guidance_rescale=guidance_rescale, threshold=self.threshold(),
                               prediction=self.prediction, known=self._known(known, i, sample.device))
        self._last_index = i
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)
