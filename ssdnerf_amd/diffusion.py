"""``GaussianDiffusion`` for the triplane latents: noise schedule, DDIM / Langevin / ancestral sampling with the rendering-loss
guidance hook, and the diffusion prior loss (behaviour of lib/models/diffusions/gaussian_diffusion.py:14-464, sampler.py:7-44,
lib/models/losses/ddpm_loss.py:11-142).  Constructor keywords, registry names and the public
methods are the reference's; the implementation is organised for the MI355X instead of following the reference's per-step host code:

* ``NoiseSchedule`` holds the float64 tables once; everything a sampling trajectory needs from them is resolved ON THE HOST, ONCE, into a
  ``SamplingPlan`` -- a flat list of network evaluations, each with its timestep and its scalar coefficients.  The loops below never index
  a numpy table with a device tensor (the reference does, which costs a device->host sync per lookup, gaussian_diffusion.py:275-283) and
  never upload a table per call.
* A step without guidance is: write ``t`` into the UNet session's static buffer, replay the captured forward (``unet_fast.UnetSession``), ONE
  fused elementwise launch (csrc/sampler_step.hip) that turns (x_t, v) into (x0, x_next) and writes x_next back IN PLACE into the session's
  input buffer.  Three launches per step, no copies, no allocation, no host sync in the loop.  ``ssdnerf_ddim_step_v`` serves DDIM at eta = 0;
  ``ssdnerf_dpmpp_step_v`` serves ``sample_method='dpmpp_2m'`` (DPM-Solver++(2M) over the same timesteps; not in the reference, opt-in), which
  also reads the x0 of the step before from one of two alternating history buffers.
* ``test_cfg['noise_source']='device'`` (opt-in; the default ``'host'`` is the seeded CPU draw described at ``_host_noise``): every noise-injecting
  step -- DDIM with eta > 0, Langevin corrections, the ancestral sampler, ``sample_method='dpmpp_2m_sde'`` (SDE-DPM-Solver++(2M); not in the
  reference, opt-in) -- stays in the session too: ``ssdnerf_sde_step_v`` makes its normals in registers from a counter-based generator
  (csrc/philox.h) keyed by ``test_cfg['noise_seed']``; the tensor-expression branch takes the same normals from ``ssdnerf_philox_normal_fill``.
* ``cfg['noise_source']='device'`` in ``forward_train`` (opt-in, ``train_cfg`` / ``test_cfg``): the prior loss takes its noise from the
  same generator under draws numbered 0x80000000 | k, and the arithmetic around the UNet -- q_sample, the V target, the per-sample mean of squares, their
  gradients -- is three launches of csrc/prior_loss.hip that make the normals in registers; what follows the mean stays in ``DDPMMSELossMod``.
* The guided step (rendering guidance, SSDNeRF's ``grad_guide_fn``) needs autograd through the UNet and the renderer; it keeps tensors in
  the graph exactly where the reference does, with the coefficients coming from the plan as Python floats.
"""
from __future__ import annotations

import math
from copy import deepcopy
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn

from . import _cabi as C
from .registry import MODULES, build_module


class _PinnedRing:
    """Two pinned host buffers per (device, shape) and an event behind each upload: a host draw lands in pinned memory and goes to the device with an
    ASYNCHRONOUS copy, so the caller is not blocked until the stream reaches the copy (a pageable-memory upload is)."""
    rings: Dict = {}

    @classmethod
    def upload(cls, shape, device) -> torch.Tensor:
        key = (tuple(shape), str(device))
        ring = cls.rings.get(key)
        if ring is None:
            if len(cls.rings) >= 8:                             # (pinned memory is a scarce resource: keep the rings of the last few shapes only)
                old = cls.rings.pop(next(iter(cls.rings)))
                for ev in old["events"]:
                    if ev is not None:
                        ev.synchronize()
            ring = cls.rings[key] = {"bufs": [torch.empty(shape, dtype=torch.float32).pin_memory() for _ in range(2)], "events": [None, None], "i": 0}
        i = ring["i"]
        ring["i"] = i ^ 1
        if ring["events"][i] is not None:
            ring["events"][i].synchronize()                     # (the upload that last used this buffer: two draws ago)
        torch.randn(shape, dtype=torch.float32, out=ring["bufs"][i])
        out = ring["bufs"][i].to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        ring["events"][i] = ev
        return out

    @classmethod
    def release(cls) -> None:
        """give the pinned buffers back (r04 advisor: up to 8 shapes x 2 buffers stayed pinned for the life of the process); in-flight uploads are waited for"""
        for ring in cls.rings.values():
            for ev in ring["events"]:
                if ev is not None:
                    ev.synchronize()
        cls.rings.clear()


def release_pinned_buffers() -> None:
    """free the pinned host staging buffers of the seeded host draws (``_host_noise``); they are re-created on demand"""
    _PinnedRing.release()


def _require_device_latent(x: torch.Tensor) -> None:
    if not x.is_cuda:
        raise ValueError("noise_source='device' needs the latent on the GPU (there is no CPU path of the counter-based generator)")


def _device_noise(like: torch.Tensor, seed: int, draw: int) -> torch.Tensor:
    """N(0, 1) of ``like``'s shape from the counter-based generator of csrc/philox.h, made on ``like``'s device in one launch: element i of the
    flattened tensor depends on (seed, draw, i) alone.  ``test_cfg['noise_source'] = 'device'``; there is no CPU path."""
    _require_device_latent(like)
    if like.numel() % 4:
        raise ValueError(f"noise_source='device': the latent's element count must be a multiple of 4, not {like.numel()}")
    out = torch.empty(like.shape, dtype=torch.float32, device=like.device)
    C.check(C.lib().ssdnerf_philox_normal_fill(C.ptr(out), C.ctypes.c_uint64(out.numel()), C.ctypes.c_uint64(int(seed) & _U64), C.u32(draw),
                                               C.stream()), "philox_normal_fill")
    return out


_U64 = (1 << 64) - 1
_SDE_FORM = {"ddim": 0, "langevin": 1, "ddpm": 2, "dpmpp": 2, "dpmpp_sde": 2}   # ``form`` of ssdnerf_sde_step_v per plan step kind


def _host_noise(like: torch.Tensor) -> torch.Tensor:
    """Fresh N(0, 1) drawn with the CPU generator and moved to the latent's device: seeding the host generator reproduces a trajectory on
    any device (mmgen's ``_get_noise_batch`` does the same).  The draw costs ~2 ns per value on the host (4.8 ms for 8 cars
    latents): callers issue it where the GPU has work queued (``_run_plan``, ``DiffusionNeRF.val_optim``), and the upload does not block (r04)."""
    if like.is_cuda:
        return _PinnedRing.upload(like.shape, like.device)
    return torch.randn(like.shape, dtype=torch.float32).to(like.device)


# ============================================================================================== the prior loss on device noise (csrc/prior_loss.hip)
_LOSS_DRAW_BASE = 1 << 31           # loss draws are numbered 0x80000000 | k: never one of the sampling draws 0, 1, 2, ... of ``_run_plan`` under the same seed
_PRIOR_DTYPES = {torch.float32: C.F32, torch.bfloat16: C.BF16}
_PRIOR_SLAB: Dict = {}              # (B, n_per) -> ssdnerf_prior_loss_partials(B, n_per), asked once per shape


def _prior_args(x0, a, b, seed, draw):
    B = x0.size(0)
    n_per = x0.numel() // B if B else 0
    return [C.ptr(a), C.ptr(b), C.u32(B), C.ctypes.c_uint64(n_per), C.ctypes.c_uint64(int(seed) & _U64), C.u32(draw)]


class _PriorQSample(torch.autograd.Function):
    """x_t = a_s x0 + b_s z, z the normals of (seed, draw) made in registers (``ssdnerf_prior_q_sample``); d x_t / d x0 = a_s.
    ``x0`` (B, ...) fp32 contiguous on the GPU, ``a`` / ``b`` (B,) fp32 contiguous."""

    @staticmethod
    def forward(ctx, x0, a, b, seed, draw):
        x_t = torch.empty_like(x0)
        C.check(C.lib().ssdnerf_prior_q_sample(C.ptr(x0), *_prior_args(x0, a, b, seed, draw), C.ptr(x_t), C.stream()), "prior_q_sample")
        ctx.save_for_backward(a)
        return x_t

    @staticmethod
    def backward(ctx, grad):
        (a,) = ctx.saved_tensors
        return grad * a.reshape(-1, *([1] * (grad.dim() - 1))), None, None, None, None


class _PriorLossV(torch.autograd.Function):
    """(msd, x0sq) per sample of the V-parameterised loss: msd = mean_i (pred - (a_s z - b_s x0))^2, x0sq = mean_i x0^2 (``ssdnerf_prior_loss_v``;
    x0sq carries no gradient: it feeds ``norm_factor`` only).  Backward: ``ssdnerf_prior_loss_v_backward`` recomputes the difference from the same
    (seed, draw); the gradient on x0 is the path through the target alone, the path through x_t belongs to ``_PriorQSample``."""

    @staticmethod
    def forward(ctx, pred, x0, a, b, seed, draw):
        B = x0.size(0)
        lib = C.lib()
        n_per = x0.numel() // B if B else 0
        if (B, n_per) not in _PRIOR_SLAB:
            _PRIOR_SLAB[B, n_per] = int(lib.ssdnerf_prior_loss_partials(B, n_per))
        buf = torch.empty(2 * B + _PRIOR_SLAB[B, n_per], dtype=torch.float32, device=x0.device)      # msd | x0sq | the slab of block partials: one allocation
        msd, x0sq, partials = buf[:B], buf[B:2 * B], buf[2 * B:]
        C.check(lib.ssdnerf_prior_loss_v(C.ptr(pred), _PRIOR_DTYPES[pred.dtype], C.ptr(x0), *_prior_args(x0, a, b, seed, draw), C.ptr(partials),
                                         C.ptr(msd), C.ptr(x0sq), C.stream()), "prior_loss_v")
        ctx.save_for_backward(pred, x0, a, b)
        ctx.seed, ctx.draw = seed, draw
        ctx.mark_non_differentiable(x0sq)
        return msd, x0sq

    @staticmethod
    def backward(ctx, grad_msd, _grad_x0sq):
        pred, x0, a, b = ctx.saved_tensors
        n_per = x0.numel() // x0.size(0) if x0.size(0) else 1
        k = (grad_msd.float() * (2.0 / n_per)).contiguous()
        grad_pred = torch.empty_like(pred)
        grad_x0 = torch.empty_like(x0) if ctx.needs_input_grad[1] else None
        C.check(C.lib().ssdnerf_prior_loss_v_backward(C.ptr(pred), _PRIOR_DTYPES[pred.dtype], C.ptr(x0), C.ptr(a), C.ptr(b), C.ptr(k),
                                                      *_prior_args(x0, a, b, ctx.seed, ctx.draw)[2:], C.ptr(grad_pred), C.ptr(grad_x0), C.stream()),
                "prior_loss_v_backward")
        return grad_pred, grad_x0, None, None, None, None


# ============================================================================================== schedule
class NoiseSchedule:
    """float64 tables of a T-step variance schedule (gaussian_diffusion.py:64-154).  ``kind``: 'linear' (betas from 1e-4 to 2e-2, rescaled by
    1000/T), 'cosine' (Nichol & Dhariwal), 'scaled_linear' (linear in sqrt(beta))."""

    def __init__(self, cfg: Dict, T: int):
        cfg = dict(cfg)
        self.kind = cfg.pop("type")
        self.T = T
        if self.kind == "linear":
            k = 1000 / T
            betas = np.linspace(k * cfg.get("beta_0", 1e-4), k * cfg.get("beta_T", 2e-2), T, dtype=np.float64)
        elif self.kind == "cosine":
            s, cap = cfg.get("s", 0.008), cfg.get("max_beta", 0.999)
            g = [math.cos((i / T + s) / (1 + s) * math.pi / 2) ** 2 for i in range(T + 1)]
            betas = np.array([min(1 - g[i + 1] / g[i], cap) for i in range(T)])
        elif self.kind == "scaled_linear":
            betas = np.linspace(cfg.get("beta_start", 1e-4) ** 0.5, cfg.get("beta_end", 2e-2) ** 0.5, T, dtype=np.float64) ** 2
        else:
            raise AttributeError(f"Unknown method name {self.kind} for beta schedule.")
        ab = np.cumprod(1.0 - betas, axis=0)
        ab_prev = np.append(1.0, ab[:-1])
        post_var = betas * (1 - ab_prev) / (1 - ab)                       # variance of q(x_{t-1} | x_t, x_0)
        self.tables = dict(
            betas=betas, alphas=1.0 - betas, alphas_bar=ab, alphas_bar_prev=ab_prev, alphas_bar_next=np.append(ab[1:], 0.0),
            sqrt_alphas_bar=np.sqrt(ab), sqrt_one_minus_alphas_bar=np.sqrt(1.0 - ab), log_one_minus_alphas_bar=np.log(1.0 - ab),
            sqrt_recip_alplas_bar=np.sqrt(1.0 / ab), sqrt_recipm1_alphas_bar=np.sqrt(1.0 / ab - 1), tilde_betas_t=post_var,
            log_tilde_betas_t_clipped=np.log(np.append(post_var[1], post_var[1:])),
            tilde_mu_t_coef1=np.sqrt(ab_prev) / (1 - ab) * betas, tilde_mu_t_coef2=np.sqrt(1.0 - betas) * (1 - ab_prev) / (1 - ab))
        self._dev: Dict = {}

    def __getitem__(self, name: str) -> np.ndarray:
        return self.tables[name]

    def signal_noise(self, device) -> torch.Tensor:
        """(2, T) fp32 on ``device``: row 0 sqrt(alpha_bar), row 1 sqrt(1 - alpha_bar); uploaded once per device, gathered by ``t`` tensors."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = torch.from_numpy(np.stack([self["sqrt_alphas_bar"], self["sqrt_one_minus_alphas_bar"]])).float().to(device)
        return self._dev[key]


@dataclass(frozen=True)
class PlanStep:
    """One network evaluation of a sampling trajectory; every coefficient is a host float resolved from the float64 tables.
    After x0 has been predicted at timestep ``t`` (signal ``a`` = sqrt(abar_t), noise level ``b`` = sqrt(1 - abar_t)), with
    eps = (x_t - a x0) / b, the latent becomes
        kind 'ddim'     :  c x0 + d eps + n z            (c = sqrt(abar_prev), d = sqrt(1 - abar_prev - eta^2 var), n = eta sqrt(var))
        kind 'langevin' :  x_t - d eps + n z             (d = delta b / 2, n = sqrt(delta) b)
        kind 'ddpm'     :  c x0 + d x_t + n z            (posterior mean coefficients, n = sqrt(var), 0 at t = 0)
        kind 'dpmpp'    :  c x0 + d x_t + e x0_prev      (DPM-Solver++(2M); x0_prev: the clipped x0 of the step before; see SamplingPlan)
        kind 'dpmpp_sde':  c x0 + d x_t + e x0_prev + n z   (SDE-DPM-Solver++(2M); n = 0 on the last step; see SamplingPlan)"""
    kind: str
    t: int
    a: float
    b: float
    c: float
    d: float
    n: float
    emit: bool            # a trajectory point of the reference's ``save_intermediates`` list (the DDIM steps, not the Langevin corrections)
    e: float = 0.0        # weight of the previous step's x0 (kinds 'dpmpp' and 'dpmpp_sde', second-order steps only)


def _ddim_step(sched: NoiseSchedule, t: int, t_prev: int, eta: float) -> PlanStep:
    """the 'ddim' step from ``t`` to ``t_prev`` (-1: past the last timestep, alpha_bar_prev[0] = 1)"""
    ab_prev = sched["alphas_bar"][t_prev] if t_prev >= 0 else sched["alphas_bar_prev"][0]
    var = sched["tilde_betas_t"][t]
    return PlanStep("ddim", t, float(sched["sqrt_alphas_bar"][t]), float(sched["sqrt_one_minus_alphas_bar"][t]), float(np.sqrt(ab_prev)),
                    float(np.sqrt(1 - ab_prev - var * eta ** 2)), float(eta * np.sqrt(var)), True)


def _langevin_step(sched: NoiseSchedule, t: int, delta: float) -> PlanStep:
    """one 'langevin' correction at ``t``"""
    sigma = float(sched["sqrt_one_minus_alphas_bar"][t])
    return PlanStep("langevin", t, float(sched["sqrt_alphas_bar"][t]), sigma, 0.0, 0.5 * delta * sigma, math.sqrt(delta) * sigma, False)


class SamplingPlan:
    """The whole trajectory of ``ddim_sample`` / ``ddpm_sample`` / ``dpmpp_2m_sample`` as a list of ``PlanStep``s (timesteps arange(T-1, -1,
    -T/n).long(): 50 -> 999, 979, ..., 19; 75 -> 999, 985, 972, ..., 12; the last DDIM step lands on alpha_bar_prev[0] = 1, i.e. x_prev = x0
    exactly, and so does the last step of 'dpmpp_2m' and 'dpmpp_2m_sde').  ``solver_order`` (1 or 2) belongs to those two alone."""

    def __init__(self, sched: NoiseSchedule, method: str, n: int, eta: float = 0.0, langevin_steps: int = 0, langevin_delta: float = 0.1,
                 langevin_t_range: Sequence[float] = (0, 1000), var_mode: str = "FIXED_LARGE", solver_order: int = 2):
        T = sched.T
        self.timesteps = torch.arange(start=T - 1, end=-1, step=-(T / n)).long()
        ts = self.timesteps.tolist()
        sa, sb, var = sched["sqrt_alphas_bar"], sched["sqrt_one_minus_alphas_bar"], sched["tilde_betas_t"]
        steps: List[PlanStep] = []
        if method == "ddim":
            for i, t in enumerate(ts):
                t_prev = ts[i + 1] if i + 1 < len(ts) else -1
                steps.append(_ddim_step(sched, t, t_prev, eta))
                if langevin_steps > 0 and langevin_t_range[0] < t_prev < langevin_t_range[1]:
                    steps += [_langevin_step(sched, t_prev, langevin_delta)] * langevin_steps
        elif method == "ddpm":
            mode = var_mode.upper()
            if mode == "FIXED_LARGE":
                table = np.append(var[1], sched["betas"])
            elif mode == "FIXED_SMALL":
                table = var
            else:
                raise AttributeError(f"Unknown denoising var output type [{var_mode}].")
            for t in ts:
                steps.append(PlanStep("ddpm", t, float(sa[t]), float(sb[t]), float(sched["tilde_mu_t_coef1"][t]), float(sched["tilde_mu_t_coef2"][t]),
                                      float(np.sqrt(table[t])) if t != 0 else 0.0, True))
        elif method in ("dpmpp_2m", "dpmpp_2m_sde"):
            # DPM-Solver++(2M) (Lu et al. 2022, data prediction): with lambda = log a - log b, h = lambda_prev - lambda_t, phi = -expm1(-h),
            #   x_prev = (b_prev / b_t) x_t + a_prev phi D,    D = x0 (first order)  or  (1 + 1/(2r)) x0 - (1/(2r)) x0_prev,  r = h_before / h.
            # The first-order step IS the eta = 0 DDIM step: a_prev phi = a_prev - b_prev a_t / b_t.  Same timesteps, one network evaluation each.
            # SDE-DPM-Solver++(2M) (the stochastic multistep form): the reverse SDE contracts x_t twice as fast as the ODE and the difference comes
            # back as fresh noise,
            #   x_prev = (b_prev / b_t) e^-h x_t + a_prev (1 - e^-2h) D + b_prev sqrt(1 - e^-2h) z,       D as above.
            # d^2 b_t^2 + n^2 = b_prev^2 (the noise level lands on the schedule) and c + e + d a_t = a_prev (so does the signal).  Its first-order step
            # IS the DDIM step with sigma^2 = (b_prev / b_t)^2 (1 - a_t^2 / a_prev^2), i.e. eta = 1.
            sde = method == "dpmpp_2m_sde"
            kind = "dpmpp_sde" if sde else "dpmpp"
            if solver_order not in (1, 2):
                raise ValueError(f"{method}: solver_order must be 1 or 2, not {solver_order!r}")
            if langevin_steps > 0:
                raise ValueError(f"{method}: Langevin corrections move x_t between the two history points of a multistep update (langevin_steps must be 0)")
            if eta != 0:
                reason = "has no eta: its noise level is the solver's own" if sde else "is the deterministic solver"
                raise ValueError(f"{method} {reason} (eta must be 0)")
            lam = np.log(sa) - np.log(sb)
            h_before = None
            for i, t in enumerate(ts):
                if i + 1 == len(ts):                                         # t_prev = -1: abar_prev = 1, lambda_prev = inf, phi = 1: x_prev = x0 exactly, no noise
                    steps.append(PlanStep(kind, t, float(sa[t]), float(sb[t]), 1.0, 0.0, 0.0, True, 0.0))
                    break
                t_prev = ts[i + 1]
                h = lam[t_prev] - lam[t]
                base = sa[t_prev] * -np.expm1(-2 * h if sde else -h)
                c, e = base, 0.0
                if solver_order == 2 and h_before is not None:
                    r = h_before / h
                    c, e = base * (1 + 1 / (2 * r)), -base / (2 * r)
                d, n_coef = sb[t_prev] / sb[t], 0.0
                if sde:
                    d, n_coef = d * np.exp(-h), sb[t_prev] * np.sqrt(-np.expm1(-2 * h))
                steps.append(PlanStep(kind, t, float(sa[t]), float(sb[t]), float(c), float(d), float(n_coef), True, float(e)))
                h_before = h
        else:
            raise AttributeError(f"Cannot find sample method [{method}_sample] correspond to [{method}].")
        self.steps = steps

    def __len__(self):
        return len(self.steps)

    def __iter__(self):
        return iter(self.steps)


# ============================================================================================== timestep samplers
@MODULES.register_module()
class UniformTimeStepSampler:
    """t ~ Categorical(prob) drawn with ``np.random`` on the HOST (mmgen's sampler): a seeded ``np.random`` yields the
    same timesteps whatever device the model lives on."""

    def __init__(self, num_timesteps, **kwargs):
        self.num_timesteps = num_timesteps
        self.prob = [1 / num_timesteps] * num_timesteps

    def sample(self, batch_size):
        return torch.from_numpy(np.random.choice(self.num_timesteps, size=(batch_size,), p=self.prob)).long()

    __call__ = sample


MODULES.register_module(name="UniformTimeStepSamplerMod", module=type("UniformTimeStepSamplerMod", (UniformTimeStepSampler,), {}))


@MODULES.register_module()
class SNRWeightedTimeStepSampler(UniformTimeStepSampler):
    """Loss weight per timestep = clip(SNR^power + bias) converted to the network's output parameterisation (x0-, eps- or v-prediction), and
    sampling density proportional to weight^prob_power (sampler.py:14-44).  ``mean`` / ``std``: float64 sqrt(abar), sqrt(1 - abar)."""

    _to_output_space = {"START_X": lambda w, m, s: w, "EPS": lambda w, m, s: w * (s / m) ** 2, "V": lambda w, m, s: w * (s ** 2)}

    def __init__(self, num_timesteps, mean, std, mode, power=1, min=-1, max=-1, bias=0, prob_power=0.0):
        self.num_timesteps = num_timesteps
        m, s = np.asarray(mean, np.float64), np.asarray(std, np.float64)
        w_x0 = (m / s) ** (2 * power) + bias
        lo, hi = (min if min > 0 else None), (max if max > 0 else None)
        if lo is not None or hi is not None:
            w_x0 = w_x0.clip(min=lo, max=hi)
        if mode not in self._to_output_space:
            raise AttributeError(f"unknown denoising mean mode {mode!r}")
        w_out = self._to_output_space[mode](w_x0, m, s)
        density = w_out ** prob_power
        density = density / density.sum()
        self.weight = torch.from_numpy(w_out / (density * num_timesteps)).to(torch.float)      # importance-corrected loss weight
        self.prob = density.tolist()


# ============================================================================================== diffusion prior loss
@MODULES.register_module()
class DDPMMSELossMod(nn.Module):
    """Per-sample ``0.5 * mean((pred - target)^2)`` x ``weight[t] * weight_scale`` (``rescale_mode='timestep_weight'``; the table comes from
    the timestep sampler), batch-reduced, optionally divided by ``norm_factor`` -- a running mean of mean(x_0^2) that only moves in training
    mode (ddpm_loss.py:11-142 over mmgen's ``DDPMLoss``).  ``log_vars``: per-quartile means as 0-dim DEVICE tensors (the reference calls
    ``.item()`` per quartile: four syncs per loss)."""

    _default_data_info = dict(pred="eps_t_pred", target="noise")
    _reductions = {"mean": lambda v: v.mean(), "sum": lambda v: v.sum(), "none": lambda v: v,
                   "flatmean": lambda v: v.flatten(1).mean(dim=1) if v.dim() > 1 else v}

    def __init__(self, rescale_mode=None, rescale_cfg=None, sampler=None, weight=None, weight_scale=1.0, log_cfgs=None, reduction="mean",
                 data_info=None, loss_name="loss_ddpm_mse", scale_norm=False, momentum=0.001):
        super().__init__()
        if reduction not in self._reductions:
            raise ValueError(reduction)
        self.weight_scale, self.reduction, self.loss_name_, self.momentum = weight_scale, reduction, loss_name, momentum
        self.data_info = dict(data_info or self._default_data_info)
        self.rescale_mode, self.timestep_weight = rescale_mode, None
        if rescale_mode == "timestep_weight":
            table = getattr(sampler, "weight", None) if sampler is not None else None
            table = weight if table is None else table
            if table is None:
                raise ValueError("rescale_mode='timestep_weight' needs a sampler with a weight table, or an explicit weight")
            self.timestep_weight = torch.as_tensor(table, dtype=torch.float)
        elif rescale_mode is not None:
            raise NotImplementedError(f"rescale_mode={rescale_mode!r}: the reference's configs only use 'timestep_weight'")
        self.log_cfgs = [log_cfgs] if isinstance(log_cfgs, dict) else list(log_cfgs or [])
        self.log_vars: Dict[str, torch.Tensor] = {}
        self.scale_norm, self.freeze_norm = scale_norm, False
        if scale_norm:
            self.register_buffer("norm_factor", torch.ones(1, dtype=torch.float))

    def _quartile_log(self, per_sample, timesteps):
        self.log_vars = {}
        for cfg in self.log_cfgs:
            if cfg.get("type") != "quartile":
                continue
            which = (timesteps.float() / cfg.get("total_timesteps", 1000) * 4).long()
            onehot = torch.nn.functional.one_hot(which.clamp(0, 3), 4).to(per_sample.dtype)             # (B, 4): no host round trip
            means = (per_sample.detach()[:, None] * onehot).sum(0) / onehot.sum(0).clamp(min=1)
            for q in range(4):
                self.log_vars[f"{cfg.get('prefix_name', 'loss')}_quartile_{q}"] = means[q]

    def forward(self, output_dict):
        assert isinstance(output_dict, dict) and "timesteps" in output_dict, "DDPM losses take the dict of network outputs with 'timesteps'"
        diff = output_dict[self.data_info["pred"]] - output_dict[self.data_info["target"]]
        return self._from_msd(diff.square().flatten(1).mean(dim=1), output_dict["timesteps"], lambda: output_dict["x_0"].detach().square().mean())

    def forward_msd(self, msd, timesteps, x0sq):
        """``forward`` from the per-sample reductions alone: ``msd`` (B,) = mean_i (pred - target)^2 and ``x0sq`` (B,) = mean_i x_0^2 per sample, as the
        fused kernels of csrc/prior_loss.hip return them (``norm_factor`` is fed ``x0sq.mean()``).  Everything behind the mean is ``forward``'s own code."""
        return self._from_msd(msd, timesteps, lambda: x0sq.detach().mean())

    def _from_msd(self, msd, t, x0_square_mean):
        per_sample = msd * 0.5
        if self.timestep_weight is not None:
            if self.timestep_weight.device != t.device:
                self.timestep_weight = self.timestep_weight.to(t.device)                                 # moved once, not per call
            per_sample = per_sample * self.timestep_weight[t] * self.weight_scale
        self._quartile_log(per_sample, t)
        loss = self._reductions[self.reduction](per_sample)
        if self.scale_norm:
            if self.training and not self.freeze_norm:
                from .parallel import reduce_mean
                self.norm_factor.mul_(1 - self.momentum).add_(self.momentum * reduce_mean(x0_square_mean()))
            loss = loss / self.norm_factor
        return loss


MODULES.register_module(name="DDPMMSELoss", module=type("DDPMMSELoss", (DDPMMSELossMod,), {}))


# ============================================================================================== the diffusion model
_FROM_X0 = {  # network output that corresponds to a given x0 (used when guidance has moved x0 and the loss wants the matching output)
    "EPS": lambda x_t, x0, a, b: (x_t - x0 * a) / b,
    "START_X": lambda x_t, x0, a, b: x0,
    "V": lambda x_t, x0, a, b: (a * x_t - x0) / b,
}
_TO_X0 = {
    "EPS": lambda x_t, out, a, b: (x_t - b * out) / a,
    "START_X": lambda x_t, out, a, b: out,
    "V": lambda x_t, out, a, b: a * x_t - b * out,
}


@MODULES.register_module()
class GaussianDiffusion(nn.Module):
    def __init__(self, denoising, ddpm_loss=dict(type="DDPMMSELoss", log_cfgs=dict(type="quartile", prefix_name="loss_mse", total_timesteps=1000)),
                 betas_cfg=dict(type="cosine"), num_timesteps=1000, num_classes=0, sample_method="ddim",
                 timestep_sampler=dict(type="UniformTimeStepSampler"), denoising_var_mode="FIXED_LARGE", denoising_mean_mode="V", train_cfg=None,
                 test_cfg=None):
        super().__init__()
        self.num_classes, self.num_timesteps, self.sample_method = num_classes, num_timesteps, sample_method
        self._denoising_cfg = deepcopy(denoising)
        self.denoising = build_module(denoising, default_args=dict(num_classes=num_classes, num_timesteps=num_timesteps))
        self.denoising_var_mode, self.denoising_mean_mode = denoising_var_mode, denoising_mean_mode
        if denoising_mean_mode.upper() not in _TO_X0:
            raise AttributeError(f"Unknown denoising mean output type [{denoising_mean_mode}].")
        self.betas_cfg = deepcopy(betas_cfg)
        self.train_cfg = deepcopy(train_cfg) if train_cfg is not None else dict()
        self.test_cfg = deepcopy(test_cfg) if test_cfg is not None else dict()
        self.schedule = NoiseSchedule(self.betas_cfg, num_timesteps)
        self.betas_schedule = self.schedule.kind
        self.sampler = build_module(timestep_sampler or dict(type="UniformTimeStepSampler"),
                                    default_args=dict(num_timesteps=num_timesteps, mean=self.schedule["sqrt_alphas_bar"],
                                                      std=self.schedule["sqrt_one_minus_alphas_bar"], mode=self.denoising_mean_mode))
        self.ddpm_loss = build_module(ddpm_loss or dict(type="DDPMMSELoss"), default_args=dict(sampler=self.sampler))
        self.use_fused_step = True          # False: every step through the generic tensor expressions (parity runs)
        self._plans: Dict = {}

    def __getattr__(self, name):
        # the schedule tables under the reference's attribute names (``betas``, ``alphas_bar``, ``sqrt_alphas_bar``, ``tilde_betas_t`` ...)
        if name != "schedule" and "schedule" in self.__dict__ and name in self.__dict__["schedule"].tables:
            return self.__dict__["schedule"].tables[name]
        return super().__getattr__(name)

    # ------------------------------------------------------------------------------------------ plans
    def ddim_timesteps(self, num_timesteps=None):
        n = self.test_cfg.get("num_timesteps", self.num_timesteps) if num_timesteps is None else num_timesteps
        return torch.arange(start=self.num_timesteps - 1, end=-1, step=-(self.num_timesteps / n)).long()

    def sampling_plan(self, method="ddim", cfg=None) -> SamplingPlan:
        cfg = self.test_cfg if cfg is None else cfg
        key = (method, cfg.get("num_timesteps", self.num_timesteps), cfg.get("eta", 0), cfg.get("langevin_steps", 0), cfg.get("langevin_delta", 0.1),
               tuple(cfg.get("langevin_t_range", [0, 1000])), self.denoising_var_mode, cfg.get("solver_order", 2))
        if key not in self._plans:
            self._plans[key] = SamplingPlan(self.schedule, *key)
        return self._plans[key]

    # ------------------------------------------------------------------------------------------ forward process
    def q_sample(self, x_0, t, noise=None):
        """x_t = a[t] x_0 + b[t] noise and the two broadcastable coefficient tensors (a = sqrt(abar), b = sqrt(1 - abar))."""
        noise = _host_noise(x_0) if noise is None else noise
        ab = self.schedule.signal_noise(x_0.device)[:, torch.as_tensor(t, device=x_0.device).reshape(-1)]
        a, b = ab[0].reshape(-1, 1, 1, 1), ab[1].reshape(-1, 1, 1, 1)
        return x_0 * a + noise * b, a, b

    # ------------------------------------------------------------------------------------------ x0 prediction (+ guidance)
    def pred_x_0(self, x_t, t, grad_guide_fn=None, concat_cond=None, cfg=dict(), update_denoising_output=False):
        """x0 predicted from (x_t, t) -- clipped to ``clip_range`` -- and the network output.  With a guidance closure ``grad_guide_fn(x0) ->
        scalar loss``: x0 <- x0 - grad * b^(2 - 2w) a^(2w - 1) * gain, where the gradient is taken w.r.t. x_t THROUGH the UNet
        (``grad_through_unet``, default) or w.r.t. x0 directly, and w = ``snr_weight_power`` (gaussian_diffusion.py:180-240)."""
        clip = cfg.get("clip_range", [-1, 1]) if cfg.get("clip_denoised", True) else None
        t = torch.as_tensor(t, device=x_t.device)
        if t.dim() == 0 or t.numel() != x_t.size(0):
            t = t.expand(x_t.size(0))
        ab = self.schedule.signal_noise(x_t.device)[:, t]
        a, b = ab[0].reshape(-1, 1, 1, 1), ab[1].reshape(-1, 1, 1, 1)
        mode = self.denoising_mean_mode.upper()
        if grad_guide_fn is None:
            out = self.denoising(x_t, t, concat_cond=concat_cond)
            x0 = _TO_X0[mode](x_t, out, a, b)
            return (x0.clamp(*clip) if clip else x0), out

        through_unet = cfg.get("grad_through_unet", True)
        w = cfg.get("snr_weight_power", 0.5)
        if through_unet:
            with torch.enable_grad():
                # sampling hands a detached latent in (under no_grad): make it a leaf.  A latent that already carries a graph (the prior loss
                # with guidance, x_t = q_sample(code)) stays IN that graph, so the UNet-path gradient still reaches the code.
                if not x_t.requires_grad:
                    x_t = x_t.detach().requires_grad_(True)
                out = self.denoising(x_t, t, concat_cond=concat_cond)
                x0 = _TO_X0[mode](x_t, out, a, b)
                if clip:
                    x0 = x0.clamp(*clip)
                (grad,) = torch.autograd.grad(grad_guide_fn(x0), x_t, retain_graph=x_t.grad_fn is not None)
        else:
            out = self.denoising(x_t, t, concat_cond=concat_cond)
            x0 = _TO_X0[mode](x_t, out, a, b)
            if clip:
                x0 = x0.clamp(*clip)
            with torch.enable_grad():
                x0 = x0.detach().requires_grad_(True)
                (grad,) = torch.autograd.grad(grad_guide_fn(x0), x0)
        x0 = x0.detach() - grad * (b ** (2 - 2 * w) * a ** (2 * w - 1) * cfg.get("guidance_gain", 1.0))
        if clip:
            x0 = x0.clamp(*clip)
        if update_denoising_output:
            out = _FROM_X0[mode](x_t, x0, a, b)
        return x0, out

    # ------------------------------------------------------------------------------------------ sampling
    def _advance(self, s: PlanStep, x_t, x0, noise=None, x0_prev=None, host_draw=True):
        """the latent after plan step ``s`` (see PlanStep).  ``host_draw`` False (device noise): a step whose ``noise`` is None adds none."""
        if _SDE_FORM[s.kind] == 2:                                           # 'ddpm', 'dpmpp', 'dpmpp_sde' (e != 0: a second-order step of the last two)
            x = s.c * x0 + s.d * x_t
            if s.e != 0:
                x = x + s.e * x0_prev
        else:
            eps = (x_t - s.a * x0) / s.b
            x = s.c * x0 + s.d * eps if s.kind == "ddim" else x_t - s.d * eps
        if s.n != 0 or s.kind == "ddpm":                                     # (the ancestral sampler draws at t = 0 too and multiplies by 0)
            if noise is None and not host_draw:
                return x
            x = x + s.n * (_host_noise(x_t) if noise is None else noise)
        return x

    def _noise_source(self, cfg, x_t):
        """(device mode?, seed) of one sampling call.  Device mode without ``noise_seed``: ONE draw of 64 bits from torch's default CPU generator, so
        ``torch.manual_seed`` still reproduces the run."""
        source = cfg.get("noise_source", "host")
        if source not in ("host", "device"):
            raise ValueError(f"test_cfg['noise_source'] must be 'host' or 'device', not {source!r}")
        if source == "host":
            return False, 0
        _require_device_latent(x_t)
        seed = cfg.get("noise_seed")
        if seed is None:
            lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
            seed = (hi << 32) | lo
        return True, int(seed) & _U64

    def _fused_ok(self, x_t, cfg, grad_guide_fn, concat_cond):
        return (self.use_fused_step and grad_guide_fn is None and concat_cond is None and self.denoising_mean_mode.upper() == "V" and x_t.is_cuda
                and x_t.dtype == torch.float32 and cfg.get("clip_denoised", True) and not torch.is_grad_enabled())

    def _run_plan(self, plan: SamplingPlan, noise, concat_cond=None, save_intermediates=False, grad_guide_fn=None, **kwargs):
        cfg = self.test_cfg
        x_t = noise
        device_noise, seed = self._noise_source(cfg, x_t)
        draw = 0                                                             # device mode: draws are numbered in plan order; a step with n == 0 consumes none
        B = x_t.size(0)
        kept: Optional[list] = [] if save_intermediates else None
        t_rows = torch.tensor([s.t for s in plan], dtype=torch.long).to(x_t.device)[:, None].expand(-1, B).contiguous()   # ONE upload for the loop
        clip = cfg.get("clip_range", [-1, 1])
        session = None
        if self._fused_ok(x_t, cfg, grad_guide_fn, concat_cond) and hasattr(self.denoising, "inference_session"):
            session = self.denoising.inference_session(x_t, t_rows[0])
            if session is not None:
                session.x.copy_(x_t)                                         # the latent lives in the UNet's static input buffer from here on
        history, x0_prev = None, None                                        # multistep kinds: the two alternating x0 buffers of the fused step / the generic branch's last x0
        pending_x0 = None                                                    # x0 of the last emitting (DDIM) step; its trajectory point is the latent AFTER
                                                                             # the Langevin corrections that follow it (gaussian_diffusion.py:313-326)
        for i, s in enumerate(plan):
            cond = concat_cond[:, i % concat_cond.size(1)] if concat_cond is not None else None
            if kept is not None and s.emit and pending_x0 is not None:
                kept += [pending_x0, session.x.clone() if session is not None else x_t]
                pending_x0 = None
            if session is not None and (device_noise or s.kind == "dpmpp" or (s.kind == "ddim" and s.n == 0)):
                # ---- device-resident step: t -> static buffer, graph replay, ONE fused update written back in place.  Under device noise that is a step
                # of any kind, its normals made in registers by the update itself; a step that injects none keeps the deterministic entry and consumes no
                # draw index.  The multistep kinds leave x0 in one of two alternating buffers and read the other, where the step before left its own.
                session.t.copy_(t_rows[i])
                v = session.run()
                multistep, prev = s.kind in ("dpmpp", "dpmpp_sde"), None
                if multistep:
                    if history is None:
                        history = [torch.empty_like(session.x), torch.empty_like(session.x)]     # allocated once per call
                    x0, prev = history[i & 1], (history[(i & 1) ^ 1] if s.e != 0 else None)
                else:
                    x0 = torch.empty_like(session.x) if kept is not None and s.emit else session.y   # (x0 is only materialised when the caller keeps it)
                x, n_el, lo, hi = C.ptr(session.x), C.ctypes.c_uint64(v.numel()), C.f32(clip[0]), C.f32(clip[1])
                if s.kind == "ddim" and s.n == 0:
                    C.check(C.lib().ssdnerf_ddim_step_v(x, C.ptr(v), n_el, C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d), lo, hi, C.ptr(x0), x, C.stream()),
                            "ddim_step_v")
                elif s.kind == "dpmpp" or (s.n == 0 and _SDE_FORM[s.kind] == 2):
                    C.check(C.lib().ssdnerf_dpmpp_step_v(x, C.ptr(v), C.ptr(prev), n_el, C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d), C.f32(s.e), lo, hi,
                                                         C.ptr(x0), x, C.stream()), "dpmpp_step_v")
                else:
                    C.check(C.lib().ssdnerf_sde_step_v(x, C.ptr(v), C.ptr(prev), n_el, _SDE_FORM[s.kind], C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d),
                                                       C.f32(s.e), C.f32(s.n), lo, hi, C.ctypes.c_uint64(seed), C.u32(draw), C.ptr(x0), x, C.stream()),
                            "sde_step_v")
                    draw += s.n != 0
                if kept is not None and s.emit:
                    pending_x0 = x0.clone() if multistep else x0                 # (a history buffer is written again two steps on)
                continue
            if session is not None:                                          # a step kind the fused form does not cover: leave the session
                x_t, session = session.x.clone(), None
            # a step that injects noise (Langevin, ancestral DDPM, eta > 0): the HOST draw first -- the device still has the previous step's work queued, the
            # draw (4.8 ms for 8 cars latents) hides under it; same generator, same order of draws as drawing inside _advance
            if device_noise:                                                 # the same normals as the fused step's: (seed, draw, element index)
                step_noise = _device_noise(x_t, seed, draw) if s.n != 0 else None
                draw += s.n != 0
            else:
                step_noise = _host_noise(x_t) if (s.n != 0 or s.kind == "ddpm") else None
            x0, _ = self.pred_x_0(x_t, t_rows[i], grad_guide_fn=grad_guide_fn, concat_cond=cond, cfg=cfg, **kwargs)
            x_t = self._advance(s, x_t.detach() if grad_guide_fn is not None else x_t, x0, noise=step_noise, x0_prev=x0_prev,
                                host_draw=not device_noise)
            if s.kind in ("dpmpp", "dpmpp_sde"):
                x0_prev = x0                                                 # (with guidance: the guided, clipped x0 that pred_x_0 returned)
            if kept is not None and s.emit:
                pending_x0 = x0
        if session is not None:
            x_t = session.x.clone()
        if pending_x0 is not None:
            kept += [pending_x0, x_t]
        return kept if save_intermediates else x_t

    def ddim_sample(self, noise, show_pbar=False, concat_cond=None, save_intermediates=False, **kwargs):
        return self._run_plan(self.sampling_plan("ddim"), noise, concat_cond, save_intermediates, **kwargs)

    def ddpm_sample(self, noise, show_pbar=False, concat_cond=None, **kwargs):
        return self._run_plan(self.sampling_plan("ddpm"), noise, concat_cond, False, **kwargs)

    def dpmpp_2m_sample(self, noise, show_pbar=False, concat_cond=None, save_intermediates=False, **kwargs):
        """DPM-Solver++(2M) over the DDIM timesteps (not in the reference; opt in with ``test_cfg['sample_method'] = 'dpmpp_2m'`` or the constructor's
        ``sample_method``): the same network evaluation, x0 prediction, clipping and guidance hook per step as ``ddim_sample``, a second-order update
        from the last two x0.  ``test_cfg['solver_order']`` 1 gives DDIM's own trajectory."""
        return self._run_plan(self.sampling_plan("dpmpp_2m"), noise, concat_cond, save_intermediates, **kwargs)

    def dpmpp_2m_sde_sample(self, noise, show_pbar=False, concat_cond=None, save_intermediates=False, **kwargs):
        """SDE-DPM-Solver++(2M) over the DDIM timesteps (not in the reference; opt in with ``test_cfg['sample_method'] = 'dpmpp_2m_sde'`` or the
        constructor's ``sample_method``): ``dpmpp_2m_sample``'s evaluation, clipping, guidance hook and history, with the solver's own noise added on
        every step but the last.  ``test_cfg['noise_source']`` decides where that noise comes from, as for every stochastic sampler here."""
        return self._run_plan(self.sampling_plan("dpmpp_2m_sde"), noise, concat_cond, save_intermediates, **kwargs)

    # single-step entry points of the reference API (each resolves its coefficients like one plan entry)
    def p_sample_ddim(self, x_t, t, t_prev, noise=None, cfg=dict(), grad_guide_fn=None, noise_seed=None, noise_draw=0, **kwargs):
        """``noise_seed`` (extra, with ``noise_draw``; also on the two entry points below): without ``noise``, take it from the device generator
        instead of the host draw"""
        t = int(t)
        s = _ddim_step(self.schedule, t, int(t_prev), cfg.get("eta", 0))
        x0, _ = self.pred_x_0(x_t, t, grad_guide_fn=grad_guide_fn, cfg=cfg, **kwargs)
        return self._advance(s, x_t, x0, self._seeded(s, x_t, noise, noise_seed, noise_draw)), x0

    def _seeded(self, s, x_t, noise, noise_seed, noise_draw):
        if noise is None and noise_seed is not None and (s.n != 0 or s.kind == "ddpm"):
            return _device_noise(x_t, noise_seed, noise_draw)
        return noise

    def p_sample_langevin(self, x_t, t, noise=None, cfg=dict(), grad_guide_fn=None, noise_seed=None, noise_draw=0, **kwargs):
        t = int(t)
        s = _langevin_step(self.schedule, t, cfg.get("langevin_delta", 0.1))
        x0, _ = self.pred_x_0(x_t, t, grad_guide_fn=grad_guide_fn, cfg=cfg, **kwargs)
        return self._advance(s, x_t, x0, self._seeded(s, x_t, noise, noise_seed, noise_draw))

    def q_posterior_mean(self, x_0, x_t, t):
        idx = torch.as_tensor(t).reshape(-1).cpu().numpy()
        c1 = x_0.new_tensor(self.schedule["tilde_mu_t_coef1"][idx], dtype=torch.float32).reshape(-1, 1, 1, 1)
        c2 = x_0.new_tensor(self.schedule["tilde_mu_t_coef2"][idx], dtype=torch.float32).reshape(-1, 1, 1, 1)
        return c1 * x_0 + c2 * x_t

    def p_sample_ddpm(self, x_t, t, noise=None, cfg=dict(), grad_guide_fn=None, noise_seed=None, noise_draw=0, **kwargs):
        key = ("ddpm-every-t", self.denoising_var_mode)
        if key not in self._plans:
            self._plans[key] = SamplingPlan(self.schedule, "ddpm", self.num_timesteps, var_mode=self.denoising_var_mode)   # every t once
        s = self._plans[key].steps[self.num_timesteps - 1 - int(t)]
        x0, _ = self.pred_x_0(x_t, int(t), grad_guide_fn=grad_guide_fn, cfg=cfg, **kwargs)
        return self._advance(s, x_t, x0, self._seeded(s, x_t, noise, noise_seed, noise_draw)), x0

    def sample_from_noise(self, noise, **kwargs):
        name = self.test_cfg.get("sample_method", self.sample_method)       # (no config of the reference sets the test_cfg key)
        method = name.lower()
        if method not in ("ddim", "ddpm", "dpmpp_2m", "dpmpp_2m_sde"):
            raise AttributeError(f"Cannot find sample method [{method}_sample] correspond to [{name}].")
        return getattr(self, f"{method}_sample")(noise=noise, **kwargs)

    # ------------------------------------------------------------------------------------------ prior loss
    def loss(self, denoising_output, x_0, noise, t, mean, std):
        key = {"EPS": "eps_t_pred", "START_X": "x_0_pred", "V": "v_t_pred"}[self.denoising_mean_mode.upper()]
        fields = {key: denoising_output, "x_0": x_0, "noise": noise, "timesteps": t}
        if key == "v_t_pred":
            fields["v_t"] = mean * noise - std * x_0
        return self.ddpm_loss(fields)

    def _loss_draw(self, cfg, noise_seed, noise_draw):
        """(seed, draw) of one device-mode loss call.  Seed: ``cfg['noise_seed']`` plus the ``torch.distributed`` rank (mod 2^64) when set; otherwise ONE
        64-bit draw from torch's CPU generator at this object's first such call, kept for its life, so ``torch.manual_seed`` reproduces a run.  Draw:
        0x80000000 | k, k counting this object's earlier counted calls under the current seed.  ``noise_seed`` / ``noise_draw`` override either and
        leave the counter alone when both are given.  The counter is plain Python state: it is NOT in the state dict, a resumed run starts at k = 0."""
        seed = noise_seed
        if seed is None:
            seed = cfg.get("noise_seed")
            if seed is not None:
                dist = torch.distributed
                seed = int(seed) + (dist.get_rank() if dist.is_available() and dist.is_initialized() else 0)
            else:
                if self.__dict__.get("_loss_own_seed") is None:
                    lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
                    self.__dict__["_loss_own_seed"] = (hi << 32) | lo
                seed = self.__dict__["_loss_own_seed"]
        seed = int(seed) & _U64
        if noise_draw is not None:
            return seed, int(noise_draw)
        at, k = self.__dict__.get("_loss_draws", (None, 0))
        k = k if at == seed else 0
        if k >= _LOSS_DRAW_BASE:
            raise RuntimeError("noise_source='device': 2^31 loss draws under one seed are used up; set another test_cfg / train_cfg 'noise_seed'")
        self.__dict__["_loss_draws"] = (seed, k + 1)
        return seed, _LOSS_DRAW_BASE | k

    def _forward_train_device(self, x_0, t, seed, draw, concat_cond, grad_guide_fn, x_t_detach):
        """the prior loss on device noise.  Fused route (V mode, no guidance, no conditioning, fp32 latent with n_per % 4 == 0, ``use_fused_step``):
        ``ssdnerf_prior_q_sample`` -> UNet -> ``ssdnerf_prior_loss_v`` (fp32 or bf16 output), the noise never in memory; everything else -- and a UNet
        output of another dtype -- goes through the tensor expressions of the host path on ``_device_noise``: the same normals, bit for bit."""
        B = x_0.size(0)
        v_loss = hasattr(self.ddpm_loss, "forward_msd") and self.ddpm_loss.data_info == dict(pred="v_t_pred", target="v_t")
        fused = (self.use_fused_step and self.denoising_mean_mode.upper() == "V" and v_loss and grad_guide_fn is None and concat_cond is None
                 and x_0.is_cuda and x_0.dtype == torch.float32 and B > 0 and (x_0.numel() // B) % 4 == 0)
        if not fused:
            return None
        ab = self.schedule.signal_noise(x_0.device)[:, t]
        a, b = ab[0].contiguous(), ab[1].contiguous()
        x_0 = x_0.contiguous()
        x_t = _PriorQSample.apply(x_0.detach() if x_t_detach else x_0, a, b, seed, draw)
        out = self.denoising(x_t, t, concat_cond=None)
        if out.dtype in _PRIOR_DTYPES:
            msd, x0sq = _PriorLossV.apply(out.contiguous(), x_0, a, b, seed, draw)
            return self.ddpm_loss.forward_msd(msd, t, x0sq)
        return self.loss(out, x_0, _device_noise(x_0, seed, draw), t, a.reshape(-1, 1, 1, 1), b.reshape(-1, 1, 1, 1))

    def forward_train(self, x_0, concat_cond=None, grad_guide_fn=None, cfg=dict(), x_t_detach=False, timesteps=None, noise=None, noise_seed=None,
                      noise_draw=None, **kwargs):
        """Diffusion prior loss of ``x_0`` (gaussian_diffusion.py:407-433).  ``timesteps`` / ``noise`` (extra): injected draws; by default both
        are drawn on the host like the reference's, so seeding reproduces them on any device.  ``log_vars['loss_ddpm_mse']`` is a detached
        0-dim tensor, not a Python float (no device sync here).
        ``cfg['noise_source'] = 'device'`` (opt-in; ``train_step`` hands in ``train_cfg``, ``val_optim`` and ``_refine_under_prior`` ``test_cfg``): the
        noise comes from the counter-based generator under ``_loss_draw``'s (seed, draw) -- ``noise_seed`` / ``noise_draw`` (extra) name them for tests
        and parity runs -- and the loss around the UNet runs in the kernels of csrc/prior_loss.hip (``_forward_train_device``).  Timesteps stay the
        sampler's host draw; an injected ``noise`` always wins."""
        assert x_0.dim() == 4
        dev = x_0.device
        source = cfg.get("noise_source", "host")
        if source not in ("host", "device"):
            raise ValueError(f"cfg['noise_source'] must be 'host' or 'device', not {source!r}")
        if noise is None and (source == "device" or noise_seed is not None):
            _require_device_latent(x_0)
            t = (self.sampler(x_0.size(0)) if timesteps is None else torch.as_tensor(timesteps).long()).to(dev)
            seed, draw = self._loss_draw(cfg, noise_seed, noise_draw)
            value = self._forward_train_device(x_0, t, seed, draw, concat_cond, grad_guide_fn, x_t_detach)
            if value is not None:
                log_vars = self.ddpm_loss.log_vars
                log_vars.update(loss_ddpm_mse=value.detach())
                return value, log_vars
            noise, timesteps = _device_noise(x_0, seed, draw), t
        t = (self.sampler(x_0.size(0)) if timesteps is None else torch.as_tensor(timesteps).long()).to(dev)
        noise = (_host_noise(x_0) if noise is None else noise).to(dev)
        x_t, a, b = self.q_sample(x_0, t, noise)
        if x_t_detach:
            x_t = x_t.detach()
        _, out = self.pred_x_0(x_t, t, grad_guide_fn=grad_guide_fn, concat_cond=concat_cond, cfg=cfg, update_denoising_output=True)
        value = self.loss(out, x_0, noise, t, a, b)
        log_vars = self.ddpm_loss.log_vars
        log_vars.update(loss_ddpm_mse=value.detach())
        return value, log_vars

    def forward_test(self, data, **kwargs):
        assert data.dim() == 4
        return self.sample_from_noise(data, **kwargs)

    def forward(self, data, return_loss=False, **kwargs):
        return self.forward_train(data, **kwargs) if return_loss else self.forward_test(data, **kwargs)
