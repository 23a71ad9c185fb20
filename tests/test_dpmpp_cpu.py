"""CPU tests of the DPM-Solver++(2M) sampler (``SamplingPlan`` method 'dpmpp_2m', ``GaussianDiffusion.dpmpp_2m_sample``, the generic branch of
``_run_plan``) and of the error bounds tests/test_dpmpp_gpu.py holds csrc/sampler_step.hip to: the plan's coefficients against a float64 restatement,
first order == DDIM, the bounds accept an fp32 emulation of the kernel and reject wrong ones, convergence on a prior whose probability-flow ODE
has a closed form, guidance, refusals, and the existing plans unchanged."""
import numpy as np
import pytest
import torch

import _dpmpp_ref as DR

SCHEDULES = ("linear", "cosine")


def _schedule(kind):
    from ssdnerf_amd.diffusion import NoiseSchedule
    return NoiseSchedule(dict(type=kind), 1000)


def _tiny_unet_cfg():
    return dict(type="DenoisingUnetMod", image_size=16, in_channels=18, base_channels=32, channels_cfg=[1, 2], resblocks_per_downsample=1,
                dropout=0.0, use_scale_shift_norm=True, downsample_conv=True, upsample_conv=True, num_heads=4, attention_res=[8],
                norm_cfg=dict(type="GN", num_groups=8))


_DIFFUSIONS = {}


def _diffusion(kind):
    """a GaussianDiffusion on schedule ``kind``; the callers assign the stand-in denoiser and their own test_cfg (one UNet build per schedule)"""
    if kind not in _DIFFUSIONS:
        import ssdnerf_amd.unet  # noqa: F401
        from ssdnerf_amd.diffusion import GaussianDiffusion
        _DIFFUSIONS[kind] = GaussianDiffusion(denoising=_tiny_unet_cfg(), betas_cfg=dict(type=kind), num_timesteps=1000,
                                              denoising_mean_mode="V").eval()
    return _DIFFUSIONS[kind]


def _sample(kind, mu, s, method, n, noise, **cfg):
    d = _diffusion(kind)
    d.denoising = DR.GaussianDenoiser(d.schedule, mu, s)
    d.test_cfg = dict(num_timesteps=n, clip_range=[-100, 100], sample_method=method, **cfg)
    with torch.no_grad():
        return d(noise.clone(), return_loss=False)


# ------------------------------------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n", [2, 3, 10, 20, 50])
def test_plan_coefficients_equal_the_float64_restatement(kind, n):
    from ssdnerf_amd.diffusion import SamplingPlan
    sched = _schedule(kind)
    plan = SamplingPlan(sched, "dpmpp_2m", n)
    want = DR.plan_coefficients_ref(sched["alphas_bar"], n)
    assert len(plan) == n == len(want) and plan.timesteps.tolist() == [w[0] for w in want]
    for s, (t, c, d, e) in zip(plan, want):
        assert s.kind == "dpmpp" and s.t == t and s.n == 0 and s.emit
        assert s.a == float(sched["sqrt_alphas_bar"][t]) and s.b == float(sched["sqrt_one_minus_alphas_bar"][t])
        for got, ref in ((s.c, c), (s.d, d), (s.e, e)):
            assert abs(got - ref) <= 1e-12 * abs(ref), (t, got, ref)
    last, first = plan.steps[-1], plan.steps[0]
    assert (last.c, last.d, last.e) == (1.0, 0.0, 0.0)
    assert first.e == 0.0
    if n > 2:
        assert all(s.e < 0 and s.c > 0 for s in plan.steps[1:-1])           # second order: extrapolation away from the previous x0


@pytest.mark.parametrize("kind", SCHEDULES)
def test_plan_with_one_step_is_the_single_last_step(kind):
    from ssdnerf_amd.diffusion import SamplingPlan
    plan = SamplingPlan(_schedule(kind), "dpmpp_2m", 1)
    assert len(plan) == 1
    s = plan.steps[0]
    assert (s.kind, s.t, s.c, s.d, s.e, s.n) == ("dpmpp", 999, 1.0, 0.0, 0.0, 0.0)


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n", [2, 3, 10, 20, 50])
def test_first_order_plan_is_the_ddim_plan(kind, n):
    """c x0 + d_ddim (x_t - a x0) / b  ==  (c_ddim - d_ddim a / b) x0 + (d_ddim / b) x_t"""
    from ssdnerf_amd.diffusion import SamplingPlan
    sched = _schedule(kind)
    one, ddim = SamplingPlan(sched, "dpmpp_2m", n, solver_order=1), SamplingPlan(sched, "ddim", n)
    assert len(one) == len(ddim) == n
    for s, r in zip(one, ddim):
        assert (s.t, s.a, s.b, s.e) == (r.t, r.a, r.b, 0.0)
        scale = abs(s.c) + abs(s.d)
        assert abs(s.d - r.d / r.b) <= 1e-12 * scale, (s, r)
        assert abs(s.c - (r.c - r.d * r.a / r.b)) <= 1e-12 * scale, (s, r)


# ------------------------------------------------------------------------------------------------ the bounds
def _f32(x):
    return np.asarray(x, np.float32)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, the sum rounds there (2^-53) and then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _emulate(x, v, q, a, b, c, d, e, lo, hi, form="separate", wrong=None):
    """the kernel in fp32 numpy.  ``form``: 'separate' (every product and sum rounds) or 'fma' (products fused into the sums).
    ``wrong``: None, or one of the four mistakes the bounds must catch."""
    a, b, c, d, e, lo, hi = (np.float32(s) for s in (a, b, c, d, e, lo, hi))
    if wrong == "c_e_exchanged":
        c, e = e, c
    if wrong == "e_sign":
        e = -e
    if form == "separate":
        p0 = a * x - b * v
    else:
        p0 = _fma(a, x, -(b * v))
    p = p0 if wrong == "clamp_after" else np.clip(p0, lo, hi)
    qq = p if wrong == "q_is_p" else q
    if form == "separate":
        xn = c * p + d * x + e * qq
    else:
        xn = _fma(e, qq, _fma(d, x, c * p))
    if wrong == "clamp_after":
        p, xn = np.clip(p, lo, hi), np.clip(xn, lo, hi)
    return _f32(p), _f32(xn)


@pytest.mark.parametrize("form", ["separate", "fma"])
def test_bounds_accept_the_fp32_emulation(form):
    x, v, q = DR.dpmpp_case(1 << 16, 11)
    for name, a, b, c, d, e in DR.dpmpp_coefficients():
        qq = None if e == 0 else q
        p, Bp, ref, Bref = DR.dpmpp_step_ref(x, v, qq, a, b, c, d, e, -1.0, 1.0)
        assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01      # the clamp binds at either end
        got_p, got_xn = _emulate(x, v, q, a, b, c, d, e, -1.0, 1.0, form)
        r0, r1 = DR.check_le(got_p, p, Bp), DR.check_le(got_xn, ref, Bref)
        assert r0[0] == 0 and r1[0] == 0, (name, form, r0, r1)
        assert r1[1] > 0.05, (name, r1)                                      # ... and the bound is of the size of the error, not far above it


@pytest.mark.parametrize("wrong", ["q_is_p", "clamp_after", "c_e_exchanged", "e_sign"])
def test_bounds_reject_wrong_updates(wrong):
    x, v, q = DR.dpmpp_case(1 << 12, 12)
    for name, a, b, c, d, e in DR.dpmpp_coefficients():
        if e == 0:
            continue
        p, Bp, ref, Bref = DR.dpmpp_step_ref(x, v, q, a, b, c, d, e, -1.0, 1.0)
        _, got_xn = _emulate(x, v, q, a, b, c, d, e, -1.0, 1.0, "separate", wrong)
        bad, ratio = DR.check_le(got_xn, ref, Bref)
        assert bad > 0.05 * x.size and ratio > 100, (name, wrong, bad, ratio)


# ------------------------------------------------------------------------------------------------ convergence on the analytic prior
PRIORS = ((0.3, 0.5), (0.0, 1.0), (-0.7, 0.2))
_RMS = {}


def _noise():
    return torch.randn(1, 18, 16, 16, generator=torch.Generator().manual_seed(21))


def _rms(kind, prior, method, n):
    """RMS error of the sampler against the ODE's exact solution; computed once per (schedule, prior, method, n) and shared"""
    key = (kind, prior, method, n)
    if key not in _RMS:
        noise = _noise()
        got = _sample(kind, prior[0], prior[1], method, n, noise)
        want = DR.gaussian_ode_solution(noise, _schedule(kind), *prior)
        _RMS[key] = float((got.double() - want).square().mean().sqrt())
    return _RMS[key]


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("prior", PRIORS)
def test_second_order_beats_ddim_at_equal_step_counts(kind, prior):
    for n in (10, 20, 50):
        e2, e1 = _rms(kind, prior, "dpmpp_2m", n), _rms(kind, prior, "ddim", n)
        print(kind, prior, n, f"dpmpp_2m {e2:.3e} ddim {e1:.3e}")
        assert e2 < e1, (kind, prior, n, e2, e1)


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("prior", PRIORS[:2])
def test_twenty_second_order_steps_beat_fifty_ddim_steps(kind, prior):
    e2, e1 = _rms(kind, prior, "dpmpp_2m", 20), _rms(kind, prior, "ddim", 50)
    print(kind, prior, f"dpmpp_2m@20 {e2:.3e} ddim@50 {e1:.3e}")
    assert e2 < e1, (kind, prior, e2, e1)


@pytest.mark.parametrize("kind", SCHEDULES)
def test_first_order_sampler_reproduces_ddim(kind):
    noise = _noise()
    for n in (10, 20):
        one = _sample(kind, 0.3, 0.5, "dpmpp_2m", n, noise, solver_order=1)
        ddim = _sample(kind, 0.3, 0.5, "ddim", n, noise)
        assert float((one - ddim).abs().max()) <= 1e-5
        two = _sample(kind, 0.3, 0.5, "dpmpp_2m", n, noise)
        assert float((two - ddim).abs().max()) > 1e-3                       # (the order is part of the plan cache key: this is another plan)


def test_save_intermediates_and_the_method_entry_points():
    d = _diffusion("linear")
    d.denoising = DR.GaussianDenoiser(d.schedule, 0.3, 0.5)
    d.test_cfg = dict(num_timesteps=6, clip_range=[-100, 100])
    noise = _noise()
    with torch.no_grad():
        traj = d.dpmpp_2m_sample(noise.clone(), save_intermediates=True)
        direct = d.dpmpp_2m_sample(noise.clone())
        default = d(noise.clone(), return_loss=False)                       # test_cfg names no method: the constructor's 'ddim'
        ddim = d.ddim_sample(noise.clone())
        d.sample_method = "dpmpp_2m"                                         # ... or the constructor argument
        try:
            by_attr = d(noise.clone(), return_loss=False)
        finally:
            d.sample_method = "ddim"
    assert len(traj) == 12 and torch.equal(traj[-1], traj[-2]) and torch.equal(traj[-1], direct)   # (x0, x_next) per step; the last x_next is x0
    assert torch.equal(default, ddim) and torch.equal(by_attr, direct) and not torch.equal(direct, ddim)


# ------------------------------------------------------------------------------------------------ guidance
def test_guided_trajectory_equals_the_float64_recursion():
    """the x0 that enters the history is the guided, clipped one"""
    kind, mu, s, n, gain = "linear", 0.3, 0.5, 5, 0.7
    sched = _schedule(kind)
    noise = _noise()
    gen = torch.Generator().manual_seed(22)
    g, w = torch.randn(1, 18, 16, 16, generator=gen), torch.rand(1, 18, 16, 16, generator=gen)
    d = _diffusion(kind)
    d.denoising = DR.GaussianDenoiser(d.schedule, mu, s)
    d.test_cfg = dict(num_timesteps=n, clip_range=[-1, 1], sample_method="dpmpp_2m", grad_through_unet=False, guidance_gain=gain)
    got = d(noise.clone(), return_loss=False, grad_guide_fn=lambda x0: ((x0 - g) ** 2 * w).sum(), save_intermediates=True)
    # the same recursion in float64: x0* -> clamp -> x0 - 2 w (x0 - g) b gain (snr_weight_power 0.5: b^1 a^0) -> clamp -> three-term update
    A, B = sched["sqrt_alphas_bar"], sched["sqrt_one_minus_alphas_bar"]
    x, q, g64, w64 = noise.double(), None, g.double(), w.double()
    want = []
    for t, c, dd, e in DR.plan_coefficients_ref(sched["alphas_bar"], n):
        a, b = A[t], B[t]
        x0 = (mu + a * s * s / (a * a * s * s + b * b) * (x - a * mu)).clamp(-1, 1)
        x0 = (x0 - 2 * w64 * (x0 - g64) * (b * gain)).clamp(-1, 1)
        x = c * x0 + dd * x + (e * q if q is not None else 0.0)
        q = x0
        want += [x0, x]
    assert len(got) == 2 * n
    for i, (u, r) in enumerate(zip(got, want)):
        assert not u.requires_grad and float((u.double() - r).abs().max()) <= 1e-5, i
    plain = _sample(kind, mu, s, "dpmpp_2m", n, noise)
    assert float((got[-1] - plain).abs().max()) > 1e-2                      # guidance moved the sample


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("cfg", [dict(langevin_steps=2), dict(eta=0.5), dict(solver_order=3)])
def test_unsupported_settings_are_refused(cfg):
    with pytest.raises(ValueError):
        _sample("linear", 0.3, 0.5, "dpmpp_2m", 5, _noise(), **cfg)


def test_unknown_method_is_still_an_attribute_error():
    with pytest.raises(AttributeError):
        _sample("linear", 0.3, 0.5, "heun", 5, _noise())


# ------------------------------------------------------------------------------------------------ existing plans
def test_existing_plan_steps_are_unchanged():
    from ssdnerf_amd.diffusion import PlanStep, SamplingPlan
    s = PlanStep("ddim", 5, 0.1, 0.2, 0.3, 0.4, 0.5, True)                  # the eight positional arguments of every existing construction
    assert s.e == 0.0 and (s.kind, s.t, s.a, s.b, s.c, s.d, s.n, s.emit) == ("ddim", 5, 0.1, 0.2, 0.3, 0.4, 0.5, True)
    for kind in SCHEDULES:
        sched = _schedule(kind)
        ab, var, betas = sched["alphas_bar"], sched["tilde_betas_t"], sched["betas"]
        for n, eta in ((10, 0.0), (50, 0.0), (75, 0.0)):
            plan = SamplingPlan(sched, "ddim", n, eta=eta)
            ts = plan.timesteps.tolist()
            assert len(plan) == n
            for i, p in enumerate(plan):
                ab_prev = ab[ts[i + 1]] if i + 1 < n else 1.0
                want = PlanStep("ddim", ts[i], float(np.sqrt(ab[ts[i]])), float(np.sqrt(1 - ab[ts[i]])), float(np.sqrt(ab_prev)),
                                float(np.sqrt(1 - ab_prev - var[ts[i]] * eta ** 2)), float(eta * np.sqrt(var[ts[i]])), True)
                assert p == want and p.e == 0.0, (kind, n, eta, i)
        plan = SamplingPlan(sched, "ddpm", 10)
        for t, p in zip(plan.timesteps.tolist(), plan):
            c1 = np.sqrt(np.append(1.0, ab[:-1])[t]) / (1 - ab[t]) * betas[t]
            c2 = np.sqrt(1.0 - betas[t]) * (1 - np.append(1.0, ab[:-1])[t]) / (1 - ab[t])
            large = np.append(var[1], betas)[t]                             # FIXED_LARGE, the default variance mode
            want = PlanStep("ddpm", t, float(np.sqrt(ab[t])), float(np.sqrt(1 - ab[t])), float(c1), float(c2), float(np.sqrt(large)) if t else 0.0, True)
            assert p == want and p.e == 0.0, (kind, t)
