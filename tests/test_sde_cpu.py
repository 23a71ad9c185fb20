"""CPU tests of the stochastic sampling feature: the counter-based generator (csrc/philox.h: known answers, a gcc build against the numpy restatement of
tests/_philox_ref.py, statistics of its normals), the ``SamplingPlan`` method 'dpmpp_2m_sde' (coefficients against a float64 restatement, the two
invariants, first order == DDIM with its own sigma, second order closer to the prior's spread than first), ``test_cfg['noise_source']`` (refusals, what
the host generator is asked for, how draws are numbered) and the error bounds tests/test_sde_gpu.py holds csrc/sampler_step.hip to (they accept an fp32
emulation of every form and reject wrong ones)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _dpmpp_ref as DR
import _philox_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCHEDULES = ("linear", "cosine")


# ------------------------------------------------------------------------------------------------ Philox
def test_restatement_gives_the_random123_known_answers():
    for ctr, key, want in PR.KNOWN_ANSWERS:
        got = [int(w) for w in PR.philox4x32_10(*ctr, *key)]
        assert got == list(want), ([hex(g) for g in got], [hex(w) for w in want])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host") / "philox_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "philox_host.c"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.philox_block.restype = lib.quad_words.restype = lib.uniform_bits.restype = None
    lib.philox_block.argtypes = [ctypes.c_void_p] * 3
    lib.quad_words.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p]
    lib.uniform_bits.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def test_gcc_build_of_philox_h_equals_the_restatement(host):
    for ctr, key, want in PR.KNOWN_ANSWERS:
        c, k, out = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
        host.philox_block(c.ctypes.data, k.ctypes.data, out.ctypes.data)
        assert out.tolist() == list(want)
    firsts = (0, (1 << 32) - 2048, (1 << 33) - 7, (1 << 40) + 3)              # ... and quads around 2^32 and beyond: the counter's second word
    for seed in (0, 1234, (1 << 63) + 5):
        for draw in (0, 1, 7):
            for first in firsts:
                out = np.zeros((4096, 4), np.uint32)
                host.quad_words(seed, draw, first, 4096, out.ctypes.data)
                want = PR.quad_words(seed, draw, first, 4096)
                assert np.array_equal(out, want), (seed, draw, first)
    w = PR.quad_words(1234, 0, 0, 4096)
    assert not np.array_equal(w, PR.quad_words(1234, 1, 0, 4096)) and not np.array_equal(w, PR.quad_words(1235, 0, 0, 4096))
    assert not np.array_equal(PR.quad_words(5, 0, 0, 16), PR.quad_words(5, 0, 1 << 32, 16))      # c1 matters
    assert not np.array_equal(PR.quad_words(5, 0, 0, 16), PR.quad_words(5 + (1 << 32), 0, 0, 16))  # so does the key's high word
    m = np.zeros(w.size, np.uint32)
    host.uniform_bits(np.ascontiguousarray(w).ctypes.data, m.ctypes.data, w.size)
    assert np.array_equal(m.reshape(w.shape), w >> 9)
    u = PR.uniforms(w)
    assert u.min() > 0 and u.max() < 1 and np.array_equal(u, u.astype(np.float32).astype(np.float64))      # exact in fp32


def test_statistics_of_the_float64_normals():
    """each within 4 standard errors of its expectation (the restatement gives 0.23, 0.35, 0.71, 0.30 and 0.66)"""
    z = PR.normals(PR.quad_words(1234, 0, 0, 1 << 20))
    z1 = PR.normals(PR.quad_words(1234, 1, 0, 1 << 20))
    N = z.size
    assert N == 1 << 22 and float(np.abs(z).max()) <= PR.Z_MAX
    figures = dict(mean=z.mean() * np.sqrt(N), var=(z.var() - 1) / np.sqrt(2 / N), m4=((z ** 4).mean() - 3) / np.sqrt(96 / N),
                   lag1=np.mean(z[:-1] * z[1:]) * np.sqrt(N), draws=np.mean(z * z1) * np.sqrt(N))
    print({k: round(float(v), 3) for k, v in figures.items()})
    for k, v in figures.items():
        assert abs(v) <= 4, (k, v)


# ------------------------------------------------------------------------------------------------ the plan
def _schedule(kind):
    from ssdnerf_amd.diffusion import NoiseSchedule
    return NoiseSchedule(dict(type=kind), 1000)


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n", [2, 3, 10, 20, 50])
def test_plan_coefficients_equal_the_float64_restatement(kind, n):
    from ssdnerf_amd.diffusion import SamplingPlan
    sched = _schedule(kind)
    plan = SamplingPlan(sched, "dpmpp_2m_sde", n)
    want = PR.sde_plan_coefficients_ref(sched["alphas_bar"], n)
    assert len(plan) == n == len(want) and plan.timesteps.tolist() == [w[0] for w in want]
    assert plan.timesteps.tolist() == SamplingPlan(sched, "dpmpp_2m", n).timesteps.tolist()
    A, B = sched["sqrt_alphas_bar"], sched["sqrt_one_minus_alphas_bar"]
    for i, (s, (t, c, d, e, nz)) in enumerate(zip(plan, want)):
        assert s.kind == "dpmpp_sde" and s.t == t and s.emit and s.a == float(A[t]) and s.b == float(B[t])
        for got, ref in ((s.c, c), (s.d, d), (s.e, e), (s.n, nz)):
            assert abs(got - ref) <= 1e-12 * abs(ref), (t, got, ref)
        if i + 1 < n:                                                        # signal and noise level land on the schedule
            tp = want[i + 1][0]
            assert abs(s.c + s.e + s.d * s.a - A[tp]) <= 1e-12 and abs(s.d ** 2 * s.b ** 2 + s.n ** 2 - B[tp] ** 2) <= 1e-12
            assert s.n > 0
    last = plan.steps[-1]
    assert (last.c, last.d, last.e, last.n) == (1.0, 0.0, 0.0, 0.0) and plan.steps[0].e == 0.0
    if n > 2:
        assert all(s.e < 0 and s.c > 0 for s in plan.steps[1:-1])


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("n", [2, 3, 10, 20, 50])
def test_first_order_plan_is_the_ddim_update_with_its_own_sigma(kind, n):
    """sigma^2 = (b_prev / b_t)^2 (1 - a_t^2 / a_prev^2); c_ddim = a_prev, d_ddim = sqrt(b_prev^2 - sigma^2); as in test_dpmpp_cpu:
    c x0 + d_ddim (x_t - a x0) / b  ==  (c_ddim - d_ddim a / b) x0 + (d_ddim / b) x_t"""
    from ssdnerf_amd.diffusion import SamplingPlan
    sched = _schedule(kind)
    A, B = sched["sqrt_alphas_bar"], sched["sqrt_one_minus_alphas_bar"]
    plan = SamplingPlan(sched, "dpmpp_2m_sde", n, solver_order=1)
    ts = plan.timesteps.tolist()
    for i, s in enumerate(plan.steps[:-1]):
        assert s.e == 0.0
        ap, bp = A[ts[i + 1]], B[ts[i + 1]]
        sigma2 = (bp / s.b) ** 2 * (1 - s.a ** 2 / ap ** 2)
        # d_ddim^2 = b_prev^2 - sigma^2 cancels almost entirely on the first cosine step (d ~ 7e-5 out of two terms of 0.75): the identity is held in
        # its squared, well-conditioned form, to 1e-12 of the terms it subtracts
        scale = abs(s.c) + abs(s.d)
        assert abs(s.n - np.sqrt(sigma2)) <= 1e-12 * scale
        assert abs((s.d * s.b) ** 2 - (bp ** 2 - sigma2)) <= 1e-12 * bp ** 2
        assert abs(s.c - (ap - s.d * s.a)) <= 1e-12 * scale                   # c_ddim - d_ddim a / b with d_ddim / b = d
    assert SamplingPlan(sched, "dpmpp_2m_sde", n).steps[0] == plan.steps[0]
    if n > 2:
        assert SamplingPlan(sched, "dpmpp_2m_sde", n).steps[1] != plan.steps[1]


# ------------------------------------------------------------------------------------------------ the sampler on the analytic prior
def _tiny_unet_cfg():
    return dict(type="DenoisingUnetMod", image_size=16, in_channels=18, base_channels=32, channels_cfg=[1, 2], resblocks_per_downsample=1,
                dropout=0.0, use_scale_shift_norm=True, downsample_conv=True, upsample_conv=True, num_heads=4, attention_res=[8],
                norm_cfg=dict(type="GN", num_groups=8))


_DIFFUSIONS = {}


def _diffusion(kind, T=1000):
    if (kind, T) not in _DIFFUSIONS:
        import ssdnerf_amd.unet  # noqa: F401
        from ssdnerf_amd.diffusion import GaussianDiffusion
        _DIFFUSIONS[kind, T] = GaussianDiffusion(denoising=_tiny_unet_cfg(), betas_cfg=dict(type=kind), num_timesteps=T, denoising_mean_mode="V").eval()
    return _DIFFUSIONS[kind, T]


def _sample(kind, mu, s, method, n, noise, T=1000, **cfg):
    d = _diffusion(kind, T)
    d.denoising = DR.GaussianDenoiser(d.schedule, mu, s)
    d.test_cfg = dict(num_timesteps=n, clip_range=[-100, 100], sample_method=method, **cfg)
    with torch.no_grad():
        return d(noise.clone(), return_loss=False)


def _noise(batch=1, seed=21):
    return torch.randn(batch, 18, 16, 16, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("kind", SCHEDULES)
@pytest.mark.parametrize("prior", [(0.0, 0.5), (0.3, 0.25)])
def test_second_order_is_closer_to_the_priors_spread(kind, prior):
    """|std / s - 1| of order 2 below that of order 1 at 20 and 50 steps; the mean within 5 s / sqrt(N) for both (host noise, 8 x 18 x 16 x 16 = 36864
    elements)"""
    mu, s = prior
    noise = _noise(8)
    N = noise.numel()
    assert N >= 1 << 15
    for n in (20, 50):
        off = {}
        for order in (2, 1):
            torch.manual_seed(100 + n)
            x = _sample(kind, mu, s, "dpmpp_2m_sde", n, noise, solver_order=order).double()
            off[order] = abs(float(x.std()) / s - 1)
            print(kind, prior, n, "order", order, "std/s - 1", round(off[order], 4), "mean - mu", round(float(x.mean()) - mu, 5))
            assert abs(float(x.mean()) - mu) <= 5 * s / N ** 0.5, (kind, prior, n, order)
        assert off[2] < off[1], (kind, prior, n, off)


def test_method_entry_points_and_save_intermediates():
    d = _diffusion("linear")
    d.denoising = DR.GaussianDenoiser(d.schedule, 0.3, 0.5)
    d.test_cfg = dict(num_timesteps=6, clip_range=[-100, 100])
    noise = _noise()
    with torch.no_grad():
        torch.manual_seed(5)
        traj = d.dpmpp_2m_sde_sample(noise.clone(), save_intermediates=True)
        torch.manual_seed(5)
        direct = d.dpmpp_2m_sde_sample(noise.clone())
        d.test_cfg["sample_method"] = "dpmpp_2m_sde"
        torch.manual_seed(5)
        by_cfg = d(noise.clone(), return_loss=False)
        torch.manual_seed(6)
        other = d(noise.clone(), return_loss=False)
        d.test_cfg["sample_method"] = "dpmpp_2m"
        ode = d(noise.clone(), return_loss=False)
    assert len(traj) == 12 and torch.equal(traj[-1], traj[-2]) and torch.equal(traj[-1], direct) and torch.equal(by_cfg, direct)
    assert not torch.equal(other, direct) and not torch.equal(ode, direct)     # the host generator decides the sample; 'dpmpp_2m' stays deterministic


@pytest.mark.parametrize("cfg", [dict(langevin_steps=2), dict(eta=0.5), dict(solver_order=3)])
def test_unsupported_settings_are_refused(cfg):
    with pytest.raises(ValueError):
        _sample("linear", 0.3, 0.5, "dpmpp_2m_sde", 5, _noise(), **cfg)


def test_noise_source_refusals():
    with pytest.raises(ValueError, match="GPU"):
        _sample("linear", 0.3, 0.5, "dpmpp_2m_sde", 5, _noise(), noise_source="device", noise_seed=1)       # a CPU latent
    with pytest.raises(ValueError, match="noise_source"):
        _sample("linear", 0.3, 0.5, "ddim", 5, _noise(), noise_source="philox")
    with pytest.raises(ValueError, match="GPU"):
        d = _diffusion("linear")
        d.denoising = DR.GaussianDenoiser(d.schedule, 0.3, 0.5)
        d.p_sample_ddim(_noise(), 999, 799, cfg=dict(eta=1.0, clip_range=[-100, 100]), noise_seed=3)
    with pytest.raises(ValueError):                                          # 'dpmpp_2m' itself stays the deterministic solver
        _sample("linear", 0.3, 0.5, "dpmpp_2m", 5, _noise(), eta=0.5)


# ------------------------------------------------------------------------------------------------ where the noise comes from
def _same(a, b):
    """bit equality that lets NaN equal NaN: the LAST step of DDIM with eta > 0 has d = sqrt(1 - 1 - eta^2 var) = NaN, here as in the reference
    (gaussian_diffusion.py:280), so such a sample is NaN throughout on every path"""
    return torch.allclose(a, b, rtol=0, atol=0, equal_nan=True)


def _draws(plan):
    return sum(1 for s in plan if s.n != 0 or s.kind == "ddpm")


@pytest.mark.parametrize("method,cfg", [("ddim", dict(eta=0.5, langevin_steps=2)), ("ddpm", {}), ("dpmpp_2m_sde", {})])
def test_default_mode_asks_the_host_generator_for_one_draw_per_noisy_step(method, cfg):
    noise = _noise(2)
    torch.manual_seed(3)
    got = _sample("cosine", 0.3, 0.5, method, 5, noise, **cfg)
    after = torch.get_rng_state()
    count = _draws(_diffusion("cosine").sampling_plan(method))
    assert count == {"ddim": 13, "ddpm": 5, "dpmpp_2m_sde": 4}[method]
    torch.manual_seed(3)
    for _ in range(count):
        torch.randn(noise.shape)
    assert torch.equal(after, torch.get_rng_state())
    torch.manual_seed(3)
    assert _same(got, _sample("cosine", 0.3, 0.5, method, 5, noise, noise_source="host", **cfg))          # 'host' is the default, spelled out
    assert bool(torch.isfinite(got).all()) == (method != "ddim")


@pytest.fixture
def cpu_stand_in(monkeypatch):
    """device mode without a device: the fill replaced by the float64 restatement rounded to fp32, the latent check switched off; records (seed, draw)"""
    from ssdnerf_amd import diffusion as D
    calls = []

    def fill(like, seed, draw):
        calls.append((seed, draw))
        return torch.from_numpy(PR.normals(PR.quad_words(seed, draw, 0, like.numel() // 4)).astype(np.float32)).reshape(like.shape)

    monkeypatch.setattr(D, "_device_noise", fill)
    monkeypatch.setattr(D, "_require_device_latent", lambda x: None)
    return calls


def test_device_mode_numbers_its_draws_and_leaves_the_host_generator_alone(cpu_stand_in):
    noise = _noise(2)
    _diffusion("cosine", 8)                                                  # (building a UNet draws its initial weights: before the state is taken)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    seed = (1 << 63) + 5
    a = _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device", noise_seed=seed)
    assert cpu_stand_in == [(seed, k) for k in range(4)]                     # the last step injects nothing and consumes no index
    del cpu_stand_in[:]
    b = _sample("cosine", 0.3, 0.5, "ddim", 4, noise, noise_source="device", noise_seed=7, eta=0.5, langevin_steps=2)
    assert cpu_stand_in == [(7, k) for k in range(10)]                       # 4 DDIM steps and 2 corrections after each of the first three
    del cpu_stand_in[:]
    c = _sample("cosine", 0.3, 0.5, "ddpm", 8, _noise(2), T=8, noise_source="device", noise_seed=7)
    assert cpu_stand_in == [(7, k) for k in range(7)]                        # t = 0: n = 0, no index (the host mode draws there and multiplies by 0)
    assert torch.equal(before, torch.get_rng_state())                        # nothing was drawn on the host
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(c).all()) and bool(torch.isnan(b).all())     # (b: see _same)
    assert torch.equal(a, _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device", noise_seed=seed))
    assert not torch.equal(a, _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device", noise_seed=seed + 1))
    # the trajectory is the float64 recursion on the restatement's normals
    sched = _diffusion("cosine").schedule
    A, B = sched["sqrt_alphas_bar"], sched["sqrt_one_minus_alphas_bar"]
    x, q, mu, s = noise.double(), None, 0.3, 0.5
    for k, (t, cc, dd, ee, nz) in enumerate(PR.sde_plan_coefficients_ref(sched["alphas_bar"], 5)):
        x0 = mu + A[t] * s * s / (A[t] ** 2 * s * s + B[t] ** 2) * (x - A[t] * mu)
        z = torch.from_numpy(PR.normals(PR.quad_words(seed, k, 0, x.numel() // 4))).reshape(x.shape) if nz != 0 else 0.0
        x = cc * x0 + dd * x + (ee * q if q is not None else 0.0) + nz * z
        q = x0
    assert float((a.double() - x).abs().max()) <= 2e-5


def test_device_mode_without_a_seed_draws_it_from_the_host_generator_once(cpu_stand_in):
    noise = _noise(2)
    torch.manual_seed(11)
    a = _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device")
    seeds = {s for s, _ in cpu_stand_in}
    state = torch.get_rng_state()
    assert len(seeds) == 1 and 0 <= next(iter(seeds)) < 1 << 64
    torch.manual_seed(11)
    assert torch.equal(a, _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device"))    # torch.manual_seed reproduces the run
    assert torch.equal(state, torch.get_rng_state())
    assert not torch.equal(a, _sample("cosine", 0.3, 0.5, "dpmpp_2m_sde", 5, noise, noise_source="device"))  # ... and the next call has another seed
    assert len({s for s, _ in cpu_stand_in}) == 2


def test_single_step_entry_points_take_a_seed(cpu_stand_in):
    d = _diffusion("linear")
    d.denoising = DR.GaussianDenoiser(d.schedule, 0.3, 0.5)
    x = _noise()
    cfg = dict(eta=1.0, clip_range=[-100, 100])
    with torch.no_grad():
        a, _ = d.p_sample_ddim(x, 999, 799, cfg=cfg, noise_seed=3, noise_draw=2)
        b = d.p_sample_langevin(x, 799, cfg=cfg, noise_seed=3, noise_draw=5)
        c, _ = d.p_sample_ddpm(x, 500, cfg=cfg, noise_seed=4)
        z = torch.from_numpy(PR.normals(PR.quad_words(3, 2, 0, x.numel() // 4)).astype(np.float32)).reshape(x.shape)
        want, _ = d.p_sample_ddim(x, 999, 799, noise=z, cfg=cfg)
    assert cpu_stand_in == [(3, 2), (3, 5), (4, 0)] and torch.equal(a, want)
    assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(c).all())


# ------------------------------------------------------------------------------------------------ the bounds
def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64, the sum rounds there (2^-53) and then to fp32"""
    return (np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
            + np.asarray(c, np.float32).astype(np.float64)).astype(np.float32)


def _emulate(form, x, v, q, z, a, b, c, d, e, nz, lo, hi, variant="separate", wrong=None):
    """the kernel in fp32 numpy.  ``variant``: 'separate' (every product and sum rounds) or 'fma' (products fused into the sums).
    ``wrong``: None, or one of the mistakes the bounds must catch.  ``z`` None: a deterministic entry, no noise term at all."""
    a, b, c, d, e, nz, lo, hi = (np.float32(s) for s in (a, b, c, d, e, nz, lo, hi))
    inv_b = np.float32(1.0) / b
    if wrong == "e_sign":
        e = -e
    if wrong == "forms_exchanged":
        form = {0: 1, 1: 0}[form]
    if wrong == "z_scaled_by_c":
        nz = c
    sep = variant == "separate"
    p0 = a * x - b * v if sep else _fma(a, x, -(b * v))
    p = p0 if wrong == "clamp_after" else np.clip(p0, lo, hi)
    if form == 2:
        if sep:
            s = c * p + d * x
            s = s + e * q if e != 0 else s
        else:
            s = _fma(d, x, c * p)
            s = _fma(e, q, s) if e != 0 else s
    else:
        eps = (x - a * p) * inv_b if sep else _fma(-a, p, x) * inv_b
        if form == 0:
            s = c * p + d * eps if sep else _fma(d, eps, c * p)
        else:
            s = x - d * eps if sep else _fma(-d, eps, x)
    xn = s if z is None else s + nz * z if sep else _fma(nz, z, s)
    if wrong == "clamp_after":
        p, xn = np.clip(p, lo, hi), np.clip(xn, lo, hi)
    return np.asarray(p, np.float32), np.asarray(xn, np.float32)


def _case(n, seed):
    x, v, q = PR.sde_case(n, seed)
    z = PR.normals(PR.quad_words(seed, 0, 0, n // 4)).astype(np.float32)
    return x, v, q, z


@pytest.mark.parametrize("variant", ["separate", "fma"])
def test_bounds_accept_the_fp32_emulation_of_every_form(variant):
    x, v, q, z = _case(1 << 16, 11)
    seen = set()
    for name, form, a, b, c, d, e, nz in PR.sde_coefficients():
        seen.add((form, e != 0))
        qq = None if e == 0 else q
        p, Bp, ref, Bref = PR.sde_step_ref(form, x, v, qq, z, a, b, c, d, e, nz, -1.0, 1.0)
        assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01      # the clamp binds at either end
        got_p, got_xn = _emulate(form, x, v, q, z, a, b, c, d, e, nz, -1.0, 1.0, variant)
        r0, r1 = PR.check_le(got_p, p, Bp), PR.check_le(got_xn, ref, Bref)
        print(name, variant, "x0", round(r0[1], 3), "x_next", round(r1[1], 3))
        assert r0[0] == 0 and r1[0] == 0, (name, variant, r0, r1)
        assert r1[1] > 0.05, (name, r1)                                      # ... and the bound is of the size of the error, not far above it
    assert seen == {(0, False), (1, False), (2, False), (2, True)}


@pytest.mark.parametrize("wrong", ["z_scaled_by_c", "clamp_after", "e_sign", "forms_exchanged"])
def test_bounds_reject_wrong_updates(wrong):
    x, v, q, z = _case(1 << 12, 12)
    tried = 0
    for name, form, a, b, c, d, e, nz in PR.sde_coefficients():
        if (wrong == "e_sign" and e == 0) or (wrong == "forms_exchanged" and form == 2):
            continue
        tried += 1
        qq = None if e == 0 else q
        _, _, ref, Bref = PR.sde_step_ref(form, x, v, qq, z, a, b, c, d, e, nz, -1.0, 1.0)
        _, got_xn = _emulate(form, x, v, q, z, a, b, c, d, e, nz, -1.0, 1.0, "separate", wrong)
        bad, ratio = PR.check_le(got_xn, ref, Bref)
        assert bad > 0.05 * x.size and ratio > 100, (name, wrong, bad, ratio)
    assert tried >= 2
