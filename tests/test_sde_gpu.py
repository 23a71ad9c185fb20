"""The counter-based normal fill and the fused stochastic step (csrc/philox.h, csrc/sampler_step.hip, through the C ABI as the sampler calls them) against the
float64 references and per-element bounds of tests/_philox_ref.py (which tests/test_sde_cpu.py proves on the restatement and on an fp32 emulation), their
refusals, the device-noise branches of ``_run_plan`` -- fused against generic, the session kept, seeds -- the untouched host mode, and the sampler through
``DiffusionNeRF.val_uncond`` and a guidance closure.

The bound of the fill needs the ulp errors of the device library's logf, sqrtf and sinpif / cospif.  The ROCm installation documents none, so they are
measured over all 2^23 arguments the generator can feed each function (tools/bench_sde.py --ulp) and read from profiles/sde.json, ``device_function_ulp``.

``python tests/test_sde_gpu.py OUT.json`` runs every kernel case and the fused / generic comparisons and writes the worst error / bound ratios and the
sampler-level differences (they are part of profiles/sde.json)."""
import json
import sys

import numpy as np
import pytest
import torch

import _dpmpp_ref as DR
import _philox_ref as PR
import test_dpmpp_gpu as TD  # (its step call; the tiny UNet, its weights and the fused / generic pair of the deterministic test)

pytestmark = pytest.mark.gpu

SEEDS = ((1234, 0), ((1 << 63) + 5, 7))
PAD = 64                                                                     # sentinel floats behind every filled buffer


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _C():
    from ssdnerf_amd import _cabi as C
    return C


def _cap():
    return int(_C().lib().ssdnerf_sde_block_cap())


def fill_status(out, n, seed, draw):
    C = _C()
    return C.lib().ssdnerf_philox_normal_fill(C.ptr(out), C.ctypes.c_uint64(n), C.ctypes.c_uint64(seed), C.u32(draw), C.stream())


def fill(n, seed, draw):
    """n normals, and whether the PAD sentinels behind them are untouched"""
    buf = torch.full((n + PAD,), 7.0, device="cuda")
    _C().check(fill_status(buf, n, seed, draw), "philox_normal_fill")
    return buf[:n].clone(), bool((buf[n:] == 7.0).all())


def step_status(x_t, v, q, n, form, a, b, c, d, e, nz, seed, draw, x0_out, xnext_out):
    """the call of diffusion.py's ``_run_plan``; returns the status code"""
    C = _C()
    return C.lib().ssdnerf_sde_step_v(C.ptr(x_t), C.ptr(v), C.ptr(q), C.ctypes.c_uint64(n), form, C.f32(a), C.f32(b), C.f32(c), C.f32(d), C.f32(e),
                                      C.f32(nz), C.f32(-1.0), C.f32(1.0), C.ctypes.c_uint64(seed), C.u32(draw), C.ptr(x0_out), C.ptr(xnext_out), C.stream())


def run_step(x_t, v, q, form, a, b, c, d, e, nz, seed, draw, x0_out, xnext_out):
    _C().check(step_status(x_t, v, q, v.numel(), form, a, b, c, d, e, nz, seed, draw, x0_out, xnext_out), "sde_step_v")


# ------------------------------------------------------------------------------------------------ the fill against the restatement
def fill_ratio(n, seed, draw):
    got, clean = fill(n, seed, draw)
    assert clean, "the fill wrote past n"
    again, _ = fill(n, seed, draw)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))       # two runs: the same bits
    ref, B = PR.normal_bounds(PR.quad_words(seed, draw, 0, n // 4), PR.device_function_ulp())
    assert float(got.abs().max()) <= PR.Z_MAX + 1e-5
    return got, PR.check_le(got.cpu(), torch.from_numpy(ref), torch.from_numpy(B)), float((got.cpu().double() - torch.from_numpy(ref)).abs().max())


@pytest.mark.parametrize("which", range(6))
def test_fill_meets_the_float64_box_muller_of_the_restatements_words(which):
    n = PR.sde_sizes(_cap())[which]
    assert n % 4 == 0 and (which < 5 or n // 4 > 256 * _cap())               # the last size takes the grid-stride loop round a second time
    outs = []
    for seed, draw in SEEDS:
        got, (bad, ratio), worst = fill_ratio(n, seed, draw)
        print(n, hex(seed), draw, "worst |z - ref|", f"{worst:.3e}", "worst error / bound", round(ratio, 3))
        assert bad == 0, (n, seed, draw, bad, ratio)
        outs.append(got)
    other, _ = fill(n, SEEDS[0][0], SEEDS[0][1] + 1)
    assert not torch.equal(other, outs[0]) and not torch.equal(outs[0], outs[1])       # another draw, another seed: other normals
    if n >= 4100:                                                            # (a wrong word order would pass none of the above; this is the sanity of the scale)
        assert abs(float(outs[0].mean())) < 5 / n ** 0.5 and abs(float(outs[0].var()) - 1) < 5 * (2 / n) ** 0.5


# ------------------------------------------------------------------------------------------------ the step against the bounds
def step_results(n, form, a, b, c, d, e, nz, seed, draw, case_seed=7):
    """(inputs, z, x0, x_next) out of place, and the number of bits in which the in-place form of the sampler (x_next over x_t, x0 over v) differs"""
    x_np, v_np, q_np = PR.sde_case(n, case_seed)
    x, v, q = cu(x_np), cu(v_np), (cu(q_np) if e != 0 else None)
    z, _ = fill(n, seed, draw)
    x0, xn = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    run_step(x, v, q, form, a, b, c, d, e, nz, seed, draw, x0, xn)
    assert torch.equal(x.cpu(), torch.from_numpy(x_np)) and torch.equal(v.cpu(), torch.from_numpy(v_np))       # inputs are left alone
    assert q is None or torch.equal(q.cpu(), torch.from_numpy(q_np))
    xa, va = x.clone(), v.clone()
    run_step(xa, va, q, form, a, b, c, d, e, nz, seed, draw, va, xa)
    bits = lambda t: t.view(torch.int32)
    aliased = int((bits(xa) != bits(xn)).sum()) + int((bits(va) != bits(x0)).sum())
    return x_np, v_np, (q_np if e != 0 else None), z.cpu(), x0.cpu(), xn.cpu(), aliased


@pytest.mark.parametrize("which", range(6))
def test_sde_step_meets_the_fp64_bounds_out_of_place_and_in_place(which):
    n = PR.sde_sizes(_cap())[which]
    seed, draw = SEEDS[which % 2]
    seen = set()
    for name, form, a, b, c, d, e, nz in PR.sde_coefficients():
        seen.add((form, e != 0))
        x_np, v_np, q_np, z, x0, xn, aliased = step_results(n, form, a, b, c, d, e, nz, seed, draw)
        p, Bp, ref, Bref = PR.sde_step_ref(form, x_np, v_np, q_np, z, a, b, c, d, e, nz, -1.0, 1.0)
        if n >= 1000:
            assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01
        r0, r1 = PR.check_le(x0, p, Bp), PR.check_le(xn, ref, Bref)
        print(name, n, "x0", round(r0[1], 3), "x_next", round(r1[1], 3))
        assert r0[0] == 0 and r1[0] == 0, (name, r0, r1)
        assert aliased == 0, name
    assert seen == {(0, False), (1, False), (2, False), (2, True)}


@pytest.mark.parametrize("which", [0, 4, 5])
def test_step_with_unit_noise_alone_returns_the_fill_bit_for_bit(which):
    """c = d = e = 0 and nz = 1 in form 2: x_next = 0 + 1 z -- the two kernels draw from one generator"""
    n = PR.sde_sizes(_cap())[which]
    x_np, v_np, _ = PR.sde_case(n, 5)
    x, v = cu(x_np), cu(v_np)
    for seed, draw in SEEDS:
        z, _ = fill(n, seed, draw)
        x0, xn = torch.empty_like(x), torch.empty_like(x)
        run_step(x, v, None, 2, 0.6, 0.8, 0.0, 0.0, 0.0, 1.0, seed, draw, x0, xn)
        assert torch.equal(xn.view(torch.int32), z.view(torch.int32)), (n, seed, draw)


@pytest.mark.parametrize("which", range(6))
def test_step_entries_equal_the_fp32_restatement_bit_for_bit(which):
    """Every instantiation behind the three step entries (csrc/sampler_step.hip) against the kernel's own fp32 operations in the kernel's order, restated
    in numpy float32 (test_sde_cpu._emulate, 'separate': the build's -ffp-contract=off makes every product and sum round on its own), with z the bits
    of the fill: x0_out and the updated latent agree BIT FOR BIT -- ``ssdnerf_ddim_step_v``, ``ssdnerf_dpmpp_step_v`` with and without e,
    ``ssdnerf_sde_step_v`` in forms 0, 1, 2 and 2 with e.  And the deterministic entries equal ``ssdnerf_sde_step_v`` with nz = 0: s + 0 z is s for
    finite z except for the sign of a zero, so that comparison is made after adding +0.0 to both."""
    from test_sde_cpu import _emulate
    n = PR.sde_sizes(_cap())[which]
    seed, draw = SEEDS[which % 2]
    x_np, v_np, q_np = PR.sde_case(n, 7)
    x, v, q = cu(x_np), cu(v_np), cu(q_np)
    z, _ = fill(n, seed, draw)
    z_np = z.cpu().numpy()
    assert np.isfinite(z_np).all()
    bits = lambda t: (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t, np.float32)).view(np.int32)
    same = lambda got, want: np.array_equal(bits(got), bits(want))
    new = lambda: (torch.full_like(x, float("nan")), torch.full_like(x, float("nan")))
    seen = set()
    for name, form, a, b, c, d, e, nz in PR.sde_coefficients():
        has_q = e != 0
        x0, xn = new()
        run_step(x, v, q if has_q else None, form, a, b, c, d, e, nz, seed, draw, x0, xn)
        want_p, want_xn = _emulate(form, x_np, v_np, q_np, z_np, a, b, c, d, e, nz, -1.0, 1.0)
        assert same(x0, want_p) and same(xn, want_xn), ("sde_step_v", name, n)
        seen.add((form, has_q, True))
        if form == 1:                                                        # (no deterministic entry takes the Langevin form)
            continue
        d0, dn = new()
        if form == 0:
            C = _C()
            C.check(C.lib().ssdnerf_ddim_step_v(C.ptr(x), C.ptr(v), C.ctypes.c_uint64(n), C.f32(a), C.f32(b), C.f32(c), C.f32(d), C.f32(-1.0), C.f32(1.0),
                                                C.ptr(d0), C.ptr(dn), C.stream()), "ddim_step_v")
        else:
            TD.run_step(x, v, q if has_q else None, a, b, c, d, e, d0, dn)
        want_p, want_dn = _emulate(form, x_np, v_np, q_np, None, a, b, c, d, e, 0.0, -1.0, 1.0)
        assert same(d0, want_p) and same(dn, want_dn), ("ddim_step_v" if form == 0 else "dpmpp_step_v", name, n)
        seen.add((form, has_q, False))
        s0, sn = new()
        run_step(x, v, q if has_q else None, form, a, b, c, d, e, 0.0, seed, draw, s0, sn)
        assert same(s0, d0) and same(sn + 0.0, dn + 0.0), ("nz = 0", name, n)
    assert seen == {(0, False, True), (1, False, True), (2, False, True), (2, True, True), (0, False, False), (2, False, False), (2, True, False)}


def test_refusals_return_an_error_code_and_launch_nothing():
    x_np, v_np, q_np = PR.sde_case(8, 3)
    x, v, q = cu(x_np), cu(v_np), cu(q_np)
    x0, xn = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    a, b, c, d, e, nz = 0.6, 0.8, 0.5, 0.4, -0.1, 0.3
    ok = lambda **kw: step_status(**{**dict(x_t=x, v=v, q=q, n=8, form=2, a=a, b=b, c=c, d=d, e=e, nz=nz, seed=1, draw=0, x0_out=x0, xnext_out=xn), **kw})
    assert ok(n=6) != 0                                                      # n % 4 != 0
    assert ok(form=3) != 0 and ok(form=-1) != 0                              # an unknown form
    assert b"form" in _C().lib().ssdnerf_last_error()
    assert ok(q=None) != 0                                                   # no history, e != 0
    assert ok(x0_out=q) != 0                                                 # x0_out == x0_prev
    assert b"alias" in _C().lib().ssdnerf_last_error()
    assert ok(x_t=None) != 0 and ok(v=None) != 0 and ok(x0_out=None) != 0 and ok(xnext_out=None) != 0
    assert fill_status(None, 8, 1, 0) != 0 and fill_status(xn, 6, 1, 0) != 0
    assert ok(n=0) == 0 and fill_status(xn, 0, 1, 0) == 0                    # n == 0 is a no-op
    torch.cuda.synchronize()
    assert bool((x0 == 7).all()) and bool((xn == 7).all()) and torch.equal(q.cpu(), torch.from_numpy(q_np))
    assert ok() == 0                                                         # the same call, well-formed
    assert ok(q=None, e=0.0) == 0 and ok(form=0, q=None, e=0.0) == 0 and ok(form=1, q=None, e=0.0) == 0
    assert ok(form=0, q=None) != 0                                           # (the history rule does not depend on the form)
    assert not bool((x0 == 7).any())


# ------------------------------------------------------------------------------------------------ the sampler: fused against generic, device noise

METHODS = {  # name -> (sampler method, test_cfg additions)
    "dpmpp_2m_sde": ("dpmpp_2m_sde", {}),
    "ddim_eta": ("ddim", dict(eta=0.5)),
    "ddpm_20": ("ddpm", dict(num_timesteps=20)),
    "ddim_langevin": ("ddim", dict(langevin_steps=2)),
}
_STATE = {}


def _diffusion():
    if "d" not in _STATE:
        _STATE["d"] = TD._small_diffusion()
        _STATE["cfg"] = dict(_STATE["d"].test_cfg)
    d = _STATE["d"]
    d.test_cfg = dict(_STATE["cfg"])
    d.use_fused_step = True
    return d


def _noise():
    return torch.randn(2, 18, 16, 16, generator=torch.Generator().manual_seed(2))


def _base():
    """the largest |fused - generic| of the two deterministic DDIM paths in this process: what test_fused_dpmpp_trajectory_equals_the_generic_one
    measures its tolerance from"""
    if "base" not in _STATE:
        d = _diffusion()
        _STATE["base"] = max(float((a - b).abs().max()) for a, b in zip(*TD.fused_and_generic(d, d.ddim_sample, _noise())))
    return _STATE["base"]


class _Calls:
    """counts the eager ``pred_x_0`` (the generic branch) and the library's step / fill launches"""
    NAMES = ("ssdnerf_ddim_step_v", "ssdnerf_dpmpp_step_v", "ssdnerf_sde_step_v", "ssdnerf_philox_normal_fill")

    def __init__(self, monkeypatch, d):
        self.n = dict.fromkeys(self.NAMES + ("pred_x_0", "host_noise"), 0)
        lib = _C().lib()
        for name in self.NAMES:
            monkeypatch.setattr(lib, name, self._wrap(name, getattr(lib, name)))
        monkeypatch.setattr(d, "pred_x_0", self._wrap("pred_x_0", d.pred_x_0))
        from ssdnerf_amd import diffusion as D
        monkeypatch.setattr(D, "_host_noise", self._wrap("host_noise", D._host_noise))

    def _wrap(self, name, fn):
        def counted(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return counted

    def take(self):
        out, self.n = self.n, dict.fromkeys(self.n, 0)
        return out


def _trajectory(d, method, fused):
    """[x0, x_next] per emitting step, straight from ``_run_plan`` (``ddpm_sample`` has no ``save_intermediates``, as in the reference)"""
    d.use_fused_step = fused
    try:
        with torch.no_grad():
            return d._run_plan(d.sampling_plan(method), _noise().cuda(), None, True)
    finally:
        d.use_fused_step = True


def device_pair(d, name, seed=77):
    method, extra = METHODS[name]
    d.test_cfg.update(noise_source="device", noise_seed=seed, **extra)
    return _trajectory(d, method, True), _trajectory(d, method, False)


def _worst(fused, generic, nan_tail):
    """largest difference over the trajectory; ``nan_tail``: the LAST latent of DDIM with eta > 0 is NaN on every path, here as in the reference
    (d = sqrt(1 - 1 - eta^2 var) on the step that lands on abar_prev = 1): it is required to be NaN on both and left out of the maximum"""
    assert len(fused) == len(generic)
    if nan_tail:
        assert bool(torch.isnan(fused[-1]).all()) and bool(torch.isnan(generic[-1]).all())
        fused, generic = fused[:-1], generic[:-1]
    return max(float((a - b).abs().max()) for a, b in zip(fused, generic))


@pytest.mark.parametrize("name", list(METHODS))
def test_fused_device_noise_trajectory_equals_the_generic_one(name, monkeypatch):
    """The tolerance is that of test_fused_dpmpp_trajectory_equals_the_generic_one: four times the largest difference between the two deterministic DDIM
    paths, measured in the run that uses it.  Both branches add bit-identical normals (the fill against the fused step), so what differs is the order of the
    fp32 operations alone.  Measured on an MI355X: see profiles/sde.json, ``sampler``."""
    d = _diffusion()
    base = _base()
    calls = _Calls(monkeypatch, d)
    d.test_cfg.update(noise_source="device", noise_seed=77, **METHODS[name][1])
    method = METHODS[name][0]
    plan = d.sampling_plan(method)
    noisy = sum(1 for s in plan if s.n != 0)
    fused = _trajectory(d, method, True)
    n_fused = calls.take()
    generic = _trajectory(d, method, False)
    n_generic = calls.take()
    # the session is kept throughout: no eager x0 prediction, no fill, no host draw; every noisy step is one sde launch, the others keep their kernels
    assert n_fused["pred_x_0"] == 0 and n_fused["ssdnerf_philox_normal_fill"] == 0 and n_fused["host_noise"] == 0, n_fused
    assert n_fused["ssdnerf_sde_step_v"] == noisy and noisy > 0, (n_fused, noisy)
    assert n_fused["ssdnerf_sde_step_v"] + n_fused["ssdnerf_ddim_step_v"] + n_fused["ssdnerf_dpmpp_step_v"] == len(plan), n_fused
    assert n_generic["pred_x_0"] == len(plan) and n_generic["ssdnerf_philox_normal_fill"] == noisy and n_generic["host_noise"] == 0, n_generic
    assert n_generic["ssdnerf_sde_step_v"] == 0
    emitting = sum(1 for s in plan if s.emit)
    assert len(fused) == len(generic) == 2 * emitting
    diff = _worst(fused, generic, nan_tail=name == "ddim_eta")
    print(f"{name}: fused vs generic over {len(plan)} steps {diff:.3e}; ddim {base:.3e}, tolerance {4 * base:.3e}")
    assert base > 0 and diff <= 4 * base, (name, diff, base)
    assert float((fused[-2] - fused[0]).abs().max()) > 1e-2                  # (a trajectory, not copies of one point)


def test_same_seed_same_sample_another_seed_another():
    """The UNet's split-K layers accumulate with atomics: two replays agree to rounding, not bit for bit (test_dpmpp_gpu holds them to 1e-4 of the largest
    magnitude, and so does this); the noise itself is the same bits."""
    d = _diffusion()
    d.test_cfg.update(noise_source="device", sample_method="dpmpp_2m_sde")
    out = {}
    with torch.no_grad():
        for key, seed in (("a", 5), ("b", 5), ("c", 6)):
            d.test_cfg["noise_seed"] = seed
            out[key] = d(_noise().cuda(), return_loss=False)
        d.test_cfg.pop("noise_seed")
        for key in ("m", "n"):
            torch.manual_seed(9)                                             # no noise_seed: one 64-bit draw from the host generator
            out[key] = d(_noise().cuda(), return_loss=False)
    scale = float(out["a"].abs().max())
    assert float((out["a"] - out["b"]).abs().max()) <= 1e-4 * scale and float((out["m"] - out["n"]).abs().max()) <= 1e-4 * scale
    assert float((out["a"] - out["c"]).abs().max()) > 1e-2 and float((out["a"] - out["m"]).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        d(_noise(), return_loss=False)                                       # device noise, CPU latent


@pytest.mark.parametrize("method,cfg", [("ddim", {}), ("dpmpp_2m", {}), ("ddim", dict(eta=0.5, langevin_steps=1)), ("dpmpp_2m_sde", {})])
def test_host_mode_is_the_parents(method, cfg, monkeypatch):
    """noise_source unset: the deterministic steps through ssdnerf_ddim_step_v / ssdnerf_dpmpp_step_v in the session, every noisy step through the eager
    branch on a host draw, the host generator left where as many ``torch.randn`` of the latent's shape leave it, and no launch of the new kernels"""
    d = _diffusion()
    calls = _Calls(monkeypatch, d)
    d.test_cfg.update(cfg)
    plan = d.sampling_plan(method)
    draws = sum(1 for s in plan if s.n != 0 or s.kind == "ddpm")
    noise = _noise()
    torch.manual_seed(3)
    with torch.no_grad():
        got = getattr(d, f"{method}_sample")(noise.cuda())
    after = torch.get_rng_state()
    n = calls.take()
    assert n["ssdnerf_sde_step_v"] == 0 and n["ssdnerf_philox_normal_fill"] == 0 and n["host_noise"] == draws, n
    torch.manual_seed(3)
    for _ in range(draws):
        torch.randn(noise.shape)
    assert torch.equal(after, torch.get_rng_state())
    if draws == 0:
        kernel = "ssdnerf_ddim_step_v" if method == "ddim" else "ssdnerf_dpmpp_step_v"
        assert n[kernel] == len(plan) and n["pred_x_0"] == 0, n
        assert bool(torch.isfinite(got).all())
    else:
        first_noisy = next(i for i, s in enumerate(plan) if s.n != 0)
        assert n["pred_x_0"] == len(plan) - first_noisy and n["ssdnerf_ddim_step_v"] + n["ssdnerf_dpmpp_step_v"] == first_noisy, n


def test_guidance_runs_the_generic_branch_on_device_noise(monkeypatch):
    d = _diffusion()
    calls = _Calls(monkeypatch, d)
    d.test_cfg.update(noise_source="device", noise_seed=3, grad_through_unet=False, guidance_gain=0.1)
    target = torch.zeros(2, 18, 16, 16, device="cuda")
    with torch.no_grad():
        plain = d.dpmpp_2m_sde_sample(_noise().cuda())
        calls.take()
        guided = d.dpmpp_2m_sde_sample(_noise().cuda(), grad_guide_fn=lambda x0: ((x0 - target) ** 2).sum())
    n = calls.take()
    steps = len(d.sampling_plan("dpmpp_2m_sde"))
    assert n["pred_x_0"] == steps and n["ssdnerf_philox_normal_fill"] == steps - 1 and n["ssdnerf_sde_step_v"] == 0 and n["host_noise"] == 0, n
    assert bool(torch.isfinite(guided).all()) and not guided.requires_grad and float((guided - plain).abs().max()) > 1e-3


def test_val_uncond_with_dpmpp_2m_sde_on_device_noise():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.registry import MODELS
    from ssdnerf_amd import synthetic as S
    cfg = dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2),
               grid_size=64,
               diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                              denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                             resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4, attention_res=[32],
                                             norm_cfg=dict(type="GN", num_groups=8))),
               decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3],
                            use_dir_enc=True, dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001,
                            max_steps=256),
               decoder_use_ema=True, freeze_decoder=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
               reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=0,
               test_cfg=dict(img_size=(128, 128), num_timesteps=4, clip_range=[-2, 2], density_thresh=0.1))
    m = MODELS.build(cfg)
    TD._randomize(m.diffusion_ema, 9)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(4)
    noise = torch.randn(2, 3, 6, 128, 128, generator=g).cuda()
    jit = [torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(8)]
    data = dict(scene_id=[0, 1], noise=noise)
    diff = m.diffusion_ema
    diff.test_cfg.update(sample_method="dpmpp_2m_sde", num_timesteps=4, noise_source="device", noise_seed=21)
    before = torch.get_rng_state()
    code, grid, bits = m.val_uncond(data, density_jitters=jit)
    assert torch.equal(before, torch.get_rng_state())                        # nothing drawn on the host
    assert code.shape == (2, 3, 6, 128, 128) and grid.shape == (2, 64 ** 3) and grid.dtype == torch.float16 and bits.shape == (2, 64 ** 3 // 8)
    assert bool(torch.isfinite(code).all()) and bool(torch.isfinite(grid.float()).all()) and float(code.abs().max()) <= 2.0
    with torch.no_grad():
        want = m.code_diff_pr_inv(diff.dpmpp_2m_sde_sample(m.code_diff_pr(noise)).float())
    assert float((code - want).abs().max()) <= 1e-4 * float(want.abs().max())
    diff.test_cfg.update(sample_method="dpmpp_2m")
    ode, _, _ = m.val_uncond(data, density_jitters=jit)
    assert float((code - ode).abs().max()) > 1e-3                            # the stochastic solver: another sample from the same start


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {"fill": 0.0, "fill_abs": 0.0}
    for n in PR.sde_sizes(_cap()):
        for seed, draw in SEEDS:
            _, (_, ratio), err = fill_ratio(n, seed, draw)
            worst["fill"], worst["fill_abs"] = max(worst["fill"], round(ratio, 4)), max(worst["fill_abs"], err)
        for name, form, a, b, c, d, e, nz in PR.sde_coefficients():
            x_np, v_np, q_np, z, x0, xn, _ = step_results(n, form, a, b, c, d, e, nz, *SEEDS[0])
            p, Bp, ref, Bref = PR.sde_step_ref(form, x_np, v_np, q_np, z, a, b, c, d, e, nz, -1.0, 1.0)
            for k, r in (("x0", PR.check_le(x0, p, Bp)), ("x_next", PR.check_le(xn, ref, Bref))):
                worst.setdefault(name, {})[k] = max(worst.get(name, {}).get(k, 0.0), round(r[1], 4))
    d = _diffusion()
    base = _base()
    sampler = dict(ddim_fused_vs_generic=base, tolerance=4 * base,
                   what="largest |fused - generic| over the trajectory, noise (2, 18, 16, 16), linear schedule, device noise")
    for name in METHODS:
        d = _diffusion()
        sampler[name] = _worst(*device_pair(d, name), nan_tail=name == "ddim_eta")
    return dict(worst_ratio=worst, sampler=sampler)


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = dict(what="worst |kernel - fp64 reference| / bound per output over every seeded case of tests/test_sde_gpu.py, and the sampler-level differences",
               device=torch.cuda.get_device_name(0), **measure())
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
