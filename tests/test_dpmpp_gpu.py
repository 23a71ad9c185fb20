"""The DPM-Solver++(2M) step (csrc/sampler_step.hip, through the C ABI as the sampler calls it) against the float64 reference and per-element bounds of
tests/_dpmpp_ref.py (which tests/test_dpmpp_cpu.py proves on an fp32 emulation), its refusals, the fused branch of ``_run_plan`` against the
generic one, and the sampler through ``DiffusionNeRF.val_uncond``.

``python tests/test_dpmpp_gpu.py OUT.json`` runs every kernel case and the fused / generic comparison and writes the worst error / bound ratios
and the two sampler-level differences (they are part of profiles/dpmpp.json)."""
import json
import sys

import numpy as np
import pytest
import torch

import _dpmpp_ref as DR

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _C():
    from ssdnerf_amd import _cabi as C
    return C


def step_status(x_t, v, q, n, a, b, c, d, e, x0_out, xnext_out):
    """the call of diffusion.py's ``_run_plan``; returns the status code"""
    C = _C()
    return C.lib().ssdnerf_dpmpp_step_v(C.ptr(x_t), C.ptr(v), C.ptr(q), C.ctypes.c_uint64(n), C.f32(a), C.f32(b), C.f32(c), C.f32(d), C.f32(e),
                                        C.f32(-1.0), C.f32(1.0), C.ptr(x0_out), C.ptr(xnext_out), C.stream())


def run_step(x_t, v, q, a, b, c, d, e, x0_out, xnext_out):
    _C().check(step_status(x_t, v, q, v.numel(), a, b, c, d, e, x0_out, xnext_out), "dpmpp_step_v")


# ------------------------------------------------------------------------------------------------ the kernel against the bounds
def step_results(n, a, b, c, d, e, seed=7):
    """(inputs, x0, x_next) out of place, and the number of bits in which the in-place form of the sampler (x_next over x_t, x0 over v) differs"""
    x_np, v_np, q_np = DR.dpmpp_case(n, seed)
    x, v, q = cu(x_np), cu(v_np), (cu(q_np) if e != 0 else None)
    x0, xn = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    run_step(x, v, q, a, b, c, d, e, x0, xn)
    assert torch.equal(x.cpu(), torch.from_numpy(x_np)) and torch.equal(v.cpu(), torch.from_numpy(v_np))       # inputs are left alone
    assert q is None or torch.equal(q.cpu(), torch.from_numpy(q_np))
    xa, va = x.clone(), v.clone()
    run_step(xa, va, q, a, b, c, d, e, va, xa)
    bits = lambda t: t.view(torch.int32)
    aliased = int((bits(xa) != bits(xn)).sum()) + int((bits(va) != bits(x0)).sum())
    return x_np, v_np, (q_np if e != 0 else None), x0.cpu(), xn.cpu(), aliased


@pytest.mark.parametrize("which", range(6))
def test_dpmpp_step_meets_the_fp64_bounds_out_of_place_and_in_place(which):
    cap = int(_C().lib().ssdnerf_dpmpp_block_cap())
    n = DR.dpmpp_sizes(cap)[which]
    assert n % 4 == 0 and (which < 5 or n // 4 > 256 * cap)                  # the last size takes the grid-stride loop round a second time
    for name, a, b, c, d, e in DR.dpmpp_coefficients():
        x_np, v_np, q_np, x0, xn, aliased = step_results(n, a, b, c, d, e)
        p, Bp, ref, Bref = DR.dpmpp_step_ref(x_np, v_np, q_np, a, b, c, d, e, -1.0, 1.0)
        if n >= 1000:
            assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01
        r0, r1 = DR.check_le(x0, p, Bp), DR.check_le(xn, ref, Bref)
        print(name, n, "x0", round(r0[1], 3), "x_next", round(r1[1], 3))
        assert r0[0] == 0 and r1[0] == 0, (name, r0, r1)
        assert aliased == 0, name
        if name == "last":
            assert torch.equal(xn, x0)                                       # c, d, e = 1, 0, 0: x_next is x0


def test_refusals_return_an_error_code_and_launch_nothing():
    x_np, v_np, q_np = DR.dpmpp_case(8, 3)
    x, v, q = cu(x_np), cu(v_np), cu(q_np)
    x0, xn = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    a, b, c, d, e = 0.6, 0.8, 0.5, 0.4, -0.1
    assert step_status(x, v, q, 6, a, b, c, d, e, x0, xn) != 0               # n % 4 != 0
    assert step_status(x, v, None, 8, a, b, c, d, e, x0, xn) != 0            # no history, e != 0
    assert step_status(x, v, q, 8, a, b, c, d, e, q, xn) != 0                # x0_out == x0_prev
    assert b"alias" in _C().lib().ssdnerf_last_error()
    assert step_status(x, v, q, 0, a, b, c, d, e, x0, xn) == 0               # n == 0 is a no-op
    torch.cuda.synchronize()
    assert bool((x0 == 7).all()) and bool((xn == 7).all()) and torch.equal(q.cpu(), torch.from_numpy(q_np))
    assert step_status(x, v, q, 8, a, b, c, d, e, x0, xn) == 0               # the same call, well-formed
    assert not bool((x0 == 7).any())


# ------------------------------------------------------------------------------------------------ fused against generic
def _tiny_unet_cfg(image_size=16):
    return dict(type="DenoisingUnetMod", image_size=image_size, in_channels=18, base_channels=32, channels_cfg=[1, 2], resblocks_per_downsample=1,
                dropout=0.0, use_scale_shift_norm=True, downsample_conv=True, upsample_conv=True, num_heads=4, attention_res=[image_size // 2],
                norm_cfg=dict(type="GN", num_groups=8))


def _randomize(module, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.2 / max(1.0, p[0].numel() ** 0.5) if p.dim() > 1 else 0.1))


def _small_diffusion():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.diffusion import GaussianDiffusion
    d = GaussianDiffusion(denoising=_tiny_unet_cfg(), betas_cfg=dict(type="linear"), num_timesteps=1000, denoising_mean_mode="V",
                          test_cfg=dict(num_timesteps=10, clip_range=[-2, 2]))
    _randomize(d, 5)
    return d.eval().cuda()


def fused_and_generic(d, sample, noise):
    out = []
    with torch.no_grad():
        for fused in (True, False):
            d.use_fused_step = fused
            out.append(sample(noise.cuda(), save_intermediates=True))
        d.use_fused_step = True
    return out


def sampler_differences(d=None):
    """(largest |fused - generic| over the 10-step trajectory of the two DDIM paths, the same of the two dpmpp_2m paths, the dpmpp_2m trajectories)"""
    d = _small_diffusion() if d is None else d
    noise = torch.randn(2, 18, 16, 16, generator=torch.Generator().manual_seed(2))
    worst = lambda pair: max(float((a - b).abs().max()) for a, b in zip(*pair))
    ddim = fused_and_generic(d, d.ddim_sample, noise)
    dpmpp = fused_and_generic(d, d.dpmpp_2m_sample, noise)
    return worst(ddim), worst(dpmpp), dpmpp


def test_fused_dpmpp_trajectory_equals_the_generic_one():
    """The tolerance is measured, not chosen: the largest difference between the two DDIM paths that were there before (fused step / tensor
    expressions; same noise, UNet and step count) times 4 -- the update has three product terms where DDIM's has two, and |c| + |e| exceeds 1 on
    second-order steps.  On an MI355X (profiles/dpmpp.json, ``sampler``): DDIM 9.5e-7, so a tolerance of 3.8e-6, and dpmpp_2m 7.2e-7; over four
    processes DDIM gave 9.5e-7 or 1.2e-6 and dpmpp_2m 7.2e-7 or 9.5e-7 (the UNet's split-K layers accumulate with atomics, so neither figure is
    the same in every run: the tolerance is measured in the run that uses it)."""
    base, diff, (fused, generic) = sampler_differences()
    print(f"fused vs generic over 10 steps: ddim {base:.3e}, dpmpp_2m {diff:.3e}, tolerance {4 * base:.3e}")
    assert len(fused) == len(generic) == 20
    assert base > 0                                                          # (two different orders of fp32 operations: they do differ)
    assert diff <= 4 * base, (diff, base)
    assert torch.equal(fused[-1], fused[-2]) and torch.equal(generic[-1], generic[-2])      # last step: x_next == x0
    assert float((fused[-1] - fused[0]).abs().max()) > 1e-2                  # (a trajectory, not ten copies of one point)


# ------------------------------------------------------------------------------------------------ through the model
def test_val_uncond_with_dpmpp_2m_and_unchanged_default():
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
    _randomize(m.diffusion_ema, 9)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().eval()
    g = torch.Generator().manual_seed(4)
    noise = torch.randn(2, 3, 6, 128, 128, generator=g).cuda()
    jit = [torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(8)]
    data = dict(scene_id=[0, 1], noise=noise)
    diff, unet = m.diffusion_ema, m.diffusion_ema.denoising

    def direct(sample):
        with torch.no_grad():
            return m.code_diff_pr_inv(sample(m.code_diff_pr(noise)).float())

    def uncond(method):
        diff.test_cfg.pop("sample_method", None)
        if method is not None:
            diff.test_cfg.update(sample_method=method, num_timesteps=4)
        return m.val_uncond(data, density_jitters=jit)

    # ---- on the inference executor (the fused steps): shapes, finiteness, another sample than DDIM's; sample_method unset is DDIM.
    # The executor's split-K layers accumulate with atomics: two replays of the SAME sampler agree to rounding, not bit for bit (measured here:
    # 4.8e-7 between two ddim_sample calls; tests/test_soak_gpu.py::test_soak_unet_executor holds replays to 1e-4 of the largest magnitude, and
    # so does this comparison).  Bit equality is asked below, where the network is deterministic.
    code_d, grid_d, bits_d = uncond(None)
    want, again = direct(diff.ddim_sample), direct(diff.ddim_sample)
    print(f"executor: val_uncond vs ddim_sample {float((code_d - want).abs().max()):.3e}; ddim_sample twice {float((again - want).abs().max()):.3e}")
    assert float((code_d - want).abs().max()) <= 1e-4 * float(want.abs().max())
    code, grid, bits = uncond("dpmpp_2m")
    assert code.shape == (2, 3, 6, 128, 128) and grid.shape == grid_d.shape == (2, 64 ** 3) and grid.dtype == torch.float16
    assert bits.shape == (2, 64 ** 3 // 8) and bits.dtype == bits_d.dtype
    assert bool(torch.isfinite(code).all()) and bool(torch.isfinite(grid.float()).all()) and float(code.abs().max()) <= 2.0
    assert float((code - code_d).abs().max()) > 1e-4                         # another solver: another sample from the same noise
    assert float((code - direct(diff.dpmpp_2m_sample)).abs().max()) <= 1e-4 * float(code.abs().max())
    # ---- the same calls, same model, with a denoiser that answers the same bits every time (the analytic stand-in; the module forward of the UNet does
    # not either: 4.8e-7 between its first two calls): bit for bit
    diff.denoising = DR.GaussianDenoiser(diff.schedule, 0.3, 0.5)
    try:
        code_e, _, _ = uncond(None)
        assert torch.equal(code_e, direct(diff.ddim_sample))                 # sample_method unset: DDIM's result for the same noise
        code_2m, _, _ = uncond("dpmpp_2m")
        assert torch.equal(code_2m, direct(diff.dpmpp_2m_sample)) and not torch.equal(code_2m, code_e)
    finally:
        diff.denoising = unet
        diff.test_cfg.pop("sample_method", None)


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}
    cap = int(_C().lib().ssdnerf_dpmpp_block_cap())
    for name, a, b, c, d, e in DR.dpmpp_coefficients():
        for n in DR.dpmpp_sizes(cap):
            x_np, v_np, q_np, x0, xn, _ = step_results(n, a, b, c, d, e)
            p, Bp, ref, Bref = DR.dpmpp_step_ref(x_np, v_np, q_np, a, b, c, d, e, -1.0, 1.0)
            for k, r in (("x0", DR.check_le(x0, p, Bp)), ("x_next", DR.check_le(xn, ref, Bref))):
                worst.setdefault(name, {})[k] = max(worst.get(name, {}).get(k, 0.0), round(r[1], 4))
    base, diff, _ = sampler_differences()
    return dict(worst_ratio=worst, sampler=dict(ddim_fused_vs_generic=base, dpmpp_2m_fused_vs_generic=diff, tolerance=4 * base,
                                                what="largest |fused - generic| over a 10-step trajectory, noise (2, 18, 16, 16), linear schedule"))


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = dict(what="worst |kernel - fp64 reference| / bound per output over every seeded case of tests/test_dpmpp_gpu.py, and the sampler-level differences",
               device=torch.cuda.get_device_name(0), **measure())
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
