"""The prior-loss kernels (csrc/prior_loss.hip, through the C ABI as ``diffusion.forward_train`` calls them) against the fp32 restatement and the float64
bounds of tests/_prior_loss_ref.py (which tests/test_prior_loss_cpu.py proves on emulations), their refusals and no-ops; the fused ``forward_train`` against a
float64 evaluation of the whole chain with the analytic denoiser, and against the generic device branch with a tiny UNet; and the wiring of
``noise_source='device'`` through ``DiffusionNeRF.train_step``, ``val_optim`` and ``val_uncond`` with the host draw patched to raise.

``python tests/test_prior_loss_gpu.py OUT.json`` runs every kernel case and the two ``forward_train`` comparisons and writes the worst error / bound ratios
and the gradient errors (they are part of profiles/prior_loss.json)."""
import copy
import json
import sys
import warnings

import numpy as np
import pytest
import torch

import _dpmpp_ref as DR
import _prior_loss_ref as LR

pytestmark = pytest.mark.gpu

SEEDS = ((1234, (1 << 31) | 0), ((1 << 63) + 5, (1 << 31) | 7))
PAD = 64                                                                     # sentinel floats behind every written buffer
KINDS = ("linear", "cosine")
T = 1000
_CASES = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _C():
    from ssdnerf_amd import _cabi as C
    return C


def _cap():
    return int(_C().lib().ssdnerf_prior_block_cap())


def _bps(n_per):
    return int(_C().lib().ssdnerf_prior_blocks_per_sample(n_per))


def _u64(v):
    return _C().ctypes.c_uint64(int(v))


def _dt(t):
    C = _C()
    return C.F32 if t is None else {torch.float32: C.F32, torch.bfloat16: C.BF16}[t.dtype]


def fill(n, seed, draw):
    C = _C()
    out = torch.empty(n, device="cuda")
    C.check(C.lib().ssdnerf_philox_normal_fill(C.ptr(out), _u64(n), _u64(seed), C.u32(draw), C.stream()), "philox_normal_fill")
    return out


def q_sample_status(x0, a, b, B, n_per, seed, draw, out):
    C = _C()
    return C.lib().ssdnerf_prior_q_sample(C.ptr(x0), C.ptr(a), C.ptr(b), C.u32(B), _u64(n_per), _u64(seed), C.u32(draw), C.ptr(out), C.stream())


def loss_status(pred, x0, a, b, B, n_per, seed, draw, partials, msd, x0sq, dtype=None):
    C = _C()
    return C.lib().ssdnerf_prior_loss_v(C.ptr(pred), _dt(pred) if dtype is None else dtype, C.ptr(x0), C.ptr(a), C.ptr(b), C.u32(B), _u64(n_per), _u64(seed),
                                        C.u32(draw), C.ptr(partials), C.ptr(msd), C.ptr(x0sq), C.stream())


def backward_status(pred, x0, a, b, k, B, n_per, seed, draw, grad_pred, grad_x0, dtype=None):
    C = _C()
    return C.lib().ssdnerf_prior_loss_v_backward(C.ptr(pred), _dt(pred) if dtype is None else dtype, C.ptr(x0), C.ptr(a), C.ptr(b), C.ptr(k), C.u32(B),
                                                 _u64(n_per), _u64(seed), C.u32(draw), C.ptr(grad_pred), C.ptr(grad_x0), C.stream())


def _schedule(kind):
    from ssdnerf_amd.diffusion import NoiseSchedule
    return NoiseSchedule(dict(type=kind), T)


def _case(which, kind):
    """the inputs of shape ``which`` on schedule ``kind`` (timesteps 0 and T - 1 among them), the fill read back, and the references -- made once"""
    if (which, kind) not in _CASES:
        B, n_per = LR.shapes(_cap())[which]
        ts = ([0, T - 1, 417] if which % 2 == 0 else [T - 1, 0, 417])[:B]
        pred, x0, a, b, k = LR.case(B, n_per, 100 + which, _schedule(kind), ts)
        seed, draw = SEEDS[which % 2]
        z = fill(B * n_per, seed, draw).cpu().numpy().reshape(B, n_per)
        _CASES[which, kind] = dict(B=B, n_per=n_per, pred=pred, x0=x0, a=a, b=b, k=k, seed=seed, draw=draw, z=z, m=LR.chain_length(n_per, _bps(n_per)))
    return _CASES[which, kind]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------ q_sample
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", range(6))
def test_q_sample_is_x0_a_plus_fill_b_bit_for_bit(which, kind):
    c = _case(which, kind)
    B, n_per, n = c["B"], c["n_per"], c["B"] * c["n_per"]
    assert n_per % 4 == 0 and (which < 5 or (n_per // 4 > 256 * _cap() and _bps(n_per) == _cap()))
    x0, a, b = cu(c["x0"]), cu(c["a"]), cu(c["b"])
    outs = []
    for draw in (c["draw"], c["draw"], c["draw"] + 1):
        buf = torch.full((n + PAD,), 7.0, device="cuda")
        _C().check(q_sample_status(x0, a, b, B, n_per, c["seed"], draw, buf), "prior_q_sample")
        assert bool((buf[n:] == 7.0).all()), "q_sample wrote past n"
        outs.append(buf[:n].reshape(B, n_per).clone())
    want = x0 * a[:, None] + cu(c["z"]) * b[:, None]
    assert torch.equal(_bits(outs[0]), _bits(want)) and torch.equal(_bits(outs[0]), _bits(outs[1])) and not torch.equal(outs[0], outs[2])
    assert np.array_equal(outs[0].cpu().numpy().view(np.int32), LR.q_sample32(c["x0"], c["z"], c["a"], c["b"]).view(np.int32))
    assert torch.equal(x0.cpu(), torch.from_numpy(c["x0"]))                  # the input is left alone


# ------------------------------------------------------------------------------------------------ the loss
def run_loss(c, pred):
    B, n_per = c["B"], c["n_per"]
    x0, a, b = cu(c["x0"]), cu(c["a"]), cu(c["b"])
    need = int(_C().lib().ssdnerf_prior_loss_partials(B, n_per))
    assert need == 2 * B * _bps(n_per)
    out = []
    for sentinel in (7.0, float("nan")):                                     # (the slab needs no initialisation: whatever it held)
        partials = torch.full((need + PAD,), sentinel, device="cuda")
        res = torch.full((2, B + PAD), 7.0, device="cuda")
        _C().check(loss_status(pred, x0, a, b, B, n_per, c["seed"], c["draw"], partials, res[0], res[1]), "prior_loss_v")
        assert bool((res[:, B:] == 7.0).all()) and (bool((partials[need:] == 7.0).all()) if sentinel == 7.0 else bool(partials[need:].isnan().all()))
        out.append(res[:, :B].clone())
    assert torch.equal(_bits(out[0]), _bits(out[1]))                         # two runs: the same bits
    return out[0][0].cpu(), out[0][1].cpu()


def loss_ratios(which, kind, bf16):
    c = _case(which, kind)
    pred = cu(c["pred"]).to(torch.bfloat16) if bf16 else cu(c["pred"])
    msd, x0sq = run_loss(c, pred)
    ref_msd, Bm, ref_x, Bx = LR.loss_ref(pred.float().cpu().numpy(), c["x0"], c["z"], c["a"], c["b"], c["m"])
    return LR.check_le(msd, ref_msd, Bm), LR.check_le(x0sq, ref_x, Bx)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", range(6))
def test_loss_forward_meets_the_fp64_bounds(which, kind, bf16):
    r0, r1 = loss_ratios(which, kind, bf16)
    print(LR.shapes(_cap())[which], kind, "bf16" if bf16 else "fp32", "msd error / bound", round(r0[1], 4), "x0sq", round(r1[1], 4))
    assert r0[0] == 0 and r1[0] == 0, (r0, r1)


@pytest.mark.parametrize("which", [0, 2, 4, 5])
def test_msd_of_the_targets_own_bits_is_exactly_zero(which):
    c = _case(which, "linear")
    target = cu(c["a"])[:, None] * cu(c["z"]) - cu(c["b"])[:, None] * cu(c["x0"])
    assert np.array_equal(target.cpu().numpy().view(np.int32), LR.target32(c["x0"], c["z"], c["a"], c["b"]).view(np.int32))
    msd, x0sq = run_loss(c, target.contiguous())
    assert bool((msd == 0).all()) and bool((x0sq > 0).all())


# ------------------------------------------------------------------------------------------------ the backward
def run_backward(c, pred, with_x0=True):
    B, n_per, n = c["B"], c["n_per"], c["B"] * c["n_per"]
    x0, a, b, k = cu(c["x0"]), cu(c["a"]), cu(c["b"]), cu(c["k"])
    gp = torch.full((n + PAD,), 7.0, device="cuda", dtype=pred.dtype)
    gx = torch.full((n + PAD,), 7.0, device="cuda")
    _C().check(backward_status(pred, x0, a, b, k, B, n_per, c["seed"], c["draw"], gp, gx if with_x0 else None), "prior_loss_v_backward")
    assert bool((gp[n:] == 7.0).all()) and bool((gx[n:] == 7.0).all()) and (with_x0 or bool((gx == 7.0).all()))
    return gp[:n].reshape(B, n_per).clone(), gx[:n].reshape(B, n_per).clone()


def backward_ratios(which, kind, bf16):
    c = _case(which, kind)
    pred = cu(c["pred"]).to(torch.bfloat16) if bf16 else cu(c["pred"])
    p32 = pred.float().cpu().numpy()
    gp, gx = run_backward(c, pred)
    want_g, want_gx = LR.backward32(p32, c["x0"], c["z"], c["a"], c["b"], c["k"])
    want_g = torch.from_numpy(want_g).to(pred.dtype)
    assert torch.equal(_bits(gp.cpu()), _bits(want_g)), "grad_pred differs from the fp32 restatement" + (" rounded to bf16" if bf16 else "")
    assert np.array_equal(gx.cpu().numpy().view(np.int32), want_gx.view(np.int32)), "grad_x0 differs from the fp32 restatement"
    gp_alone, _ = run_backward(c, pred, with_x0=False)
    assert torch.equal(_bits(gp_alone), _bits(gp))                           # grad_x0_out NULL: the same grad_pred, nothing else written
    g, Bg, gx64, Bgx = LR.backward_ref(p32, c["x0"], c["z"], c["a"], c["b"], c["k"], bf16=bf16)
    return LR.check_le(gp.float().cpu(), g, Bg), LR.check_le(gx.cpu(), gx64, Bgx)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", range(6))
def test_backward_equals_the_restatement_and_meets_the_fp64_bounds(which, kind, bf16):
    r0, r1 = backward_ratios(which, kind, bf16)
    print(LR.shapes(_cap())[which], kind, "bf16" if bf16 else "fp32", "grad_pred error / bound", round(r0[1], 4), "grad_x0", round(r1[1], 4))
    assert r0[0] == 0 and r1[0] == 0, (r0, r1)


# ------------------------------------------------------------------------------------------------ refusals and no-ops
def test_refusals_return_an_error_code_and_launch_nothing():
    C = _C()
    c = _case(1, "linear")                                                   # (2, 8)
    x0, a, b, k, pred = cu(c["x0"]), cu(c["a"]), cu(c["b"]), cu(c["k"]), cu(c["pred"])
    new = lambda: torch.full((2, 8), 7.0, device="cuda")
    xt, gp, gx, msd, x0sq, partials = new(), new(), new(), torch.full((2,), 7.0, device="cuda"), torch.full((2,), 7.0, device="cuda"), new()
    q = lambda **kw: q_sample_status(**{**dict(x0=x0, a=a, b=b, B=2, n_per=8, seed=1, draw=0, out=xt), **kw})
    lo = lambda **kw: loss_status(**{**dict(pred=pred, x0=x0, a=a, b=b, B=2, n_per=8, seed=1, draw=0, partials=partials, msd=msd, x0sq=x0sq), **kw})
    bw = lambda **kw: backward_status(**{**dict(pred=pred, x0=x0, a=a, b=b, k=k, B=2, n_per=8, seed=1, draw=0, grad_pred=gp, grad_x0=gx), **kw})
    assert q(x0=None) != 0 and q(a=None) != 0 and q(b=None) != 0 and q(out=None) != 0
    assert q(n_per=6) != 0 and q(out=x0) != 0
    assert b"alias" in C.lib().ssdnerf_last_error()
    assert all(lo(**{name: None}) != 0 for name in ("pred", "x0", "a", "b", "partials", "msd", "x0sq"))
    assert lo(n_per=6) != 0 and lo(dtype=1) != 0 and lo(dtype=3) != 0 and lo(dtype=-1) != 0
    assert b"dtype" in C.lib().ssdnerf_last_error()
    assert all(bw(**{name: None}) != 0 for name in ("pred", "x0", "a", "b", "k", "grad_pred"))
    assert bw(n_per=6) != 0 and bw(dtype=1) != 0 and bw(dtype=7) != 0
    # no-ops, null pointers and all
    assert q(B=0) == 0 and q(n_per=0) == 0 and lo(B=0) == 0 and lo(n_per=0) == 0 and bw(B=0) == 0 and bw(n_per=0) == 0
    assert q(B=0, x0=None, out=None) == 0 and lo(n_per=0, pred=None) == 0
    assert int(C.lib().ssdnerf_prior_loss_partials(0, 8)) == 0
    torch.cuda.synchronize()
    for t in (xt, gp, gx, msd, x0sq, partials):
        assert bool((t == 7).all())
    assert torch.equal(x0.cpu(), torch.from_numpy(c["x0"]))
    assert q() == 0 and lo() == 0 and bw() == 0 and bw(grad_x0=None) == 0    # the same calls, well-formed
    torch.cuda.synchronize()
    assert not bool((xt == 7).any()) and not bool((msd == 7).any()) and not bool((gp == 7).any())


# ------------------------------------------------------------------------------------------------ forward_train, analytic denoiser
MU, S_ = 0.3, 0.5


def _analytic(kind):
    import ssdnerf_amd.unet  # noqa: F401
    from ssdnerf_amd.diffusion import GaussianDiffusion
    from test_sde_cpu import _tiny_unet_cfg
    d = GaussianDiffusion(denoising=_tiny_unet_cfg(), betas_cfg=dict(type=kind), num_timesteps=T, denoising_mean_mode="V",
                          ddpm_loss=dict(type="DDPMMSELossMod", data_info=dict(pred="v_t_pred", target="v_t")))
    d.denoising = DR.GaussianDenoiser(d.schedule, MU, S_)
    return d.eval()


def analytic_ratios(kind, x_t_detach):
    d = _analytic(kind)
    x_np = (MU + S_ * np.random.default_rng(3).normal(size=(2, 18, 16, 16))).astype(np.float32)
    ts = [0, T - 1] if kind == "linear" else [T - 1, 0]
    seed, draw = SEEDS[1]
    x0 = cu(x_np).requires_grad_(True)
    loss, _ = d.forward_train(x0, cfg=dict(noise_source="device"), timesteps=ts, x_t_detach=x_t_detach, noise_seed=seed, noise_draw=draw)
    loss.backward()
    n_per = x_np[0].size
    z = fill(x_np.size, seed, draw).cpu().numpy()
    want, B_loss, grad, B_grad = LR.gaussian_chain_ref(x_np, z, ts, d.schedule, MU, S_, x_t_detach, LR.chain_length(n_per, _bps(n_per)))
    assert float(grad.abs().max()) > 1e-6 and float(want) > 1e-3
    return LR.check_le(loss.detach().cpu().reshape(1), want.reshape(1), B_loss.reshape(1)), LR.check_le(x0.grad.cpu().reshape(2, -1), grad, B_grad)


@pytest.mark.parametrize("x_t_detach", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_forward_train_meets_the_fp64_chain_with_the_analytic_denoiser(kind, x_t_detach, monkeypatch):
    from ssdnerf_amd import diffusion as D
    monkeypatch.setattr(D, "_host_noise", _raise)
    monkeypatch.setattr(D, "_device_noise", _raise)                          # the fused route: no fill either
    r0, r1 = analytic_ratios(kind, x_t_detach)
    print(kind, "x_t_detach" if x_t_detach else "", "loss error / bound", round(r0[1], 4), "code gradient", round(r1[1], 4))
    assert r0[0] == 0 and r1[0] == 0, (r0, r1)


def _raise(*a, **k):
    raise AssertionError("the host draw (or the fill) was asked for in fused device mode")


# ------------------------------------------------------------------------------------------------ forward_train, tiny UNet: fused against generic
_STATE = {}


def _tiny():
    if "d" not in _STATE:
        import ssdnerf_amd  # noqa: F401
        from ssdnerf_amd.diffusion import GaussianDiffusion
        from test_diffusion_gpu import _randomize, _tiny_unet_cfg
        d = GaussianDiffusion(denoising=_tiny_unet_cfg(), betas_cfg=dict(type="linear"), num_timesteps=T, denoising_mean_mode="V",
                              ddpm_loss=dict(type="DDPMMSELossMod", rescale_mode="timestep_weight", data_info=dict(pred="v_t_pred", target="v_t"),
                                             weight_scale=4.0, log_cfgs=dict(type="quartile", prefix_name="loss_mse", total_timesteps=1000)),
                              timestep_sampler=dict(type="SNRWeightedTimeStepSampler", power=0.5))
        _randomize(d, 5)
        _STATE["d"] = d.eval().cuda()
    d = _STATE["d"]
    d.use_fused_step = True
    return d


TINY_T = [700, 150]


def _tiny_run(d, x_np, fused, seed, draw):
    """(x_t the UNet saw, loss, gradient on x_0, quartile logs) of one ``forward_train`` on device noise"""
    seen = []
    hook = d.denoising.register_forward_pre_hook(lambda mod, args: seen.append(args[0].detach().clone()))
    d.use_fused_step = fused
    try:
        x0 = cu(x_np).requires_grad_(True)
        loss, logs = d.forward_train(x0, cfg=dict(noise_source="device"), timesteps=TINY_T, noise_seed=seed, noise_draw=draw)
        loss.backward()
    finally:
        hook.remove()
        d.use_fused_step = True
    return seen[0], loss.detach(), x0.grad.detach().clone(), {k: v.clone() for k, v in logs.items()}


def _tiny_reference(d, x_np, z):
    """the generic chain in float64 on the read-back noise: oracle/diffusion.py's CPU UNet with the product's weights in float64.  Its time-embedding branch
    (the sinusoid the oracle builds in fp32, and the linear layers that only ever see it) stays fp32: it does not depend on x_0, and both paths under
    comparison share it."""
    from oracle import diffusion as OD
    keep32 = lambda k: "time_embedding" in k or "embedding_layer" in k
    sd = {k: (v.detach().cpu().clone() if keep32(k) else v.detach().cpu().double()) for k, v in d.denoising.state_dict().items()}
    t = torch.tensor(TINY_T)
    x0 = torch.from_numpy(x_np).double().requires_grad_(True)
    ab = d.schedule.signal_noise("cpu")[:, t].double()
    a, b = ab[0].reshape(-1, 1, 1, 1), ab[1].reshape(-1, 1, 1, 1)
    zz = torch.from_numpy(z).double().reshape(x0.shape)
    x_t = x0 * a + zz * b
    v = OD.unet_forward(sd, x_t, t, image_size=16, base_channels=32, channels_cfg=(1, 2), resblocks_per_downsample=1, num_heads=4, attention_res=(8,),
                        norm_groups=8)
    assert v.dtype == torch.float64
    per = (v - (a * zz - b * x0)).square().flatten(1).mean(1) * 0.5 * d.ddpm_loss.timestep_weight.cpu().double()[t] * d.ddpm_loss.weight_scale
    loss = per.mean()
    (grad,) = torch.autograd.grad(loss, x0)
    return loss.detach(), grad


def tiny_figures():
    d = _tiny()
    x_np = np.random.default_rng(4).normal(size=(2, 18, 16, 16)).astype(np.float32)
    seed, draw = SEEDS[0]
    xt_f, loss_f, grad_f, logs_f = _tiny_run(d, x_np, True, seed, draw)
    xt_g, loss_g, grad_g, logs_g = _tiny_run(d, x_np, False, seed, draw)
    z = fill(x_np.size, seed, draw).cpu().numpy()
    loss64, grad64 = _tiny_reference(d, x_np, z)
    rel = lambda g: float((g.cpu().double() - grad64).norm() / grad64.norm())
    return dict(x_t_equal=torch.equal(_bits(xt_f), _bits(xt_g)), loss_fused=float(loss_f), loss_generic=float(loss_g), loss_fp64=float(loss64),
                loss_rel_diff=abs(float(loss_f) - float(loss_g)) / abs(float(loss_g)), grad_rel_l2_fused=rel(grad_f), grad_rel_l2_generic=rel(grad_g),
                logs_close=all(abs(float(logs_f[k]) - float(logs_g[k])) <= 2 * x_np[0].size * LR.U32 * abs(float(logs_g[k])) for k in logs_g),
                n_per=int(x_np[0].size))


def test_fused_forward_train_against_the_generic_device_branch_with_a_tiny_unet(monkeypatch):
    """x_t bit-equal; the losses within 2 n_per u relative (both sum the same fp32 terms in different orders: the worst case of any order); the
    gradient on x_0 against the float64 chain through the oracle UNet: the fused path's relative L2 error at most twice the generic path's own (the
    two differ by a handful of roundings in front of the same backward; a wrong coefficient is off by O(1)).  Measured on an MI355X: see
    profiles/prior_loss.json, ``tiny_unet``."""
    from ssdnerf_amd import diffusion as D
    monkeypatch.setattr(D, "_host_noise", _raise)
    f = tiny_figures()
    print(f)
    assert f["x_t_equal"]
    assert f["loss_rel_diff"] <= 2 * f["n_per"] * LR.U32, f
    assert f["logs_close"]
    assert abs(f["loss_fused"] - f["loss_fp64"]) <= 1e-3 * abs(f["loss_fp64"])              # (the reference is this loss, not another)
    assert 0 < f["grad_rel_l2_generic"] < 1e-2 and f["grad_rel_l2_fused"] <= 2 * f["grad_rel_l2_generic"], f


# ------------------------------------------------------------------------------------------------ wiring
def _model():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    from test_recons_gpu import DEC, UNET, _randomize
    hw = 64
    m = MODELS.build(dict(
        type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
        diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"), denoising=dict(UNET), denoising_mean_mode="V",
                       timestep_sampler=dict(type="SNRWeightedTimeStepSampler", power=0.5),
                       ddpm_loss=dict(type="DDPMMSELossMod", rescale_mode="timestep_weight", data_info=dict(pred="v_t_pred", target="v_t"),
                                      weight_scale=4.0, scale_norm=True)),
        decoder=dict(DEC), decoder_use_ema=True, freeze_decoder=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
        reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=4,
        train_cfg=dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=1, n_inverse_rays=hw * hw, n_decoder_rays=hw * hw,
                       loss_coef=0.1 / (hw * hw), optimizer=dict(type="SGD", lr=1.0)),
        test_cfg=dict(img_size=(hw, hw), num_timesteps=2, clip_range=[-2, 2], density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=hw * hw,
                      loss_coef=0.1 / (hw * hw), cond_mode="optim", n_inverse_steps=2, extra_scene_step=1,
                      optimizer=dict(type="Adam", lr=0.005, weight_decay=0.0))))
    _randomize(m.diffusion.denoising, 9)
    _randomize(m.diffusion_ema.denoising, 9)
    params = S.make_decoder_params()
    m.decoder.load_state_dict(params, strict=False)
    m.decoder_ema.load_state_dict(params, strict=False)
    return m.cuda()


def _views(hw=64, seed=41):
    from ssdnerf_amd import synthetic as S
    g = torch.Generator().manual_seed(seed)
    return dict(cond_imgs=torch.rand(1, 1, hw, hw, 3, generator=g).cuda(), cond_poses=S.spiral_poses()[[64]].cuda()[None],
                cond_intrinsics=S.cars_intrinsics(hw, hw).cuda()[None, None])


class _Watch:
    """the host draw and the pinned upload patched to raise (or, ``count_only``, counted); launches of the fill and of the fused loss counted"""

    def __init__(self, monkeypatch, count_only=False):
        from ssdnerf_amd import diffusion as D
        self.n = dict(host_noise=0, fill=0, prior_loss=0, q_sample=0, backward=0)
        lib = _C().lib()
        for key, name in (("fill", "ssdnerf_philox_normal_fill"), ("prior_loss", "ssdnerf_prior_loss_v"), ("q_sample", "ssdnerf_prior_q_sample"),
                          ("backward", "ssdnerf_prior_loss_v_backward")):
            monkeypatch.setattr(lib, name, self._wrap(key, getattr(lib, name)))
        if count_only:
            monkeypatch.setattr(D, "_host_noise", self._wrap("host_noise", D._host_noise))
        else:
            monkeypatch.setattr(D, "_host_noise", _raise)
            monkeypatch.setattr(D._PinnedRing, "upload", classmethod(lambda cls, *a, **k: _raise()))

    def _wrap(self, key, fn):
        def counted(*a, **k):
            self.n[key] += 1
            return fn(*a, **k)
        return counted


def _train_once(m, seed=5):
    m = copy.deepcopy(m).train()
    m.train_cfg.update(noise_source="device", noise_seed=seed)
    opt = dict(diffusion=torch.optim.SGD(m.diffusion.parameters(), lr=1e-3), decoder=torch.optim.SGD(m.decoder.parameters(), lr=0.05))
    np.random.seed(13)
    torch.manual_seed(13)
    out = m.train_step(dict(scene_id=[1], scene_name=["a"], **_views()), opt)
    return out["log_vars"]["loss_ddpm_mse"].clone()


def test_train_step_runs_on_device_noise(monkeypatch):
    m = _STATE.setdefault("model", _model())
    watch = _Watch(monkeypatch)
    before = None
    losses = []
    for _ in range(2):
        losses.append(_train_once(m))
        before = before or dict(watch.n)
    assert before == dict(host_noise=0, fill=0, prior_loss=1, q_sample=1, backward=1), before
    assert bool(torch.isfinite(losses[0])) and torch.equal(_bits(losses[0].reshape(1)), _bits(losses[1].reshape(1))), losses     # seeded alike: the same bits
    assert not torch.equal(losses[0], _train_once(m, seed=6))


def test_val_optim_and_val_uncond_run_on_device_noise(monkeypatch):
    m = copy.deepcopy(_STATE.setdefault("model", _model())).eval()
    for cfg in (m.test_cfg, m.diffusion_ema.test_cfg):
        cfg.update(noise_source="device", noise_seed=21)
    watch = _Watch(monkeypatch)
    np.random.seed(3)
    torch.manual_seed(3)
    state = torch.get_rng_state()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        code, grid, bits = m.val_optim(_views())
    assert not any("val_optim" in str(w.message) for w in caught)            # no warning about a foreign draw: there is no prefetch to protect
    assert code.shape == (1, 3, 6, 128, 128) and bool(torch.isfinite(code).all())
    assert watch.n == dict(host_noise=0, fill=0, prior_loss=2, q_sample=2, backward=2), watch.n
    assert torch.equal(state, torch.get_rng_state())                         # a seed is set: nothing drawn on the host
    noise = torch.randn(1, 3, 6, 128, 128, generator=torch.Generator().manual_seed(4)).cuda()
    code, grid, bits = m.val_uncond(dict(scene_id=[0], noise=noise))         # n_inverse_steps = 2: the sample is polished under the prior
    assert code.shape == (1, 3, 6, 128, 128) and bool(torch.isfinite(code).all())
    assert watch.n == dict(host_noise=0, fill=0, prior_loss=4, q_sample=4, backward=4), watch.n


def test_host_mode_still_draws_on_the_host(monkeypatch):
    m = copy.deepcopy(_STATE.setdefault("model", _model()))
    watch = _Watch(monkeypatch, count_only=True)
    opt = dict(diffusion=torch.optim.SGD(m.diffusion.parameters(), lr=1e-3), decoder=torch.optim.SGD(m.decoder.parameters(), lr=0.05))
    torch.manual_seed(7)
    m.train().train_step(dict(scene_id=[1], scene_name=["a"], **_views()), opt)
    assert watch.n == dict(host_noise=1, fill=0, prior_loss=0, q_sample=0, backward=0), watch.n
    after = torch.get_rng_state()
    torch.manual_seed(7)
    torch.randn(1, 18, 128, 128)
    assert torch.equal(after, torch.get_rng_state())
    torch.manual_seed(7)
    m.eval().val_optim(_views())
    assert watch.n == dict(host_noise=3, fill=0, prior_loss=0, q_sample=0, backward=0), watch.n      # one draw per outer iteration (the second: prefetched)
    after = torch.get_rng_state()
    torch.manual_seed(7)
    for _ in range(2):
        torch.randn(1, 18, 128, 128)
    assert torch.equal(after, torch.get_rng_state())


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = dict(msd=0.0, x0sq=0.0, grad_pred=0.0, grad_x0=0.0, msd_bf16=0.0, grad_pred_bf16=0.0)
    for which in range(6):
        for kind in KINDS:
            for bf16 in (False, True):
                sfx = "_bf16" if bf16 else ""
                r0, r1 = loss_ratios(which, kind, bf16)
                r2, r3 = backward_ratios(which, kind, bf16)
                worst["msd" + sfx], worst["grad_pred" + sfx] = max(worst["msd" + sfx], round(r0[1], 4)), max(worst["grad_pred" + sfx], round(r2[1], 4))
                worst["x0sq"], worst["grad_x0"] = max(worst["x0sq"], round(r1[1], 4)), max(worst["grad_x0"], round(r3[1], 4))
    analytic = {}
    for kind in KINDS:
        for detach in (False, True):
            r0, r1 = analytic_ratios(kind, detach)
            analytic[f"{kind}{'_x_t_detach' if detach else ''}"] = dict(loss=round(r0[1], 4), code_gradient=round(r1[1], 4))
    return dict(worst_ratio=worst, analytic_denoiser=analytic, tiny_unet=tiny_figures())


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = dict(what="worst |kernel - fp64 reference| / bound per output over every case of tests/test_prior_loss_gpu.py; the fused forward_train against "
                    "the fp64 chain (analytic denoiser) and, with a tiny UNet, its gradient's relative L2 error beside the generic device branch's",
               device=torch.cuda.get_device_name(0), **measure())
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
