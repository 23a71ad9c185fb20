"""CPU tests of the prior loss on device noise: the error bounds tests/test_prior_loss_gpu.py holds csrc/prior_loss.hip to (tests/_prior_loss_ref.py:
they accept fp32 emulations with two summation orders and reject six wrong formulas), and the plumbing of ``cfg['noise_source']`` in
``GaussianDiffusion.forward_train`` with the fill replaced by the numpy restatement, as tests/test_sde_cpu.py does: how loss draws are numbered, where
the seed comes from, what the host generator is asked for, refusals, and ``DDPMMSELossMod.forward_msd`` against ``forward``."""
import copy

import numpy as np
import pytest
import torch

import _dpmpp_ref as DR
import _prior_loss_ref as LR
import test_sde_cpu as TS

CAP = 512                                                                    # (any cap serves the emulations; the GPU tests ask the library)


# ------------------------------------------------------------------------------------------------ the bounds
def _z(B, n_per, seed=1234, draw=(1 << 31) | 3):
    return LR.normals32(seed, draw, B * n_per).reshape(B, n_per)


@pytest.mark.parametrize("order,shape", [("sequential", (3, 124)), ("pairwise", (3, 4100)), ("pairwise", (2, 1024)), ("sequential", (1, 4))])
def test_bounds_accept_the_fp32_emulation(order, shape):
    B, n_per = shape
    pred, x0, a, b, k = LR.case(B, n_per, 5)
    z = _z(B, n_per)
    m = LR.emulation_chain(n_per, order)
    for bf16 in (False, True):
        p = torch.from_numpy(pred).to(torch.bfloat16).float().numpy() if bf16 else pred
        msd, Bm, x0sq, Bx = LR.loss_ref(p, x0, z, a, b, m)
        d32 = LR.diff32(p, x0, z, a, b)
        r0 = LR.check_le(LR.mean_sq32(d32, order), msd, Bm)
        r1 = LR.check_le(LR.mean_sq32(x0, order), x0sq, Bx)
        g, Bg, gx, Bgx = LR.backward_ref(p, x0, z, a, b, k, bf16=bf16)
        g32, gx32 = LR.backward32(p, x0, z, a, b, k)
        got_g = torch.from_numpy(g32).to(torch.bfloat16).float() if bf16 else g32
        r2, r3 = LR.check_le(got_g, g, Bg), LR.check_le(gx32, gx, Bgx)
        print(order, shape, "bf16" if bf16 else "fp32", "msd", round(r0[1], 3), "x0sq", round(r1[1], 3), "grad_pred", round(r2[1], 3), "grad_x0", round(r3[1], 3))
        assert r0[0] == 0 and r1[0] == 0 and r2[0] == 0 and r3[0] == 0, (r0, r1, r2, r3)
        if n_per >= 1000:
            assert r2[1] > 0.05 and r3[1] > 0.05                             # the element bounds are of the size of the error, not far above it
    d, delta = LR.element_ref(pred, x0, z, a, b)
    assert LR.check_le(LR.diff32(pred, x0, z, a, b), d, delta)[0] == 0
    xt = (torch.from_numpy(x0).double() * torch.from_numpy(a).double()[:, None] + torch.from_numpy(z).double() * torch.from_numpy(b).double()[:, None])
    assert float((torch.from_numpy(LR.q_sample32(x0, z, a, b)).double() - xt).abs().max()) <= 3 * LR.U32 * float(xt.abs().max() + 6)


def test_msd_of_the_targets_own_bits_is_zero_in_the_restatement():
    pred, x0, a, b, _ = LR.case(3, 1020, 6)
    z = _z(3, 1020)
    d = LR.diff32(LR.target32(x0, z, a, b), x0, z, a, b)
    assert not d.any() and float(LR.mean_sq32(d, "pairwise").max()) == 0.0


@pytest.mark.parametrize("wrong", ["target_sign", "a_b_exchanged", "sum_for_mean", "next_samples_coefficients", "next_draw", "grad_x0_minus_b"])
def test_bounds_reject_wrong_formulas(wrong):
    B, n_per = 3, 1020
    pred, x0, a, b, k = LR.case(B, n_per, 7)
    z = _z(B, n_per)
    m = LR.emulation_chain(n_per, "pairwise")
    msd, Bm, _, _ = LR.loss_ref(pred, x0, z, a, b, m)
    g, Bg, gx, Bgx = LR.backward_ref(pred, x0, z, a, b, k)
    aa, bb, zz = a, b, z
    if wrong == "a_b_exchanged":
        aa, bb = b, a
    elif wrong == "next_samples_coefficients":
        aa, bb = np.roll(a, -1), np.roll(b, -1)
    elif wrong == "next_draw":
        zz = _z(B, n_per, draw=((1 << 31) | 3) + 1)
    d32 = LR.diff32(pred, x0, zz, aa, bb)
    if wrong == "target_sign":
        d32 = pred - (LR._col(a) * z + LR._col(b) * x0)
    got_msd = LR.mean_sq32(d32, "pairwise")
    if wrong == "sum_for_mean":
        got_msd = got_msd * np.float32(n_per)
    got_g = LR._col(k) * d32
    got_gx = got_g * LR._col(bb)
    if wrong == "grad_x0_minus_b":
        got_gx = -got_gx
        bad, ratio = LR.check_le(got_gx, gx, Bgx)
        assert bad > 0.9 * gx.numel() and ratio > 100, (bad, ratio)
        assert LR.check_le(got_msd, msd, Bm)[0] == 0 and LR.check_le(got_g, g, Bg)[0] == 0       # (nothing else is wrong)
        return
    bad, ratio = LR.check_le(got_msd, msd, Bm)
    assert bad == B and ratio > 100, (wrong, bad, ratio)
    if wrong != "sum_for_mean":
        bad, ratio = LR.check_le(got_g, g, Bg)
        assert bad > 0.9 * g.numel() and ratio > 100, (wrong, bad, ratio)
        bad, ratio = LR.check_le(got_gx, gx, Bgx)
        assert bad > 0.9 * gx.numel() and ratio > 100, (wrong, bad, ratio)


def test_chain_length_and_geometry():
    assert LR.blocks_per_sample(4, CAP) == 1 and LR.blocks_per_sample(1024, CAP) == 1 and LR.blocks_per_sample(1028, CAP) == 2
    big = LR.shapes(CAP)[-1][1]
    assert LR.blocks_per_sample(big, CAP) == CAP and big // 4 == 256 * CAP + 1
    assert LR.chain_length(4, 1) == 4 + 6 + 3 + 1 + 6 and LR.chain_length(big, CAP) == 8 + 6 + 3 + CAP // 64 + 6
    assert LR.chain_length(18 * 128 * 128, LR.blocks_per_sample(18 * 128 * 128, CAP)) == 4 + 6 + 3 + 5 + 6     # a cars latent: one trip


# ------------------------------------------------------------------------------------------------ plumbing
_LOSS_FIELDS = {"EPS": dict(pred="eps_t_pred", target="noise"), "START_X": dict(pred="x_0_pred", target="x_0"), "V": dict(pred="v_t_pred", target="v_t")}


def _diffusion(kind="cosine", mode="V"):
    from ssdnerf_amd.diffusion import DDPMMSELossMod
    d = TS._diffusion(kind)
    d.denoising = DR.GaussianDenoiser(d.schedule, 0.3, 0.5)
    d.ddpm_loss = DDPMMSELossMod(data_info=_LOSS_FIELDS[mode], log_cfgs=dict(type="quartile", prefix_name="loss_mse", total_timesteps=1000))
    d.test_cfg = dict()
    for key in ("_loss_own_seed", "_loss_draws"):
        d.__dict__.pop(key, None)
    return d


def _x0(batch=2, seed=3):
    return torch.randn(batch, 18, 16, 16, generator=torch.Generator().manual_seed(seed))


@pytest.fixture
def cpu_stand_in(monkeypatch):
    """device mode without a device: the fill replaced by the float64 restatement rounded to fp32, the latent check switched off; records (seed, draw)"""
    from ssdnerf_amd import diffusion as D
    calls = []

    def fill(like, seed, draw):
        calls.append((seed, draw))
        return torch.from_numpy(LR.normals32(seed, draw, like.numel())).reshape(like.shape)

    monkeypatch.setattr(D, "_device_noise", fill)
    monkeypatch.setattr(D, "_require_device_latent", lambda x: None)
    return calls


T2 = [0, 999]
BASE = 1 << 31


def test_loss_draws_are_numbered_from_2_to_the_31_per_seed(cpu_stand_in):
    d, x0 = _diffusion(), _x0()
    cfg = dict(noise_source="device", noise_seed=7)
    vals = [d.forward_train(x0, cfg=cfg, timesteps=T2)[0] for _ in range(3)]
    assert cpu_stand_in == [(7, BASE), (7, BASE + 1), (7, BASE + 2)]
    assert not torch.equal(vals[0], vals[1])
    del cpu_stand_in[:]
    d.forward_train(x0, cfg=dict(cfg, noise_seed=(1 << 64) + 9), timesteps=T2)       # another seed (taken mod 2^64): its own count
    d.forward_train(x0, cfg=dict(cfg, noise_seed=9), timesteps=T2)
    d.forward_train(x0, cfg=cfg, timesteps=T2)
    assert cpu_stand_in == [(9, BASE), (9, BASE + 1), (7, BASE)]
    del cpu_stand_in[:]
    a, _ = d.forward_train(x0, cfg=cfg, timesteps=T2, noise_seed=11, noise_draw=5)   # both named: the counter is left alone
    d.forward_train(x0, cfg=cfg, timesteps=T2, noise_seed=11)                         # the seed named: counted under it
    d.forward_train(x0, cfg=cfg, timesteps=T2)
    assert cpu_stand_in == [(11, 5), (11, BASE), (7, BASE)]
    # the value is the host formula on the restatement's normals
    z = torch.from_numpy(LR.normals32(11, 5, x0.numel())).reshape(x0.shape)
    want, _ = d.forward_train(x0, timesteps=T2, noise=z)
    assert torch.equal(a, want)
    d.__dict__["_loss_draws"] = (7, BASE)
    with pytest.raises(RuntimeError, match="2\\^31"):
        d.forward_train(x0, cfg=cfg, timesteps=T2)
    assert "_loss_draws" not in d.state_dict() and "_loss_own_seed" not in d.state_dict()   # the counter is not checkpointed


def test_seed_takes_the_rank_offset_mod_2_to_the_64(cpu_stand_in, monkeypatch):
    d, x0 = _diffusion(), _x0()
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: True)
    monkeypatch.setattr(torch.distributed, "get_rank", lambda: 3)
    d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=7), timesteps=T2)
    d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=(1 << 64) - 1), timesteps=T2)
    d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=7), timesteps=T2, noise_seed=7)      # a named seed is taken as it is
    assert cpu_stand_in == [(10, BASE), (2, BASE), (7, BASE)]


def test_with_a_seed_nothing_is_drawn_on_the_host_without_one_exactly_once_per_object(cpu_stand_in):
    d, x0 = _diffusion(), _x0()
    other = copy.deepcopy(d)
    torch.manual_seed(3)
    before = torch.get_rng_state()
    d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=7))       # (timesteps: the sampler's np.random draw)
    assert torch.equal(before, torch.get_rng_state())
    del cpu_stand_in[:]
    for _ in range(3):
        d.forward_train(x0, cfg=dict(noise_source="device"), timesteps=T2)
    after = torch.get_rng_state()
    seeds = {s for s, _ in cpu_stand_in}
    assert len(seeds) == 1 and [k for _, k in cpu_stand_in] == [BASE, BASE + 1, BASE + 2]
    torch.manual_seed(3)
    lo, hi = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
    assert seeds == {(hi << 32) | lo} and torch.equal(after, torch.get_rng_state())   # torch.manual_seed reproduces the run
    other.forward_train(x0, cfg=dict(noise_source="device"), timesteps=T2)    # another object: its own seed draw, its own count
    assert cpu_stand_in[-1][1] == BASE and cpu_stand_in[-1][0] not in seeds


def test_host_mode_draws_one_randn_of_the_latents_shape_per_call(cpu_stand_in):
    d, x0 = _diffusion(), _x0()
    torch.manual_seed(5)
    a, _ = d.forward_train(x0, timesteps=T2)
    b, _ = d.forward_train(x0, cfg=dict(noise_source="host"), timesteps=T2)
    after = torch.get_rng_state()
    torch.manual_seed(5)
    za, zb = torch.randn(x0.shape), torch.randn(x0.shape)
    assert torch.equal(after, torch.get_rng_state()) and cpu_stand_in == []
    assert torch.equal(a, d.forward_train(x0, timesteps=T2, noise=za)[0]) and torch.equal(b, d.forward_train(x0, timesteps=T2, noise=zb)[0])


def test_injected_noise_wins(cpu_stand_in):
    d, x0 = _diffusion(), _x0()
    z = torch.randn(x0.shape, generator=torch.Generator().manual_seed(8))
    torch.manual_seed(1)
    before = torch.get_rng_state()
    got, _ = d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=7), timesteps=T2, noise=z)
    assert cpu_stand_in == [] and torch.equal(before, torch.get_rng_state()) and "_loss_draws" not in d.__dict__
    assert torch.equal(got, d.forward_train(x0, timesteps=T2, noise=z)[0])


def test_refusals():
    d, x0 = _diffusion(), _x0()
    with pytest.raises(ValueError, match="noise_source"):
        d.forward_train(x0, cfg=dict(noise_source="philox"), timesteps=T2)
    with pytest.raises(ValueError, match="GPU"):
        d.forward_train(x0, cfg=dict(noise_source="device", noise_seed=1), timesteps=T2)       # a CPU latent
    with pytest.raises(ValueError, match="GPU"):
        d.forward_train(x0, timesteps=T2, noise_seed=1)


@pytest.mark.parametrize("mode", ["EPS", "START_X", "V"])
def test_other_mean_modes_and_guidance_see_the_same_noise(cpu_stand_in, mode):
    d, x0 = _diffusion(mode=mode), _x0()
    d.denoising_mean_mode = mode
    try:
        z = torch.from_numpy(LR.normals32(7, BASE, x0.numel())).reshape(x0.shape)
        for guide in (None, lambda x: (x ** 2).sum()):
            for key in ("_loss_draws",):
                d.__dict__.pop(key, None)
            cfg = dict(noise_source="device", noise_seed=7, grad_through_unet=False, guidance_gain=0.1)
            got, _ = d.forward_train(x0, cfg=cfg, timesteps=T2, grad_guide_fn=guide)
            want, _ = d.forward_train(x0, cfg=dict(cfg, noise_source="host"), timesteps=T2, grad_guide_fn=guide, noise=z)
            assert torch.equal(got, want) and bool(torch.isfinite(got))
    finally:
        d.denoising_mean_mode = "V"


# ------------------------------------------------------------------------------------------------ DDPMMSELossMod.forward_msd
@pytest.mark.parametrize("scale_norm", [False, True])
@pytest.mark.parametrize("reduction", ["mean", "sum", "none", "flatmean"])
def test_forward_msd_equals_forward_to_the_last_bit(scale_norm, reduction):
    from ssdnerf_amd.diffusion import DDPMMSELossMod
    g = torch.Generator().manual_seed(4)
    B = 4
    # x_0 from a few dyadic values: every partial sum of its squares is exact in fp32, so mean(x_0^2) over the tensor and the mean of the per-sample
    # means are the same number -- 'the same numbers' for both entries
    x0 = torch.tensor([0.5, 1.0, -1.5, 2.0])[torch.randint(0, 4, (B, 2, 4, 4), generator=g)]
    pred, target = torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g)
    t = torch.tensor([0, 300, 620, 999])
    table = torch.rand(1000, generator=g) + 0.5
    mods = [DDPMMSELossMod(rescale_mode="timestep_weight", weight=table, weight_scale=1.7, reduction=reduction, scale_norm=scale_norm, momentum=0.1,
                           log_cfgs=dict(type="quartile", prefix_name="loss_mse", total_timesteps=1000), data_info=dict(pred="v_t_pred", target="v_t"))
            for _ in range(2)]
    for m in mods:
        m.train()
    for _ in range(2):                                                       # (twice: the second call divides by a norm_factor that has moved)
        a = mods[0](dict(v_t_pred=pred, v_t=target, x_0=x0, timesteps=t))
        msd = (pred - target).square().flatten(1).mean(dim=1)
        x0sq = x0.square().flatten(1).mean(dim=1)
        assert torch.equal(x0sq.mean(), x0.square().mean())
        b = mods[1].forward_msd(msd, t, x0sq)
        assert a.shape == b.shape and torch.equal(a, b)
        assert set(mods[0].log_vars) == set(mods[1].log_vars) == {f"loss_mse_quartile_{q}" for q in range(4)}
        assert all(torch.equal(mods[0].log_vars[k], mods[1].log_vars[k]) for k in mods[0].log_vars)
        if scale_norm:
            assert torch.equal(mods[0].norm_factor, mods[1].norm_factor) and float(mods[0].norm_factor) != 1.0
    mods[1].eval()                                                            # eval mode: norm_factor stays
    if scale_norm:
        keep = mods[1].norm_factor.clone()
        mods[1].forward_msd(msd, t, x0sq)
        assert torch.equal(keep, mods[1].norm_factor)
