"""The total-variation regulariser on the MI355X: the kernels (csrc/tv_loss.hip) against the float64 restatement of tests/_tv_ref.py under its
per-element bounds, the reference's own values (tests/golden/tv_loss.npz), flat planes, extreme magnitudes, bit-identical repeats, TVLoss through
TanhCode, and stage-1 fitting: MultiSceneNeRF.train_step and BaseNeRF.val_step with the stage-1 model dict."""
import os

import numpy as np
import pytest
import torch

import _tv_ref as T

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tv_loss.npz")


def _raw(x, g, p):
    """(slice means, gradient) straight from the C ABI"""
    from ssdnerf_amd import _cabi as C
    x = x.contiguous()
    n, h, w = x[..., 0, 0].numel(), x.shape[-2], x.shape[-1]
    means = torch.empty(x.shape[:-2], device=x.device)
    grad = torch.empty_like(x)
    C.check(C.lib().ssdnerf_tv_loss_forward(C.ptr(x), C.u32(n), C.u32(h), C.u32(w), C.f32(p), C.ptr(means), C.stream()), "tv_loss_forward")
    C.check(C.lib().ssdnerf_tv_loss_backward(C.ptr(x), C.ptr(g), C.u32(n), C.u32(h), C.u32(w), C.f32(p), C.ptr(grad), C.stream()), "tv_loss_backward")
    torch.cuda.synchronize()
    return means, grad


def _check(x, p, seed=0):
    g = torch.empty(x.shape[:-2]).uniform_(0.5, 2.0, generator=torch.Generator().manual_seed(seed)).cuda()
    means, grad = _raw(x.cuda(), g, p)
    xs, gs = x.cpu().numpy(), g.cpu().numpy()
    assert T.mean_excess(means.cpu().numpy(), xs, p) <= 1, (tuple(x.shape), p, T.mean_excess(means.cpu().numpy(), xs, p))
    assert T.grad_excess(grad.cpu().numpy(), xs, p, gs) <= 1, (tuple(x.shape), p, T.grad_excess(grad.cpu().numpy(), xs, p, gs))
    return means, grad


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 3.0])
def test_stage1_shape_against_the_restatement(p):
    from ssdnerf_amd import synthetic as S
    planes = torch.stack([S.make_triplane(60 + i) for i in range(4)])                                  # (4, 3, 6, 128, 128)
    rand = torch.randn(4, 3, 6, 128, 128, generator=torch.Generator().manual_seed(1)) * 0.5
    _check(torch.cat([planes, rand]).float(), p)


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 3.0])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 17), (17, 1), (7, 13), (5, 8), (33, 130)])
def test_odd_shapes_against_the_restatement(h, w, p):
    x = torch.randn(2, 3, 5, h, w, generator=torch.Generator().manual_seed(h * 100 + w))
    _check(x, p)
    _check(x[:, :, 1:4], p)                                                                              # a sliced (non-contiguous) view


def test_reference_fixture():
    from ssdnerf_amd.codes import TVLoss
    z = np.load(GOLDEN)
    for k in range(int(z["n_cases"])):
        x, p, weight = z[f"x_{k}"], float(z[f"power_{k}"]), float(z[f"weight_{k}"])
        leaf = torch.from_numpy(x).cuda().requires_grad_(True)
        value = TVLoss(power=p, loss_weight=weight)(leaf)
        value.backward()
        assert value.dim() == 0 and value.dtype == torch.float32
        want = float(z[f"value_{k}"])
        n = z[f"means_{k}"].size                                         # + the fp32 mean over n slices and the product with the weight
        assert abs(float(value) - want) <= (T.mean_c(p) + n + 1) * T.U * abs(want), (k, float(value), want)
        g = np.full(x.shape[:-2], weight / n)
        _, mag = T.grad_ref(x, p, g)
        err = np.abs(leaf.grad.cpu().numpy().astype(np.float64) - z[f"grad_{k}"])
        assert np.all(err <= (T.grad_c(p) + 2) * T.U * mag), (k, float(err.max()))       # + 2: the fp32 upstream weight / n


@pytest.mark.parametrize("p", [1.0, 1.5, 3.0])
def test_flat_and_piecewise_constant_planes(p):
    x = torch.full((2, 3, 6, 32, 32), 0.25)
    x[1, :, :, 10:, 7:] = -1.5                                                                          # one step edge per slice of scene 1
    means, grad = _check(x, p)
    assert bool((means[0] == 0).all()) and bool((grad[0] == 0).all())
    assert torch.isfinite(grad).all() and torch.isfinite(means).all()
    _, mag = T.grad_ref(x.numpy(), p, np.ones(x.shape[:-2]))
    assert bool((grad[1].cpu()[torch.from_numpy(mag[1] == 0)] == 0).all())                                # flat away from the edge: exactly 0


@pytest.mark.parametrize("scale", [1e3, 1e-3])
def test_extreme_magnitudes(scale):
    x = torch.randn(2, 3, 6, 64, 64, generator=torch.Generator().manual_seed(11)) * scale
    for p in (1.0, 1.5, 2.0, 3.0):
        _check(x, p)


def test_bench_shape_is_bit_identical_between_calls():
    x = torch.randn(8, 3, 6, 128, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    g = torch.rand(8, 3, 6, device="cuda")
    m0, g0 = _raw(x, g, 1.5)
    m1, g1 = _raw(x, g, 1.5)
    assert torch.equal(m0, m1) and torch.equal(g0, g1)


def _torch_restatement(t, p):
    """the reference's expression (diff, cat, stack, norm, pow, mean) in PyTorch"""
    diffs = []
    for dim in (-2, -1):
        pad = list(t.shape)
        pad[dim] = 1
        diffs.append(torch.cat([torch.diff(t, dim=dim), t.new_zeros(pad)], dim=dim))
    return torch.stack(diffs, dim=0).norm(dim=0).pow(p).mean(dim=(-2, -1)).mean()


def test_tvloss_through_tanhcode_matches_autograd():
    from ssdnerf_amd.codes import TanhCode, TVLoss
    from ssdnerf_amd.tv_loss import tv_slice_means
    leaf = (torch.randn(2, 3, 6, 128, 128, generator=torch.Generator().manual_seed(3)) * 0.3).cuda().requires_grad_(True)
    act = TanhCode(scale=2)
    loss = TVLoss(power=1.5, loss_weight=1.7)(act(leaf))
    loss.backward()
    ref_leaf = leaf.detach().double().requires_grad_(True)
    ref = _torch_restatement(act(ref_leaf), 1.5) * 1.7
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    err = (leaf.grad.double() - ref_leaf.grad).abs()
    assert float(err.max()) <= 1e-5 * float(ref_leaf.grad.abs().max()), float(err.max())
    with pytest.raises(TypeError):
        tv_slice_means(leaf.detach().double())


# ---------------------------------------------------------------------------------------------- stage-1 fitting with the stage-1 model dict
DEC = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[6 * 3, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
           dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)


def _stage1_model(train_cfg=None, test_cfg=None):
    """paper_cfgs/stage1_cars_recons16v.py's model dict (TVLoss power 1.5), with the synthetic decoder"""
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
                          decoder=DEC, decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=2458, init_from_mean=True,
                          train_cfg=train_cfg or {}, test_cfg=test_cfg or {}))
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    with torch.no_grad():           # the running mean code a trained model would hold (all zeros would render an empty grid: no gradient)
        m.init_code.copy_(S.make_triplane(80))
    return m.cuda()


def _views(scene_seeds, view_ids, size=64):
    """(images, poses, intrinsics) of synthetic scenes, rendered as test_rows_gpu.py renders its targets"""
    from ssdnerf_amd import nerf, synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.density import get_density
    dec = TriPlaneDecoder(**{k: v for k, v in DEC.items() if k != "type"})
    dec.load_state_dict(S.make_decoder_params(), strict=False)
    dec = dec.cuda().eval()
    codes = torch.stack([S.make_triplane(s) for s in scene_seeds]).cuda()
    n = len(scene_seeds)
    with torch.no_grad():
        _, bits = get_density(dec, codes, 64, density_thresh=0.1, density_step=4)
        poses = S.spiral_poses()[view_ids].cuda()[None].expand(n, -1, -1, -1).contiguous()
        intr = S.cars_intrinsics(size, size).cuda()[None, None].expand(n, len(view_ids), -1).contiguous()
        image, _ = nerf.render(dec, codes, bits, size, size, intr, poses)
    return image.clamp(0, 1), poses, intr


def test_stage1_train_step_runs_on_the_tv_regulariser(tmp_path):
    """Fails without the HIP TVLoss: the stage-1 reg_loss used to be a stub that raised on its first call."""
    train_cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=2, n_inverse_rays=2 ** 12, n_decoder_rays=2 ** 12,
                     loss_coef=0.1 / (64 * 64), optimizer=dict(type="Adam", lr=1e-2, weight_decay=0.), save_dir=str(tmp_path / "cache"))
    m = _stage1_model(train_cfg=train_cfg).train()
    imgs, poses, intr = _views([51, 52], [30, 150])
    data = dict(scene_id=[0, 2], scene_name=["s0", "s2"], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr)
    opt = dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    torch.manual_seed(1)
    out1 = m.train_step(data, opt)
    code_1 = m.cache[2]["param"]["code_"].clone()
    out2 = m.train_step(data, opt)
    for out in (out1, out2):
        assert out["num_samples"] == 2
        for k in ("reg_loss", "pixel_loss", "loss", "train_psnr", "code_rms"):
            assert bool(torch.isfinite(torch.as_tensor(out["log_vars"][k]).float()).all()), k
        assert float(out["log_vars"]["reg_loss"]) > 0
    assert float(code_1.abs().max()) > 0 and not torch.equal(m.cache[2]["param"]["code_"], code_1)
    assert sorted(os.listdir(tmp_path / "cache")) == ["s0.pth", "s2.pth"]


TEST_VIEWS, COND_VIEWS = [20, 100, 180], [0, 60, 120, 200]


def _val_batch(scene_seeds, names):
    imgs, poses, intr = _views(scene_seeds, COND_VIEWS)
    timgs, tposes, tintr = _views(scene_seeds, TEST_VIEWS)
    return dict(scene_name=names, cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr, test_poses=tposes, test_intrinsics=tintr,
                test_imgs=timgs.cpu())


def _draws(n_scenes, n_steps, seed):
    g = torch.Generator().manual_seed(seed)
    march = [torch.rand(n_scenes, 2 ** 12, generator=g).cuda() for _ in range(n_steps)]
    jitter = [torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range((n_steps + 15) // 16)]
    return dict(march_noises=march, density_jitters=jitter)


def _tv(code):
    from ssdnerf_amd.tv_loss import tv_slice_means
    return float(tv_slice_means(code.float().contiguous(), 1.5).mean())


def test_stage1_val_step_reconstructs_and_scores(tmp_path):
    """Fails without BaseNeRF.val_step: MultiSceneNeRF had no val_step at all."""
    from ssdnerf_amd import parallel
    test_cfg = dict(img_size=(64, 64), density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 12, loss_coef=0.1 / (64 * 64), n_inverse_steps=30,
                    optimizer=dict(type="Adam", lr=0.08, weight_decay=0.), lr_scheduler=dict(type="ExponentialLR", gamma=0.998))
    m = _stage1_model(test_cfg=test_cfg).eval()
    data = _val_batch([71, 72], ["a", "b"])

    def run(steps, weight=1.0, save_dir=None):
        m.test_cfg.update(n_inverse_steps=steps)
        m.test_cfg.pop("save_dir", None)
        if save_dir is not None:
            m.test_cfg["save_dir"] = save_dir
        m.reg_loss.loss_weight = weight
        torch.manual_seed(3)
        return m.val_step(data, **_draws(2, steps, 4))

    out = run(30, save_dir=str(tmp_path / "scenes"))
    lv = out["log_vars"]
    assert set(lv) == {"test_psnr", "test_ssim", "train_psnr", "code_rms"}
    assert all(np.isfinite(v) for v in lv.values()), lv
    assert out["num_samples"] == 2 and out["code"].shape == (2, 3, 6, 128, 128)
    assert out["test_metrics"]["psnr"].shape == (2, 3) and lv["test_psnr"] == pytest.approx(float(out["test_metrics"]["psnr"].mean()), rel=1e-6)
    pred = out["pred_imgs"]
    assert pred.shape == (2, 3, 3, 64, 64) and torch.equal(torch.round(pred * 255) / 255, pred)
    one = run(1)
    assert lv["train_psnr"] > one["log_vars"]["train_psnr"], (lv["train_psnr"], one["log_vars"]["train_psnr"])

    files = sorted(os.listdir(tmp_path / "scenes"))
    assert files == ["a.pth", "b.pth"]
    entries = [torch.load(tmp_path / "scenes" / f) for f in files]
    code, grid, bits = m.load_scene(dict(code=entries), load_density=True)
    assert torch.equal(code, out["code"]) and torch.equal(grid, out["density_grid"]) and torch.equal(bits, out["density_bitfield"])

    # evaluate_3d over two batches of the saved scenes (2 + 1): the scene-weighted means of what val_step logs per batch
    cached = [dict(data, code=entries), dict({k: v[:1] for k, v in data.items()}, code=entries[:1])]
    per = [m.val_step(b)["log_vars"] for b in cached]
    got = parallel.evaluate_3d(m, cached)
    for key in ("test_psnr", "test_ssim", "code_rms"):
        assert got[key] == pytest.approx((2 * per[0][key] + per[1][key]) / 3, rel=1e-6), key
    m.test_cfg.update(n_inverse_steps=1)
    fitted = parallel.evaluate_3d(m, [data], **_draws(2, 1, 4))
    assert {"test_psnr", "test_ssim", "train_psnr", "code_rms"} <= set(fitted) and all(np.isfinite(float(v)) for v in fitted.values())

    # on the same seeds and draws, a heavy TV weight leaves a smoother code than weight 0
    heavy, none = run(30, weight=100.0), run(30, weight=0.0)
    assert _tv(heavy["code"]) < _tv(none["code"]), (_tv(heavy["code"]), _tv(none["code"]))
