"""Test-view PSNR / SSIM on the MI355X: the fused kernel (csrc/metrics.hip) against the float64 restatement (tests/_metrics_ref.py) over shapes
and contents, its exact cases, determinism at the bench shape, and the scores DiffusionNeRF.val_step and parallel.evaluate_3d report."""
import pytest
import torch

from _metrics_ref import C1, mse_psnr_ref, ssim_ref

pytestmark = pytest.mark.gpu


def _raw(pred, target):
    """(mse, ssim) straight from the C ABI, one value per image pair"""
    from ssdnerf_amd import _cabi as C
    mse = torch.empty(pred[..., 0, 0, 0].numel(), device=pred.device)
    ssim = torch.empty_like(mse)
    a, b = pred.contiguous(), target.contiguous()
    C.check(C.lib().ssdnerf_image_metrics(C.ptr(a), C.ptr(b), C.u32(mse.numel()), C.u32(pred.shape[-3]), C.u32(pred.shape[-2]), C.ptr(mse),
                                          C.ptr(ssim), C.stream()), "image_metrics")
    torch.cuda.synchronize()
    return mse, ssim


def _check_against_restatement(pred, target):
    from ssdnerf_amd.metrics import image_metrics
    psnr, ssim = image_metrics(pred, target)
    torch.cuda.synchronize()
    assert psnr.shape == ssim.shape == pred.shape[:-3] and psnr.dtype == ssim.dtype == torch.float32
    p, t = pred.reshape(-1, *pred.shape[-3:]).cpu().numpy(), target.reshape(-1, *pred.shape[-3:]).cpu().numpy()
    for i, (got_psnr, got_ssim) in enumerate(zip(psnr.flatten().tolist(), ssim.flatten().tolist())):
        mse, want_psnr = mse_psnr_ref(p[i], t[i])
        assert abs(got_ssim - ssim_ref(p[i], t[i])) <= 2e-6, (i, got_ssim, ssim_ref(p[i], t[i]))
        assert abs(got_psnr - want_psnr) <= 1e-4, (i, got_psnr, want_psnr)
    mse, ssim2 = _raw(pred, target)
    assert torch.equal(ssim2, ssim.flatten())
    for i, got in enumerate(mse.tolist()):
        want, _ = mse_psnr_ref(p[i], t[i])
        assert abs(got - want) <= 1e-6 * want, (i, got, want)
    return psnr, ssim


def _near_flat(n, h, w, g):
    """bright nearly flat views, quantised to k/255, and a copy that differs by +-1/255 in patches: the rendered background edge, where
    E[x^2] - E[x]^2 in fp32 misses the SSIM by up to 6.5e-5"""
    base = torch.round(0.92 * 255 + torch.randint(-1, 2, (n, h, w, 3), generator=g).float()) / 255
    patch = torch.rand(n, h // 4 + 1, w // 4 + 1, 1, generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :h, :w] < 0.5
    step = torch.randint(-1, 2, (n, h, w, 3), generator=g).float() / 255
    return base, (base + patch * step).clamp(0, 1)


@pytest.mark.parametrize("n,h,w", [(16, 128, 128), (3, 7, 7), (3, 9, 13), (2, 97, 130), (2, 64, 400)])
def test_kernel_matches_restatement_random_and_near_flat(n, h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    a, b = torch.rand(n, h, w, 3, generator=g), torch.rand(n, h, w, 3, generator=g)
    _check_against_restatement(a.cuda(), b.cuda())
    x, y = _near_flat(n, h, w, g)
    _check_against_restatement(x.cuda(), y.cuda())


def test_kernel_matches_restatement_on_rendered_views():
    from ssdnerf_amd import nerf, synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.density import get_density
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256)
    dec.load_state_dict(S.make_decoder_params(), strict=False)
    dec = dec.cuda().eval()
    code = torch.stack([S.make_triplane(21), S.make_triplane(22)]).cuda()
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():
        _, bits = get_density(dec, code, 64, density_thresh=0.1, density_step=4, jitters=[torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(4)])
        poses = S.spiral_poses()[[5, 70, 150, 220]].cuda()[None].expand(2, -1, -1, -1).contiguous()
        intr = S.cars_intrinsics(128, 128).cuda()[None, None].expand(2, 4, -1).contiguous()
        image, _ = nerf.render(dec, code, bits, 128, 128, intr, poses, grid_size=64, bg_color=1.0)
    pred = torch.round(image.clamp(0, 1) * 255) / 255
    assert pred.shape == (2, 4, 128, 128, 3) and float(pred.min()) < 0.9          # something was rendered
    noisy = (pred + 0.03 * torch.randn(pred.shape, generator=g).cuda()).clamp(0, 1)
    shifted = torch.roll(pred, shifts=(1, 2), dims=(2, 3))
    _, s_noisy = _check_against_restatement(pred, noisy)
    _, s_shift = _check_against_restatement(pred, shifted)
    assert float(s_noisy.max()) < 1 and float(s_shift.max()) < 1


def test_exact_cases():
    from ssdnerf_amd.metrics import image_metrics
    g = torch.Generator().manual_seed(5)
    x = torch.rand(4, 33, 41, 3, generator=g).cuda()
    mse, ssim = _raw(x, x.clone())
    assert bool((ssim == 1.0).all()) and bool((mse == 0).all()), (ssim, mse)
    psnr, ssim = image_metrics(x, x.clone())
    assert bool((ssim == 1.0).all()) and float((psnr - 60).abs().max()) < 1e-4, psnr        # -10 log10(0 + 1e-6)
    for p, q in [(0.25, 0.75), (0.9, 0.9 + 1 / 255), (0.0, 1.0)]:
        _, s = image_metrics(torch.full((2, 12, 9, 3), p).cuda(), torch.full((2, 12, 9, 3), q).cuda())
        want = (2 * p * q + C1) / (p * p + q * q + C1)
        assert float((s.double() - want).abs().max()) <= 2e-6, (p, q, s, want)


def test_wrapper_rejects_unconverted_inputs_and_takes_strided_ones():
    from ssdnerf_amd.metrics import image_metrics
    x = torch.rand(2, 16, 16, 3, device="cuda")
    with pytest.raises(TypeError):
        image_metrics(x.half(), x.half())
    with pytest.raises(ValueError):
        image_metrics(x.cpu(), x.cpu())
    with pytest.raises(ValueError):
        image_metrics(x[..., :2], x[..., :2])
    with pytest.raises(ValueError):
        image_metrics(x.permute(0, 3, 1, 2), x.permute(0, 3, 1, 2))
    with pytest.raises(RuntimeError, match="7 x 7"):
        image_metrics(x[:, :6], x[:, :6])
    y = torch.rand(16, 2, 16, 3, device="cuda").transpose(0, 1)                 # non-contiguous
    p0, s0 = image_metrics(x, y)
    p1, s1 = image_metrics(x, y.contiguous())
    assert torch.equal(p0, p1) and torch.equal(s0, s1)


def test_bench_shape_is_bit_identical_between_calls():
    from ssdnerf_amd.metrics import image_metrics
    g = torch.Generator(device="cuda").manual_seed(9)
    a = torch.rand(8, 251, 128, 128, 3, device="cuda", generator=g)
    b = (a + 0.05 * torch.randn(a.shape, device="cuda", generator=g)).clamp(0, 1)
    p0, s0 = image_metrics(a, b)
    p1, s1 = image_metrics(a, b)
    assert p0.shape == (8, 251)
    assert torch.equal(p0, p1) and torch.equal(s0, s1)


# ---------------------------------------------------------------------------------------------- val_step / evaluate_3d
@pytest.fixture(scope="module")
def model_and_scenes():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    cfg = dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2),
               grid_size=64,
               diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                              denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                             resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4, attention_res=[32],
                                             norm_cfg=dict(type="GN", num_groups=8))),
               decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3],
                            use_dir_enc=True, dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001,
                            max_steps=256),
               decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss"), cache_size=0,
               test_cfg=dict(img_size=(128, 128), density_thresh=0.1, density_step=4))
    m = MODELS.build(cfg)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().eval()
    code = S.make_scene_batch(3, seed=40).cuda()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        grid, bits = m.get_density(m.decoder_ema, code, cfg=m.test_cfg, jitters=[torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(4)])
    scenes = [dict(param=dict(code=code[i], density_grid=grid[i], density_bitfield=bits[i])) for i in range(3)]
    return m, scenes


def _batch(scenes, views, size=128, test_imgs=None):
    from ssdnerf_amd import synthetic as S
    n = len(scenes)
    data = dict(code=scenes, test_poses=S.spiral_poses()[views].cuda()[None].expand(n, -1, -1, -1).contiguous(),
                test_intrinsics=S.cars_intrinsics(size, size).cuda()[None, None].expand(n, len(views), -1).contiguous())
    if test_imgs is not None:
        data["test_imgs"] = test_imgs
    return data


def _targets(pred_chw, seed):
    g = torch.Generator().manual_seed(seed)
    hwc = pred_chw.permute(0, 1, 3, 4, 2).cpu()
    return (hwc + 0.04 * torch.randn(hwc.shape, generator=g)).clamp(0, 1)          # on the host, as a data loader hands it over


def test_val_step_scores_test_views(model_and_scenes):
    m, scenes = model_and_scenes
    plain = m.val_step(_batch(scenes[:2], [10, 90, 170]))
    assert plain["log_vars"] == {} and "test_metrics" not in plain
    target = _targets(plain["pred_imgs"], 1)
    out = m.val_step(_batch(scenes[:2], [10, 90, 170], test_imgs=target))
    assert torch.equal(out["pred_imgs"], plain["pred_imgs"])
    psnr, ssim = out["test_metrics"]["psnr"], out["test_metrics"]["ssim"]
    assert psnr.shape == ssim.shape == (2, 3) and psnr.is_cuda
    assert out["log_vars"]["test_psnr"] == pytest.approx(float(psnr.mean()), rel=1e-6)
    assert out["log_vars"]["test_ssim"] == pytest.approx(float(ssim.mean()), rel=1e-6)
    pred = out["pred_imgs"].permute(0, 1, 3, 4, 2).cpu().numpy()
    for s in range(2):
        for v in range(3):
            assert abs(float(ssim[s, v]) - ssim_ref(pred[s, v], target[s, v].numpy())) <= 2e-6
            assert abs(float(psnr[s, v]) - mse_psnr_ref(pred[s, v], target[s, v].numpy())[1]) <= 1e-4
    m.test_cfg["skip_eval"] = True
    try:
        skipped = m.val_step(_batch(scenes[:2], [10, 90, 170], test_imgs=target))
    finally:
        del m.test_cfg["skip_eval"]
    assert skipped["log_vars"] == {} and "test_metrics" not in skipped and torch.equal(skipped["pred_imgs"], plain["pred_imgs"])


def test_val_step_renders_at_the_ground_truth_size(model_and_scenes):
    m, scenes = model_and_scenes
    target = torch.rand(1, 2, 64, 64, 3, generator=torch.Generator().manual_seed(4))
    out = m.val_step(_batch(scenes[:1], [30, 200], size=64, test_imgs=target))
    assert out["pred_imgs"].shape == (1, 2, 3, 64, 64) and out["test_metrics"]["ssim"].shape == (1, 2)
    assert 0 < out["log_vars"]["test_psnr"] < 60


def test_evaluate_3d_scene_weighted_mean(model_and_scenes):
    from ssdnerf_amd import parallel
    m, scenes = model_and_scenes
    views = [15, 100]
    batches = []
    for sc, seed in [(scenes[:2], 5), (scenes[2:], 6)]:
        pred = m.val_step(_batch(sc, views))["pred_imgs"]
        batches.append(_batch(sc, views, test_imgs=_targets(pred, seed)))
    per = [m.val_step(b)["log_vars"] for b in batches]
    got = parallel.evaluate_3d(m, batches)
    for key in ("test_psnr", "test_ssim"):
        want = (2 * per[0][key] + per[1][key]) / 3
        assert got[key] == pytest.approx(want, rel=1e-6), key
