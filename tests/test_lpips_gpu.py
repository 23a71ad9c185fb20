"""LPIPS on the MI355X.  Every kernel of csrc/lpips.hip, and the existing fp32-class convolution on the thirteen VGG16 shapes, against float64
computed from the exact values the kernel read (the style of tests/test_unet_kernels_fp64_gpu.py); ``LPIPSVGG`` end to end against the float64
restatement (tests/_lpips_ref.py) within the accuracy of the reference's own default arithmetic; and the scores val_step / evaluate_3d report.

End-to-end figures measured on the MI355X (seeded weights, the five pair kinds of ``make_pairs``; worst relative error over the pairs against the
tolerance, the TF32 emulation's own worst error): see profiles/lpips.json."""
import pytest
import torch
import torch.nn.functional as F

from _fp64_bounds import check_le, conv_ref, f32x2_bound
from _lpips_ref import (SCALE, SHIFT, check_lpips_layer, lpips_ref, make_pairs, make_tap_input, rel_err)

pytestmark = pytest.mark.gpu


def _cl(x):
    return x.cuda().contiguous(memory_format=torch.channels_last)


def _bits(x):
    return x.contiguous(memory_format=torch.channels_last).view(torch.int32) if x.dim() == 4 else x.view(torch.int32)


@pytest.fixture(scope="module")
def sd():
    from ssdnerf_amd import synthetic as S
    return S.make_lpips_params(1)


@pytest.fixture(scope="module")
def net(sd):
    from ssdnerf_amd.lpips import LPIPSVGG
    return LPIPSVGG.from_state_dict(sd)


# ---------------------------------------------------------------------------------------------- the input kernel
@pytest.mark.parametrize("n,h,w", [(3, 16, 16), (2, 50, 70), (1, 128, 128)])
def test_lpips_input_within_two_ulps(n, h, w):
    from ssdnerf_amd.lpips import lpips_input
    g = torch.Generator().manual_seed(h + w)
    pred = torch.round(torch.rand(n, h, w, 3, generator=g) * 255) / 255
    target = torch.rand(n, h, w, 3, generator=g)
    target[0, 0, :4] = torch.tensor([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.485, 0.456, 0.406], [0.25, 0.5, 0.75]])
    out = lpips_input(pred.cuda(), target.cuda())
    torch.cuda.synchronize()
    assert out.shape == (2 * n, 8, h, w) and out.is_contiguous(memory_format=torch.channels_last)
    got = out.permute(0, 2, 3, 1).cpu()                                    # (2n, h, w, 8)
    assert not bool(got[..., 3:].any()) and not bool(torch.signbit(got[..., 3:]).any())
    # the constants are the fp32 values the kernel holds; everything else in float64
    shift, scale = torch.tensor(SHIFT, dtype=torch.float32).double(), torch.tensor(SCALE, dtype=torch.float32).double()
    ref = ((2 * torch.cat([pred, target]).double() - 1) - shift) / scale
    _, e = torch.frexp(ref)
    ulp = torch.ldexp(torch.ones_like(ref), e - 24)
    err = (got[..., :3].double() - ref).abs() / ulp
    print(f"lpips_input {n} x {h} x {w}: worst error {float(err.max()):.3f} ulp")
    assert float(err.max()) <= 2.0


# ---------------------------------------------------------------------------------------------- ReLU + pool
@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("H,W", [(16, 16), (17, 23), (9, 14), (2, 3)])
def test_relu_pool_is_exact_and_its_split_form_matches_split_f32(C, H, W):
    from ssdnerf_amd.lpips import relu_pool_nhwc
    from ssdnerf_amd.unet_fast import split_f32_nhwc
    g = torch.Generator().manual_seed(C + H)
    x = _cl(torch.randn(3, C, H, W, generator=g))
    for pool in (False, True):
        want = F.max_pool2d(F.relu(x), 2, 2) if pool else F.relu(x)
        plain = relu_pool_nhwc(x, pool=pool)
        split = relu_pool_nhwc(x, pool=pool, split_out=True)
        torch.cuda.synchronize()
        assert plain.shape == want.shape and plain.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(_bits(plain), _bits(want)), (pool, float((plain - want).abs().max()))
        assert torch.equal(_bits(split), _bits(split_f32_nhwc(plain))), pool


def test_relu_pool_keeps_nan_and_clears_negative_zero():
    """as ``torch.relu`` and ``max_pool2d`` do: a NaN must not turn into a plausible number"""
    from ssdnerf_amd.lpips import relu_pool_nhwc
    x = torch.randn(2, 64, 6, 7, generator=torch.Generator().manual_seed(0))
    x[0, 3, 2, 2] = float("nan")                                            # first of its 2 x 2 window
    x[1, 9, 3, 5] = float("nan")                                            # last of its window
    x[0, 5, 0, 0] = -0.0
    x[0, 5, 0, 1], x[0, 5, 1, 0], x[0, 5, 1, 1] = -1.0, -0.0, -2.0
    x = _cl(x)
    for pool in (False, True):
        got, want = relu_pool_nhwc(x, pool=pool).cpu(), (F.max_pool2d(F.relu(x.cpu()), 2, 2) if pool else F.relu(x.cpu()))
        assert torch.equal(got.isnan(), want.isnan()) and int(got.isnan().sum()) == 2, pool
        assert torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0)), pool
        assert not bool(torch.signbit(got.nan_to_num(7.0)).any()), pool


# ---------------------------------------------------------------------------------------------- the convolutions, on new ground
def _vgg_layers(h, w):
    from ssdnerf_amd.lpips import CHANNELS, FEATURE_IDX, TAPS
    H, W = h, w
    for i, (idx, (cin, cout)) in enumerate(zip(FEATURE_IDX, CHANNELS)):
        yield i, idx, cin, cout, H, W
        if i in TAPS[:-1]:
            H, W = H // 2, W // 2


@pytest.mark.parametrize("h,w,B", [(128, 128, 2), (50, 70, 2), (37, 19, 6)])
def test_convolution_with_bias_on_the_thirteen_vgg_shapes(sd, h, w, B):
    """conv + bias of every trunk layer (Cin padded 3 -> 8 on the first; the 8 x 8 level is cut along K) within ``f32x2_bound``, on the on-the-fly split
    and, where the layer takes it, on PRE-SPLIT input"""
    from ssdnerf_amd import unet_fast as UF
    g = torch.Generator().manual_seed(h)
    ws = UF.shared_splitk_ws("cuda")
    seen = set()
    for i, idx, cin, cout, H, W in _vgg_layers(h, w):
        wt, bias = sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"].cuda()
        if i == 0:
            wt, cin = torch.cat([wt, wt.new_zeros(cout, 5, 3, 3)], 1), 8
            x = torch.cat([torch.randn(B, 3, H, W, generator=g) * 2, torch.zeros(B, 5, H, W)], 1)
        else:                                                                  # what a ReLU (and a pool) leaves: non-negative, many zeros
            x = F.relu(torch.randn(B, cin, H, W, generator=g))
        x = _cl(x)
        hi, lo = UF.split_bf16x2_adjacent(wt.cuda())
        ref, A = conv_ref(x.cpu(), hi.float().cpu().double() + lo.float().cpu().double(), bias.cpu())
        bound = f32x2_bound(A, 9 * cin)
        plan = int(UF.C.lib().ssdnerf_conv2d_nhwc_f32x2_plan(UF.C.u32(B * H * W), UF.C.u32(cin), UF.C.u32(cout), UF.C.u32(3), 0, 0))
        y = UF.conv2d_nhwc_f32x2(x, hi, lo, bias=bias, splitk_ws=ws)
        torch.cuda.synchronize()
        bad, worst = check_le(y.cpu(), ref, bound)
        kind = UF.presplit_supported(x, cout, 3) if cin % 32 == 0 else 0
        print(f"conv {i + 1:2d} {cin:3d} -> {cout:3d} @ {H} x {W}: splits {plan >> 8}, worst error / bound {worst:.3f}, pre-split kind {kind}")
        assert bad == 0, (i, worst)
        seen.add(("splits", (plan >> 8) > 1))
        if kind:
            yp = UF.conv2d_nhwc_f32x2_presplit(UF.split_f32_nhwc(x), hi, lo, bias, splitk_ws=ws)
            torch.cuda.synchronize()
            bad, worst = check_le(yp.cpu(), ref, bound)
            print(f"        pre-split: worst error / bound {worst:.3f}")
            assert bad == 0, (i, "presplit", worst)
        assert not bool(ws.any()), "the split-K scratch must be left all zero"
    if (h, w) == (128, 128):
        assert ("splits", True) in seen, "the 8 x 8 level was expected to be cut along K"


# ---------------------------------------------------------------------------------------------- the tap kernel
@pytest.mark.parametrize("C", [64, 128, 256, 512])
@pytest.mark.parametrize("n,H,W", [(3, 16, 16), (2, 17, 23), (5, 5, 4), (1, 64, 64)])
def test_lpips_layer_within_its_bound(C, n, H, W):
    from ssdnerf_amd.lpips import lpips_layer, relu_pool_nhwc
    x = _cl(make_tap_input(n, C, H, W, seed=C + H + n))
    assert bool((F.relu(x).sum(1) == 0).any())
    lin = (torch.rand(C, generator=torch.Generator().manual_seed(C)) * 2 / C).cuda()
    acc = torch.zeros(n, device="cuda")
    pooled = lpips_layer(x, lin, acc)
    torch.cuda.synchronize()
    bad, worst = check_lpips_layer(acc, x.cpu(), lin.cpu(), n)
    print(f"lpips_layer C = {C}, {n} pairs of {H} x {W}: worst error / bound {worst:.3f}")
    assert bad == 0, worst
    # the fused pooled output is relu_pool's, plain and pre-split
    assert torch.equal(_bits(pooled), _bits(relu_pool_nhwc(x, pool=True)))
    acc_s = torch.zeros(n, device="cuda")
    pooled_s = lpips_layer(x, lin, acc_s, split_out=True)
    assert torch.equal(_bits(pooled_s), _bits(relu_pool_nhwc(x, pool=True, split_out=True))) and torch.equal(acc_s, acc)
    # it ADDS to acc; without a pooled output (the last tap) the value is the same bits
    start = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 0.05).cuda()
    acc2 = start.clone()
    assert lpips_layer(x, lin, acc2, pool_out=False) is None
    torch.cuda.synchronize()
    bad, worst = check_lpips_layer(acc2, x.cpu(), lin.cpu(), n, acc_in=start.cpu())
    assert bad == 0, worst
    assert torch.equal(acc2, start + acc)
    # two calls: the same bits
    again = torch.zeros(n, device="cuda")
    pooled_again = lpips_layer(x, lin, again)
    assert torch.equal(again, acc) and torch.equal(_bits(pooled_again), _bits(pooled))


def test_lpips_layer_signed_weights_and_identical_images():
    from ssdnerf_amd.lpips import lpips_layer
    n, C, H, W = 2, 128, 11, 13
    x = make_tap_input(n, C, H, W, seed=9)
    x[n:] = x[:n]
    x = _cl(x)
    lin = torch.randn(C, generator=torch.Generator().manual_seed(1)).cuda()
    acc = torch.zeros(n, device="cuda")
    lpips_layer(x, lin, acc, pool_out=False)
    assert acc.tolist() == [0.0, 0.0]                                      # identical features: every difference is exactly zero
    y = _cl(make_tap_input(n, C, H, W, seed=10))
    lpips_layer(y, lin, acc, pool_out=False)
    torch.cuda.synchronize()
    assert check_lpips_layer(acc, y.cpu(), lin.cpu(), n)[0] == 0


def test_lpips_layer_gives_nan_for_the_pair_that_holds_one():
    from ssdnerf_amd.lpips import lpips_layer, relu_pool_nhwc
    n, C, H, W = 3, 128, 9, 10
    clean = make_tap_input(n, C, H, W, seed=4)
    x = clean.clone()
    x[n + 1, 17, 8, 3] = float("nan")                                       # the target of pair 1, in the odd last row (no pooled pixel reads it)
    x[2, 40, 2, 5] = float("nan")                                           # the prediction of pair 2
    lin = (torch.rand(C, generator=torch.Generator().manual_seed(C)) * 2 / C).cuda()
    acc, ref = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    pooled = lpips_layer(_cl(x), lin, acc)
    lpips_layer(_cl(clean), lin, ref)
    torch.cuda.synchronize()
    assert acc.isnan().tolist() == [False, True, True] and float(acc[0]) == float(ref[0]) > 0
    assert torch.equal(pooled.isnan(), relu_pool_nhwc(_cl(x), pool=True).isnan()) and int(pooled.isnan().sum()) == 1 and bool(pooled[2, 40, 1, 2].isnan())


# ---------------------------------------------------------------------------------------------- end to end
def _tolerance(a, b, sd):
    """(float64 restatement, the worst relative error of its TF32 emulation over the pairs): the accuracy of the reference's own default arithmetic"""
    exact = lpips_ref(a, b, sd)
    return exact, float(rel_err(lpips_ref(a, b, sd, mode="tf32"), exact).max())


@pytest.mark.parametrize("h,w", [(64, 64), (50, 70), (128, 128)])
def test_lpips_end_to_end_within_the_tf32_tolerance(sd, net, h, w):
    a, b = make_pairs(h, w)
    exact, tol = _tolerance(a, b, sd)
    got = {chunk: net(a.cuda(), b.cuda(), chunk=chunk) for chunk in (32, 3, 1)}
    torch.cuda.synchronize()
    assert got[32].shape == (5,) and got[32].dtype == torch.float32
    for chunk, value in got.items():
        err = rel_err(value, exact)
        print(f"LPIPSVGG {h} x {w}, chunk {chunk}: relative error {[f'{e:.2e}' for e in err.tolist()]}, worst {float(err.max()):.2e}; TF32 tolerance {tol:.2e}; "
              f"values {[f'{v:.3e}' for v in exact.tolist()]}")
        assert float(err.max()) <= tol, (chunk, err.tolist(), tol)
    # (two whole calls need not return the same bits: the convolutions that are cut along K add their partial sums with fp32 atomics, as in the UNet;
    #  the passes of csrc/lpips.hip are bit-reproducible, test_lpips_layer_within_its_bound)
    assert float(rel_err(net(a.cuda(), b.cuda()), exact).max()) <= tol
    # leading shapes, and a pair of identical images
    same = net(torch.stack([a, a]).cuda(), torch.stack([a, a]).cuda())
    assert same.shape == (2, 5) and float(same.min()) >= 0 and float(same.max()) <= 1e-9, same.tolist()
    mixed = net(torch.cat([a[:2], a[2:3]]).cuda(), torch.cat([b[:2], a[2:3]]).cuda())
    assert 0 <= float(mixed[2]) <= 1e-9 and float(rel_err(mixed[:2], exact[:2]).max()) <= tol


def test_lpips_of_an_image_with_a_nan_is_nan(net):
    """a NaN pixel in a rendered or ground-truth image shows in the score of that pair, as it does in PSNR and SSIM, and in no other pair's"""
    g = torch.Generator().manual_seed(8)
    a, b = torch.rand(4, 32, 40, 3, generator=g), torch.rand(4, 32, 40, 3, generator=g)
    a[1, 20, 31, 2] = float("nan")
    b[3, 0, 0, 0] = float("nan")
    for chunk in (32, 1):
        got = net(a.cuda(), b.cuda(), chunk=chunk).cpu()
        assert got.isnan().tolist() == [False, True, False, True], (chunk, got.tolist())
        assert float(got[0]) > 0 and float(got[2]) > 0
    net.release_buffers()
    assert not net._bufs
    assert float(net(a[:1].cuda(), b[:1].cuda())) > 0 and net._bufs         # the next call allocates them again


def test_lpips_checks_its_inputs(net):
    from ssdnerf_amd.metrics import image_lpips
    a = torch.rand(2, 32, 32, 3, device="cuda")
    assert image_lpips(a, a.flip(0), net).shape == (2,)
    assert net(a[:0], a[:0]).shape == (0,)
    with pytest.raises(ValueError):
        net(a, a[:1])
    with pytest.raises(ValueError):
        net(a[..., :2], a[..., :2])
    with pytest.raises(TypeError):
        net(a.double(), a.double())
    with pytest.raises(ValueError):
        net(a.cpu(), a.cpu())
    with pytest.raises(ValueError):
        net(a[:, :15], a[:, :15])
    assert net.max_chunk(128, 128) >= 32 and net.max_chunk(1024, 1024) == 3


# ---------------------------------------------------------------------------------------------- val_step / evaluate_3d
DEC = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
           dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)


@pytest.fixture(scope="module")
def diffusion_model_and_scenes():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    cfg = dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
               diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                              denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                             resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4, attention_res=[32],
                                             norm_cfg=dict(type="GN", num_groups=8))),
               decoder=DEC, decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss"), cache_size=0,
               test_cfg=dict(img_size=(64, 64), density_thresh=0.1, density_step=4))
    m = MODELS.build(cfg)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().eval()
    code = S.make_scene_batch(3, seed=40).cuda()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        grid, bits = m.get_density(m.decoder_ema, code, cfg=m.test_cfg, jitters=[torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(4)])
    return m, [dict(param=dict(code=code[i], density_grid=grid[i], density_bitfield=bits[i])) for i in range(3)]


def _batch(scenes, views, size=64, test_imgs=None):
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
    return (hwc + 0.04 * torch.randn(hwc.shape, generator=g)).clamp(0, 1)


def _check_scores(out, target, sd):
    """``test_lpips`` is the mean of ``test_metrics['lpips']``, which matches the restatement on pred_imgs against test_imgs within the TF32 tolerance"""
    lp = out["test_metrics"]["lpips"]
    S_, V = target.shape[:2]
    assert lp.shape == (S_, V) and lp.is_cuda and lp.dtype == torch.float32
    assert out["log_vars"]["test_lpips"] == pytest.approx(float(lp.mean()), rel=1e-6)
    pred = out["pred_imgs"].permute(0, 1, 3, 4, 2).cpu().flatten(0, 1)
    exact, tol = _tolerance(pred, target.float().flatten(0, 1), sd)
    err = rel_err(lp.flatten(), exact)
    print(f"val_step lpips {lp.flatten().tolist()}: worst relative error {float(err.max()):.2e}, TF32 tolerance {tol:.2e}")
    assert float(err.max()) <= tol


def test_diffusion_val_step_reports_lpips(diffusion_model_and_scenes, sd, net):
    m, scenes = diffusion_model_and_scenes
    views = [10, 90, 170]
    plain = m.val_step(_batch(scenes[:2], views))
    target = _targets(plain["pred_imgs"], 1)
    without = m.val_step(_batch(scenes[:2], views, test_imgs=target))
    assert set(without["log_vars"]) == {"test_psnr", "test_ssim"} and set(without["test_metrics"]) == {"psnr", "ssim"}
    m.set_lpips(net)
    try:
        out = m.val_step(_batch(scenes[:2], views, test_imgs=target))
        assert set(out["log_vars"]) == {"test_psnr", "test_ssim", "test_lpips"} and set(out["test_metrics"]) == {"psnr", "ssim", "lpips"}
        assert set(out) == set(without) and torch.equal(out["pred_imgs"], without["pred_imgs"])
        assert out["log_vars"]["test_psnr"] == without["log_vars"]["test_psnr"] and torch.equal(out["test_metrics"]["ssim"], without["test_metrics"]["ssim"])
        _check_scores(out, target, sd)
        assert "lpips" not in " ".join(m.state_dict())
        m.use_lpips_metric = False
        off = m.val_step(_batch(scenes[:2], views, test_imgs=target))
        assert set(off["log_vars"]) == {"test_psnr", "test_ssim"} and set(off["test_metrics"]) == {"psnr", "ssim"}
        m.use_lpips_metric = True
        assert "test_lpips" not in m.val_step(_batch(scenes[:2], views))["log_vars"]          # no ground truth: nothing to score
    finally:
        m.set_lpips(None)
        m.use_lpips_metric = True


def test_evaluate_3d_returns_the_scene_weighted_lpips(diffusion_model_and_scenes, net):
    from ssdnerf_amd import parallel
    m, scenes = diffusion_model_and_scenes
    views = [15, 100]
    batches = []
    for sc, seed in [(scenes[:2], 5), (scenes[2:], 6)]:
        batches.append(_batch(sc, views, test_imgs=_targets(m.val_step(_batch(sc, views))["pred_imgs"], seed)))
    assert "test_lpips" not in parallel.evaluate_3d(m, batches)
    m.set_lpips(net)
    try:
        per = [m.val_step(b)["log_vars"] for b in batches]
        got = parallel.evaluate_3d(m, batches)
    finally:
        m.set_lpips(None)
    for key in ("test_psnr", "test_ssim", "test_lpips"):
        assert got[key] == pytest.approx((2 * per[0][key] + per[1][key]) / 3, rel=1e-6), key
    assert got["test_lpips"] > 0


def test_stage1_val_step_reports_lpips_from_a_weights_file(sd, tmp_path):
    """a stage-1 MultiSceneNeRF fits its codes to the conditioning views, then scores the test views; the net comes from test_cfg['lpips_weights']"""
    from ssdnerf_amd import nerf, synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.density import get_density
    from ssdnerf_amd.registry import MODELS
    torch.save(sd, tmp_path / "vgg_lpips.pth")
    test_cfg = dict(img_size=(64, 64), density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 12, loss_coef=0.1 / (64 * 64), n_inverse_steps=4,
                    optimizer=dict(type="Adam", lr=0.08, weight_decay=0.), lr_scheduler=dict(type="ExponentialLR", gamma=0.998))
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64, decoder=DEC,
                          decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=0, init_from_mean=True, test_cfg=test_cfg))
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    with torch.no_grad():
        m.init_code.copy_(S.make_triplane(80))
    m = m.cuda().eval()

    dec = TriPlaneDecoder(**{k: v for k, v in DEC.items() if k != "type"})
    dec.load_state_dict(S.make_decoder_params(), strict=False)
    dec = dec.cuda().eval()
    codes = torch.stack([S.make_triplane(s) for s in (71, 72)]).cuda()

    def views(ids):
        with torch.no_grad():
            _, bits = get_density(dec, codes, 64, density_thresh=0.1, density_step=4)
            poses = S.spiral_poses()[ids].cuda()[None].expand(2, -1, -1, -1).contiguous()
            intr = S.cars_intrinsics(64, 64).cuda()[None, None].expand(2, len(ids), -1).contiguous()
            image, _ = nerf.render(dec, codes, bits, 64, 64, intr, poses)
        return image.clamp(0, 1), poses, intr

    imgs, poses, intr = views([0, 60, 120, 200])
    timgs, tposes, tintr = views([20, 100, 180])
    data = dict(scene_name=["a", "b"], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr, test_poses=tposes, test_intrinsics=tintr, test_imgs=timgs.cpu())

    def run():
        g = torch.Generator().manual_seed(4)
        torch.manual_seed(3)
        return m.val_step(data, march_noises=[torch.rand(2, 2 ** 12, generator=g).cuda() for _ in range(4)],
                          density_jitters=[torch.rand(64 ** 3, 3, generator=g).cuda()])

    without = run()
    assert set(without["log_vars"]) == {"test_psnr", "test_ssim", "train_psnr", "code_rms"} and set(without["test_metrics"]) == {"psnr", "ssim"}
    m.test_cfg["lpips_weights"] = str(tmp_path / "vgg_lpips.pth")
    out = run()
    assert set(out["log_vars"]) == {"test_psnr", "test_ssim", "test_lpips", "train_psnr", "code_rms"}
    assert len(m.lpips) == 1 and out["pred_imgs"].shape == without["pred_imgs"].shape
    _check_scores(out, timgs.cpu(), sd)
    assert not any("lpips" in k for k in m.state_dict())
