"""PNG output on the GPU (csrc/png_rows.hip, ssdnerf_amd/viz.py): ``ssdnerf_png_filter_rows`` byte for byte against the independent
numpy restatement (tests/_viz_ref.py) on every path of the kernel, ``ssdnerf_code_plane_rgb`` against the matplotlib fixture
(tests/golden/viridis_map.npz), and the files ``val_step(..., viz_dir=)`` writes, read back with the project's own PNG reader.  Every comparison is byte
or pixel equality.  Every test fails without the feature (the module has no ``viz``, the library no such exports)."""
import os

import numpy as np
import pytest
import torch

import _viz_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX = "srn_tiny/cars"
GUARD = 256                                                              # sentinel bytes on either side of `out`


@pytest.fixture
def in_golden(monkeypatch):
    monkeypatch.chdir(GOLDEN)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "viridis_map.npz"))


def _raw_filter(pred, target):
    """one call of the C ABI on device tensors; `out` sits between two runs of sentinel bytes, which are checked"""
    from ssdnerf_amd import _cabi as C
    n, h, w, _ = pred.shape
    L = 3 * w * (1 if target is None else 2)
    size = n * h * (1 + L)
    padded = torch.full((2 * GUARD + size,), 0xA5, dtype=torch.uint8, device="cuda")
    out = padded[GUARD:GUARD + size]
    C.check(C.lib().ssdnerf_png_filter_rows(C.ptr(pred), int(pred.dtype == torch.uint8), C.ptr(target),
                                            int(target is not None and target.dtype == torch.uint8), n, h, w, C.ptr(out), C.stream()), "png_filter_rows")
    torch.cuda.synchronize()
    host = padded.cpu().numpy()
    assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + size:] == 0xA5), "written outside out"
    return host[GUARD:GUARD + size].reshape(n, h, 1 + L)


def _dev(a):
    return None if a is None else torch.from_numpy(a).cuda()


@pytest.mark.parametrize("kinds", R.KINDS, ids=lambda k: "-".join(k))
def test_filter_rows_equals_restatement_at_the_cpu_suites_shapes(kinds):
    from ssdnerf_amd import viz
    seen = set()
    for h, w, with_target in R.SHAPES:
        pred, target = R.case(h, w, with_target, *kinds)
        want = R.filter_rows_ref(pred, target)
        assert np.array_equal(_raw_filter(_dev(pred), _dev(target)), want), (kinds, h, w, with_target)
        got = viz.filter_rows(_dev(pred), _dev(target))
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
        seen |= set(R.filter_types(want).reshape(-1).tolist())
    assert seen == {0, 1, 2, 3, 4}, seen


def _noisy_pair(n, h, w, seed):
    """a smooth image with noise and a noisy copy of it, as float32 off the k / 255 grid (the rounding and the truncation both matter)"""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (0.5 + 0.45 * np.sin(0.07 * xx + 0.05 * yy)[None, :, :, None] * np.cos(np.arange(3) + np.arange(n)[:, None, None, None])).astype(np.float32)
    pred = (base + g.normal(0, 0.01, base.shape)).astype(np.float32)
    target = np.clip(base + g.normal(0, 0.03, base.shape), -0.1, 1.1).astype(np.float32)
    pred[:, h // 2:] = np.round(np.clip(pred[:, h // 2:], 0, 1) * 255) / np.float32(255)      # the lower half at k / 255, as val_step hands it over
    return pred, target


@pytest.fixture(scope="module")
def pair_128():
    """3 x 128 x 128 with a target, and the restatement's rows for it: computed once (plain Python loops), shared, not modified"""
    pred, target = _noisy_pair(3, 128, 128, 1)
    lines = R.quantise(pred, target)
    return pred, target, lines, R.filter_lines_ref(lines)


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_filter_rows_at_128_by_128_with_target(pair_128, kind):
    """rows of 769 bytes: three passes of a wave, the 16-byte (float32) and 4-byte (uint8) vector loads.  The uint8 operands are the float32 ones'
    own bytes, so both kinds must give the same rows."""
    pred, target, lines, want = pair_128
    if kind == "u8":
        target, pred = (np.ascontiguousarray(half.reshape(3, 128, 128, 3)) for half in (lines[..., :384], lines[..., 384:]))
    assert want.shape == (3, 128, 769) and len(set(R.filter_types(want).reshape(-1).tolist())) >= 3
    assert np.array_equal(_raw_filter(_dev(pred), _dev(target)), want)


@pytest.mark.parametrize("kinds", [("f32", "u8"), ("u8", "f32")], ids=lambda k: "-".join(k))
@pytest.mark.parametrize("with_target", [False, True])
def test_filter_rows_at_width_341(kinds, with_target):
    """rows of 1024 and 2047 bytes: longer than one pass of a wave, 3 w no multiple of 4 (the byte path), a partial last pass"""
    pred, target = _noisy_pair(1, 4, 341, 2)
    if kinds[0] == "u8":
        pred = R.quantise(pred).reshape(pred.shape)
    if kinds[1] == "u8":
        target = R.quantise(target).reshape(target.shape)
    target = target if with_target else None
    want = R.filter_rows_ref(pred, target)
    assert want.shape[-1] == (2047 if with_target else 1024)
    assert np.array_equal(_raw_filter(_dev(pred), _dev(target)), want)


def test_filter_rows_every_tail_and_unaligned_operands():
    """widths 1 .. 12 (every residue of the row length modulo 4 and modulo 3 x 4), and operands that start off a 16-byte boundary with a width that
    would otherwise take the vector path"""
    g = np.random.default_rng(4)
    for w in range(1, 13):
        pred = g.random((2, 3, w, 3), dtype=np.float32)
        target = g.integers(0, 256, (2, 3, w, 3), dtype=np.uint8)
        assert np.array_equal(_raw_filter(_dev(pred), _dev(target)), R.filter_rows_ref(pred, target)), w
    pred, target = g.random((2, 5, 8, 3), dtype=np.float32), g.integers(0, 256, (2, 5, 8, 3), dtype=np.uint8)
    flat_p, flat_t = torch.zeros(pred.size + 1, device="cuda"), torch.zeros(target.size + 1, dtype=torch.uint8, device="cuda")
    flat_p[1:].copy_(torch.from_numpy(pred).reshape(-1))
    flat_t[1:].copy_(torch.from_numpy(target).reshape(-1))
    off_p, off_t = flat_p[1:].view(pred.shape), flat_t[1:].view(target.shape)
    assert off_p.data_ptr() % 16 == 4 and off_t.data_ptr() % 4 == 1
    assert np.array_equal(_raw_filter(off_p, off_t), R.filter_rows_ref(pred, target))


def test_filter_rows_rejects_bad_arguments_host_side():
    import ctypes
    from ssdnerf_amd import _cabi as C
    lib, fake = C.lib(), ctypes.c_void_p(256)
    for args, cause in [((None, 0, None, 0, 1, 2, 2, fake), "null pointer"), ((fake, 0, None, 0, 1, 0, 2, fake), "h >= 1"),
                        ((fake, 0, None, 0, 1, 2, 0, fake), "h >= 1"), ((fake, 0, None, 0, 1, 2, (1 << 28) + 1, fake), "2^28")]:
        assert lib.ssdnerf_png_filter_rows(*args, None) == -1
        msg = lib.ssdnerf_last_error().decode()
        assert msg.startswith("png_filter_rows") and cause in msg, msg
    assert lib.ssdnerf_png_filter_rows(fake, 0, None, 0, 0, 2, 2, fake, None) == 0           # n == 0: a no-op


# ---------------------------------------------------------------------------------------------- code planes
@pytest.mark.parametrize("key,code_range", [("m1_1", (-1, 1)), ("m2_2", (-2, 2))])
def test_code_plane_rgb_reproduces_matplotlib(fixture, key, code_range):
    from ssdnerf_amd import viz
    x, want = fixture["x_" + key], fixture["rgb_" + key]
    xs = np.concatenate([x, np.zeros((-x.size) % 3, np.float32)])
    code = torch.from_numpy(xs.reshape(1, 3, 1, 1, -1).copy()).cuda()
    got = viz.code_plane_rgb(code, code_range, flip_z=True)
    assert got.is_cuda and np.array_equal(got.cpu().numpy().reshape(-1, 3)[:x.size], want)


@pytest.mark.parametrize("flip_z", [False, True])
@pytest.mark.parametrize("shape", [(2, 3, 6, 16, 16), (1, 3, 1, 1, 1), (2, 3, 2, 3, 5)])
def test_code_plane_rgb_equals_restatement(fixture, shape, flip_z):
    from ssdnerf_amd import viz
    code = np.random.default_rng(6).uniform(-1.3, 1.3, shape).astype(np.float32)
    if code.size > 7:
        code.reshape(-1)[::7] = np.nan
    want = R.colour_map_ref(R.plane_sheet_ref(code, flip_z), fixture["table"], -1, 1)
    got = viz.code_plane_rgb(torch.from_numpy(code).cuda(), (-1, 1), flip_z=flip_z).cpu().numpy()
    assert got.shape == (shape[0], 3 * shape[3], shape[2] * shape[4], 3) and np.array_equal(got, want)
    rows = viz.filter_rows(torch.from_numpy(want).cuda()).cpu().numpy()     # ... and on through the row filter as a uint8 pred without a target
    assert np.array_equal(rows, R.filter_rows_ref(want))


# ---------------------------------------------------------------------------------------------- val_step
DEC = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
           dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)
VIEWS = [10, 90, 170]


@pytest.fixture(scope="module")
def models_and_scenes():
    """the smallest DiffusionNeRF the GPU suite builds (tests/test_metrics_gpu.py), a MultiSceneNeRF on the same decoder, and two scenes"""
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    common = dict(code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64, decoder=DEC, decoder_use_ema=True, bg_color=1,
                  pixel_loss=dict(type="MSELoss"), cache_size=0)
    diff = MODELS.build(dict(type="DiffusionNeRF", code_reshape=(18, 128, 128),
                             diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                                            denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                                           resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4,
                                                           attention_res=[32], norm_cfg=dict(type="GN", num_groups=8))),
                             test_cfg=dict(img_size=(16, 16), density_thresh=0.1, density_step=4, clip_range=[-2, 2]), **common))
    base = MODELS.build(dict(type="MultiSceneNeRF", test_cfg=dict(img_size=(16, 16), density_thresh=0.1), **common))
    for m in (diff, base):
        m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
        m.cuda().eval()
    code = S.make_scene_batch(2, seed=40).cuda()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        grid, bits = diff.get_density(diff.decoder_ema, code, cfg=diff.test_cfg, jitters=[torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(4)])
    scenes = [dict(param=dict(code=code[i], density_grid=grid[i], density_bitfield=bits[i])) for i in range(2)]
    return dict(diffusion=diff, base=base), scenes


def _batch(scenes, test_imgs=None, size=16):
    from ssdnerf_amd import synthetic as S
    n = len(scenes)
    data = dict(code=scenes, scene_name=["car_a", "car_b"][:n], test_poses=S.spiral_poses()[VIEWS].cuda()[None].expand(n, -1, -1, -1).contiguous(),
                test_intrinsics=S.cars_intrinsics(size, size).cuda()[None, None].expand(n, len(VIEWS), -1).contiguous())
    if test_imgs is not None:
        data.update(test_imgs=test_imgs, test_img_paths=[["rgb/{:06d}.png".format(v) for v in VIEWS] for _ in range(n)])
    return data


def _read(path):
    from ssdnerf_amd.datasets import decode_png
    with open(path, "rb") as f:
        return decode_png(f.read(), path)


def _bytes_of(folder):
    out = {}
    for name in sorted(os.listdir(folder)):
        with open(os.path.join(folder, name), "rb") as f:
            out[name] = f.read()
    return out


@pytest.mark.parametrize("which", ["diffusion", "base"])
def test_val_step_writes_what_it_returns(models_and_scenes, fixture, tmp_path, which):
    models, scenes = models_and_scenes
    m = models[which]
    code_range = m.test_cfg.get("clip_range", [-1, 1])
    # without ground truth: the numbered names, the prediction alone
    plain_dir = str(tmp_path / "plain")
    plain = m.val_step(_batch(scenes), viz_dir=plain_dir)
    pred = torch.round(plain["pred_imgs"].permute(0, 1, 3, 4, 2) * 255).to(torch.uint8).cpu().numpy()
    assert pred.shape == (2, 3, 16, 16, 3) and pred.min() < 128 < pred.max()
    views = ["scene_{}_{:03d}.png".format(n, v) for n in ("car_a", "car_b") for v in range(3)]
    planes = ["scene_car_a.png", "scene_car_b.png"]
    assert sorted(os.listdir(plain_dir)) == sorted(views + planes)
    for i, name in enumerate(views):
        assert np.array_equal(_read(os.path.join(plain_dir, name)), pred[i // 3, i % 3]), name
    for i, name in enumerate(planes):
        want = R.colour_map_ref(R.plane_sheet_ref(plain["code"][i:i + 1].cpu().numpy(), False), fixture["table"], *code_range)[0]
        img = _read(os.path.join(plain_dir, name))
        assert img.shape == (3 * 128, 6 * 128, 3) and np.array_equal(img, want), name
    # scored: [truncated ground truth | prediction], named after the returned per-view scores
    g = torch.Generator().manual_seed(1)
    hwc = plain["pred_imgs"].permute(0, 1, 3, 4, 2).cpu()
    target = (hwc + 0.04 * torch.randn(hwc.shape, generator=g)).clamp(0, 1)
    scored_dir = str(tmp_path / "scored")
    out = m.val_step(_batch(scenes, test_imgs=target), viz_dir=scored_dir)
    assert torch.equal(out["pred_imgs"], plain["pred_imgs"])
    psnr, ssim = out["test_metrics"]["psnr"].cpu(), out["test_metrics"]["ssim"].cpu()
    names = ["scene_{}_{:06d}_psnr{:02.1f}_ssim{:.2f}_lpips{:.3f}.png".format(n, VIEWS[v], psnr[s, v], ssim[s, v], float("nan"))
             for s, n in enumerate(("car_a", "car_b")) for v in range(3)]
    assert sorted(os.listdir(scored_dir)) == sorted(names + planes)
    truth = (target * 255).to(torch.uint8).numpy()
    for i, name in enumerate(names):
        img = _read(os.path.join(scored_dir, name))
        assert img.shape == (16, 32, 3) and np.array_equal(img[:, :16], truth[i // 3, i % 3]) and np.array_equal(img[:, 16:], pred[i // 3, i % 3]), name
    # two calls write byte-identical files
    again_dir = str(tmp_path / "again")
    m.val_step(_batch(scenes, test_imgs=target), viz_dir=again_dir)
    assert _bytes_of(again_dir) == _bytes_of(scored_dir)
    with pytest.raises(KeyError, match="scene_name"):
        m.val_step({k: v for k, v in _batch(scenes).items() if k != "scene_name"}, viz_dir=str(tmp_path / "no"))


def test_val_step_on_a_stored_views_batch_writes_the_same_bytes(in_golden, tmp_path):
    """the fitted reconstruction of a loader batch whose ``cond_imgs`` stay in the uint8 store (``StoredViews``) against the dense batch: the same
    files, byte for byte (the fit draws the same rays from the same seed, tests/test_ray_sample_gpu.py)"""
    import test_tv_loss_gpu as TV
    from ssdnerf_amd import datasets as D
    from ssdnerf_amd.config import build_dataloader
    test_cfg = dict(density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 8, loss_coef=0.1 / (8 * 8), n_inverse_steps=2,
                    optimizer=dict(type="Adam", lr=0.08, weight_decay=0.), lr_scheduler=dict(type="ExponentialLR", gamma=0.998))
    ds = D.ShapeNetSRN(PREFIX, step=2, num_test_imgs=2)                      # alpha_01 and zeta_03: 4 conditioning + 2 test views of 8 x 8
    dense, stored = next(iter(build_dataloader(ds, 2))), next(iter(build_dataloader(ds, 2, cond_imgs="stored")))
    assert isinstance(stored["cond_imgs"], D.StoredViews) and torch.equal(dense["test_imgs"], stored["test_imgs"])
    m = TV._stage1_model(test_cfg=test_cfg).eval()
    written = []
    for name, batch in (("dense", dense), ("stored", stored)):
        torch.manual_seed(2)
        out = m.val_step(batch, viz_dir=str(tmp_path / name))
        written.append(_bytes_of(str(tmp_path / name)))
        assert len(written[-1]) == 2 * 2 + 2 + 1                            # the views, the scenes' planes, the mean code's
    assert "scene_000_mean.png" in written[0] and list(written[0]) == list(written[1])
    assert written[0] == written[1]
    truth = (dense["test_imgs"] * 255).to(torch.uint8).cpu().numpy()
    pred = torch.round(out["pred_imgs"].permute(0, 1, 3, 4, 2) * 255).to(torch.uint8).cpu().numpy()
    psnr, ssim = out["test_metrics"]["psnr"].cpu(), out["test_metrics"]["ssim"].cpu()
    for s, scene in enumerate(stored["scene_name"]):
        for v, path in enumerate(stored["test_img_paths"][s]):
            name = "scene_{}_{}_psnr{:02.1f}_ssim{:.2f}_lpips{:.3f}.png".format(scene, os.path.splitext(os.path.basename(path))[0], psnr[s, v],
                                                                                ssim[s, v], float("nan"))
            assert name in written[1], (name, list(written[1]))
            img = _read(os.path.join(str(tmp_path / "stored"), name))
            assert np.array_equal(img[:, :8], truth[s, v]) and np.array_equal(img[:, 8:], pred[s, v]), name
