"""FID / KID on the MI355X: the two kernels of csrc/feature_stats.hip (fp64 MFMA) bit for bit against numpy on inputs where every summation order gives the
same bits, within worst-case first-order bounds on random features (tests/_fidkid_ref.py; tests/test_fidkid_cpu.py shows what those bounds reject), bit-identical
from call to call, and the scores ``parallel.evaluate_3d(..., metrics=[FIDKID])`` reports for views rendered by ``DiffusionNeRF.val_step``."""
import functools

import numpy as np
import pytest
import torch

import _fidkid_ref as R
from ssdnerf_amd import fidkid as FK

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16), (3, 16), (5, 20), (67, 48), (130, 200), (2008, 2048)]        # (n, D): n not a multiple of 4, D not a multiple of the 64 x 64 tile, the workload


@functools.lru_cache(maxsize=None)
def _moment_case(kind, n, D):
    """features and their float64 moments, computed once per shape"""
    x = R.exact_features(n, D, seed=n + D) if kind == "exact" else R.random_features(n, D, seed=n + D)
    s, outer = R.moments_ref(x)
    return x, s, outer


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _gpu_moments(x, splits=None):
    fm = FK.FeatureMoments(x.shape[1], "cuda")
    t = torch.from_numpy(x).cuda()
    for part in (t.split(splits) if splits else [t]):
        fm.update(part)
    torch.cuda.synchronize()
    return fm


# ---------------------------------------------------------------------------------------------- moments
@pytest.mark.parametrize("n,D", SHAPES)
def test_moments_are_exact_where_every_order_is(n, D):
    x, s, outer = _moment_case("exact", n, D)
    fm = _gpu_moments(x)
    assert fm.count == n
    got = fm.outer.cpu().numpy()
    assert np.array_equal(_bits(fm.sum.cpu().numpy()), _bits(s))
    assert np.array_equal(_bits(got), _bits(outer)), float(np.abs(got - outer).max())
    assert np.array_equal(got, got.T)
    # only the 64 x 64 tiles on and above the diagonal are written
    raw = fm._outer.cpu().numpy()
    tile_i, tile_j = np.arange(D)[:, None] // 64, np.arange(D)[None, :] // 64
    assert not raw[tile_j < tile_i].any() and np.array_equal(raw[tile_j >= tile_i], outer[tile_j >= tile_i])


def test_moments_of_successive_updates_equal_one_update():
    x = R.exact_features(73, 48, seed=7)
    one, three = _gpu_moments(x), _gpu_moments(x, splits=[5, 67, 1])
    s, outer = R.moments_ref(x)
    assert three.count == one.count == 73
    assert torch.equal(three.sum, one.sum) and torch.equal(three._outer, one._outer)
    assert np.array_equal(_bits(three.outer.cpu().numpy()), _bits(outer)) and np.array_equal(_bits(three.sum.cpu().numpy()), _bits(s))
    three.update(torch.empty(0, 48, device="cuda"))                               # n == 0: nothing happens
    assert three.count == 73 and torch.equal(three._outer, one._outer)


@pytest.mark.parametrize("n,D", [(67, 48), (130, 200), (2008, 2048)])
def test_moments_within_their_bounds(n, D):
    x, s, outer = _moment_case("random", n, D)
    absx = R.abs_outer(x)
    fm = _gpu_moments(x)
    bad, worst = R.check_le(fm.outer.cpu().numpy(), outer, R.outer_bound(x, absx))
    print(f"moments ({n}, {D}): worst |outer - ref| / bound {worst:.3f}")
    assert bad == 0, worst
    bad, worst = R.check_le(fm.sum.cpu().numpy(), s, 2 * n * R.U * np.abs(x.astype(np.float64)).sum(0))
    assert bad == 0, worst
    bad, worst = R.check_le(fm.cov.cpu().numpy(), np.cov(x.astype(np.float64), rowvar=False), R.cov_bound(x, absx))
    print(f"moments ({n}, {D}): worst |cov - np.cov| / bound {worst:.3f}")
    assert bad == 0, worst
    again = _gpu_moments(x)
    assert torch.equal(again._outer, fm._outer) and torch.equal(again.sum, fm.sum)              # the same bits from call to call


# ---------------------------------------------------------------------------------------------- KID sums
@pytest.mark.parametrize("num_subsets", [1, 3])
@pytest.mark.parametrize("m", [2, 17, 24, 100])
def test_kid_sums_are_exact_where_every_order_is(m, num_subsets):
    g = np.random.RandomState(m + num_subsets)
    fake, real = R.exact_kid_features(3 * m, seed=m), R.exact_kid_features(3 * m, seed=m + 50)
    idx_f, idx_r = R.draw_subsets(g, 3 * m, 3 * m, num_subsets, m)                # unsorted draws without replacement
    fake[idx_f[0, 1]] = fake[idx_f[0, 0]]                                        # two POSITIONS of a subset that hold equal rows: the pair counts
    idx_r[0, 1] = idx_r[0, 0]                                                    # ... and one row at two positions
    if num_subsets > 1:
        idx_f[1, 0], idx_r[2, m - 1] = idx_f[0, 0], idx_r[0, 0]                  # a row shared between subsets (idx_f[1] may now hold it twice: allowed)
    want, _ = R.kid_sums_ref(fake, real, idx_f, idx_r)
    got = FK.kid_subset_sums(torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda(), idx_f, idx_r)
    assert got.shape == (num_subsets, 3) and got.dtype == np.float64
    assert np.array_equal(_bits(got), _bits(want)), (got - want).tolist()
    assert idx_f[0, 0] != idx_f[0, 1] and (fake[idx_f[0, 0]] == fake[idx_f[0, 1]]).all()         # (the restatement drops position i == j only)


@functools.lru_cache(maxsize=None)
def _kid_case(m, D):
    g = np.random.RandomState(m + D)
    fake, real = R.random_features(3 * m, D, seed=m), R.random_features(3 * m, D, seed=m + 1)
    idx_f, idx_r = R.draw_subsets(g, 3 * m, 3 * m, 2, m)
    ref, mags = R.kid_sums_ref(fake, real, idx_f, idx_r)
    return fake, real, idx_f, idx_r, ref, mags


@pytest.mark.parametrize("m,D", [(16, 20), (33, 100), (1000, 2048)])
def test_kid_sums_within_their_bounds(m, D):
    fake, real, idx_f, idx_r, ref, mags = _kid_case(m, D)
    f, r = torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda()
    got = FK.kid_subset_sums(f, r, idx_f, idx_r)
    bound = R.kid_sums_bound(mags, m, D)
    bad, worst = R.check_le(got, ref, bound)
    print(f"kid sums (m = {m}, D = {D}): worst |S - ref| / bound {worst:.4f}; relative errors {(np.abs(got - ref) / ref).max():.2e}")
    assert bad == 0, worst
    assert np.array_equal(_bits(FK.kid_subset_sums(f, r, idx_f, idx_r)), _bits(got))            # the same bits from call to call
    kid, kid_ref = R.kid_from_sums(got, m), R.kid_from_sums(ref, m)
    assert abs(kid - kid_ref) <= R.kid_bound_from_sums(bound, mags, m)


def test_kid_draws_like_the_reference_and_runs_on_the_gpu_stores():
    fake, real = R.random_features(90, 48, seed=1), R.random_features(70, 48, seed=2)
    got = FK.kid(torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda(), num_subsets=5, max_subset_size=32, rng=np.random.RandomState(3))
    want, tol = R.calc_kid_ref(real, fake, 5, 32, np.random.RandomState(3))
    assert abs(got - want) <= tol, (got, want, tol)
    whole = FK.kid(torch.from_numpy(fake).cuda(), torch.from_numpy(real).cuda(), num_subsets=2, max_subset_size=1000, rng=np.random.RandomState(3))
    want, tol = R.calc_kid_ref(real, fake, 2, 1000, np.random.RandomState(3))             # m = 70: the smaller store
    assert abs(whole - want) <= tol


# ---------------------------------------------------------------------------------------------- val_step / evaluate_3d
@pytest.fixture(scope="module")
def model_and_scenes():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    cfg = dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
               diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                              denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=32, channels_cfg=[1, 1, 2],
                                             resblocks_per_downsample=1, dropout=0.0, use_scale_shift_norm=True, num_heads=4, attention_res=[32],
                                             norm_cfg=dict(type="GN", num_groups=8))),
               decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
                            dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256),
               decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss"), cache_size=0,
               test_cfg=dict(img_size=(32, 32), density_thresh=0.1, density_step=4))
    m = MODELS.build(cfg)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().eval()
    code = S.make_scene_batch(2, seed=40).cuda()
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        grid, bits = m.get_density(m.decoder_ema, code, cfg=m.test_cfg, jitters=[torch.rand(64 ** 3, 3, generator=g).cuda() for _ in range(4)])
    return m, [dict(param=dict(code=code[i], density_grid=grid[i], density_bitfield=bits[i])) for i in range(2)]


def _batch(scenes, views, test_imgs=None):
    from ssdnerf_amd import synthetic as S
    n = len(scenes)
    data = dict(code=scenes, test_poses=S.spiral_poses()[views].cuda()[None].expand(n, -1, -1, -1).contiguous(),
                test_intrinsics=S.cars_intrinsics(32, 32).cuda()[None, None].expand(n, len(views), -1).contiguous())
    if test_imgs is not None:
        data["test_imgs"] = test_imgs
    return data


def test_evaluate_3d_reports_fid_and_kid_of_rendered_views(model_and_scenes):
    from ssdnerf_amd import parallel
    m, scenes = model_and_scenes
    views = [10, 70, 130, 200]
    pred = m.val_step(_batch(scenes, views))["pred_imgs"]
    assert pred.shape == (2, 4, 3, 32, 32)
    g = torch.Generator().manual_seed(1)
    hwc = pred.permute(0, 1, 3, 4, 2).cpu()
    target = (hwc + 0.1 * torch.randn(hwc.shape, generator=g)).clamp(0, 1)                       # on the host, as a data loader hands it over
    batches = [_batch(scenes[:1], views, test_imgs=target[:1]), _batch(scenes[1:], views, test_imgs=target[1:])]
    plain = parallel.evaluate_3d(m, batches)
    ext = R.PoolProject(32, 32, dim=48, seed=0)
    metric = FK.FIDKID(num_images=8, max_subset_size=8, num_subsets=3, extractor=ext, feature_dim=48, seed=0)
    out = parallel.evaluate_3d(m, batches, metrics=[metric], feed_batch_size=3)
    assert set(out) == set(plain) | {"fid", "fid_mean", "fid_cov", "kid"} and all(out[k] == plain[k] for k in plain)
    assert out["fid"] == out["fid_mean"] + out["fid_cov"] and metric.result_dict["kid"] == out["kid"]
    # what was stored is the extractor's answer to the views in [-1, 1] with their channels flipped (bgr2rgb defaults to True), fakes and reals, fed batch
    # by batch (one scene each) in pieces of feed_batch_size
    fakes, reals = metric.features("fakes"), metric.features("reals")
    assert fakes.is_cuda and fakes.shape == reals.shape == (8, 48)
    assert metric.bgr2rgb is True
    assert torch.equal(fakes, torch.cat([ext((b * 2 - 1).flip(1)) for scene in pred for b in scene.split(3)]))
    assert torch.equal(reals, torch.cat([ext((b * 2 - 1).flip(1)) for scene in target.cuda().permute(0, 1, 4, 2, 3) for b in scene.split(3)]))
    # the scores against the restatement on those features; 8 samples of 48 features: 41 null directions at least
    f32, r32 = fakes.cpu().numpy(), reals.cpu().numpy()
    f64, r64 = f32.astype(np.float64), r32.astype(np.float64)
    mf, cf, mr, cr = f64.mean(0), np.cov(f64, rowvar=False), r64.mean(0), np.cov(r64, rowvar=False)
    want = R.frechet_ref(mf, cf, mr, cr)
    tol = R.fid_null_tol(cf, cr, float(R.cov_bound(f32).max()), float(R.cov_bound(r32).max()), 48) + 8 * 48 * R.U * float(mf @ mf + mr @ mr)
    kid, kid_tol = R.calc_kid_ref(r32, f32, 3, 8, np.random.RandomState(0))
    print(f"fid {out['fid']:.9f} (restatement {want[0]:.9f}, tolerance {tol:.2e}), kid {out['kid']:.9f} ({kid * 1000:.9f}, tolerance {kid_tol * 1000:.2e})")
    assert abs(out["fid"] - want[0]) <= tol and abs(out["fid_mean"] - want[1]) <= tol
    assert abs(out["kid"] - kid * 1000) <= kid_tol * 1000
    assert out["fid"] > 0 and tol < 0.1 * out["fid"]                                           # (the tolerance means something)
