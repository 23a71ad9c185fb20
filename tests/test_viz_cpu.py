"""PNG output without a GPU (ssdnerf_amd/viz.py): the numpy path of ``filter_rows`` and of the colour map against the independent
restatement (tests/_viz_ref.py) and the matplotlib fixture (tests/golden/viridis_map.npz), the files through the project's own PNG reader, and the
``viz_dir`` plumbing of ``val_step`` / ``evaluate_3d`` on a CPU model over the srn_tiny fixture tree.  Every comparison is byte or pixel equality.

Rendering and scoring have no CPU path in this project, so the ``val_step`` tests replace exactly those two calls (``model.render`` and
``models.image_metrics``) by deterministic stand-ins; everything between the rendered image and the files is the product's code."""
import glob
import os

import numpy as np
import pytest
import torch

import _viz_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX = "srn_tiny/cars"


@pytest.fixture
def in_golden(monkeypatch):
    """the fixture's image paths are relative to tests/golden"""
    monkeypatch.chdir(GOLDEN)


@pytest.fixture(scope="module")
def fixture():
    return np.load(os.path.join(GOLDEN, "viridis_map.npz"))


def _t(a):
    return None if a is None else torch.from_numpy(a)


# ---------------------------------------------------------------------------------------------- rows
def test_restatement_meets_its_conditions():
    """over the crafted inputs the restatement chooses every filter type; a constant image is the tie case (Up wins over Paeth at equal score);
    un-filtering gives the scanlines back"""
    seen = set()
    for h, w, with_target in R.SHAPES:
        pred, target = R.case(h, w, with_target, "u8", "u8")
        rows = R.filter_rows_ref(pred, target)
        seen |= set(R.filter_types(rows).reshape(-1).tolist())
        assert np.array_equal(R.unfilter(rows), R.quantise(pred, target))
    assert seen == {0, 1, 2, 3, 4}, seen
    assert R.filter_types(R.filter_rows_ref(np.full((1, 4, 5, 3), 77, np.uint8))).tolist() == [[1, 2, 2, 2]]


def test_byte_rules_of_the_restatement():
    """k / 255 gives k under both rules; ties go to even for pred and down for target; outside [0, 1] clamps; NaN is 0"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).reshape(1, 1, 256, 1).repeat(3, axis=3)
    assert np.array_equal(R.quantise(k).reshape(256, 3)[:, 0], np.arange(256)) and np.array_equal(R.quantise(k, k).reshape(-1, 3)[:256, 0], np.arange(256))
    x = np.float32([[[[2.5 / 255, 3.5 / 255, -1.0], [7.0, np.nan, 0.999]]]])
    assert R.quantise(x).reshape(-1).tolist() == [2, 4, 0, 255, 0, 255]
    assert R.quantise(x, x).reshape(-1)[:6].tolist() == [2, 3, 0, 255, 0, 254]


@pytest.mark.parametrize("kinds", R.KINDS, ids=lambda k: "-".join(k))
def test_filter_rows_cpu_equals_restatement(kinds):
    from ssdnerf_amd import viz
    seen = set()
    for h, w, with_target in R.SHAPES:
        pred, target = R.case(h, w, with_target, *kinds)
        want = R.filter_rows_ref(pred, target)
        got = viz.filter_rows(_t(pred), _t(target))
        assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (2, h, 1 + 3 * w * (2 if with_target else 1))
        assert np.array_equal(got.numpy(), want), (kinds, h, w, with_target)
        seen |= set(R.filter_types(want).reshape(-1).tolist())
    assert seen == {0, 1, 2, 3, 4}, seen


def test_filter_rows_rejects_bad_operands():
    from ssdnerf_amd import viz
    good = torch.zeros(1, 2, 2, 3)
    for bad in (torch.zeros(2, 2, 3), torch.zeros(1, 2, 2, 4), torch.zeros(1, 2, 2, 3, dtype=torch.float64), torch.zeros(0, 2, 2, 3)):
        with pytest.raises(ValueError):
            viz.filter_rows(bad)
    with pytest.raises(ValueError):
        viz.filter_rows(good, torch.zeros(1, 2, 3, 3))


@pytest.mark.parametrize("kinds", [("f32", "f32"), ("u8", "u8")], ids=lambda k: "-".join(k))
def test_png_bytes_decode_to_the_expected_pixels(kinds):
    from ssdnerf_amd import viz
    from ssdnerf_amd.datasets import decode_png
    for h, w, with_target in R.SHAPES:
        pred, target = R.case(h, w, with_target, *kinds)
        width = w * (2 if with_target else 1)
        want = R.quantise(pred, target).reshape(2, h, width, 3)
        rows = viz.filter_rows(_t(pred), _t(target))
        for i in range(2):
            for level in (0, 6):
                data = viz.png_bytes(rows[i], width, h, level=level)
                assert np.array_equal(decode_png(data), want[i]), (h, w, with_target, level)
    with pytest.raises(ValueError):
        viz.png_bytes(rows[0], width + 1, h)


def test_png_bytes_decode_with_pillow():
    Image = pytest.importorskip("PIL.Image")
    import io
    from ssdnerf_amd import viz
    for h, w, with_target in R.SHAPES:
        pred, target = R.case(h, w, with_target, "f32", "u8")
        width = w * (2 if with_target else 1)
        want = R.quantise(pred, target).reshape(2, h, width, 3)
        rows = viz.filter_rows(_t(pred), _t(target))
        with Image.open(io.BytesIO(viz.png_bytes(rows[1], width, h))) as im:
            assert im.mode == "RGB" and im.size == (width, h)
            assert np.array_equal(np.asarray(im), want[1])


# ---------------------------------------------------------------------------------------------- colour map and layout
def test_shipped_table_is_the_fixtures(fixture):
    from ssdnerf_amd import viz
    table = viz.viridis_table()
    assert table.dtype == np.uint8 and table.shape == (256, 3) and np.array_equal(table, fixture["table"])


@pytest.mark.parametrize("key,code_range", [("m1_1", (-1, 1)), ("m2_2", (-2, 2))])
def test_colour_map_reproduces_matplotlib(fixture, key, code_range):
    """the restatement and the CPU path against what matplotlib gave for every fixture input (bin edges and their float32 neighbours, the range's ends,
    values outside, +-inf, NaN, random values)"""
    from ssdnerf_amd import viz
    x, want = fixture["x_" + key], fixture["rgb_" + key]
    assert np.isnan(x).any() and np.isinf(x).any() and x.size > 4000
    assert np.array_equal(R.colour_map_ref(x, fixture["table"], *code_range), want)
    pad = (-x.size) % 3
    xs = np.concatenate([x, np.zeros(pad, np.float32)])
    code = torch.from_numpy(xs.reshape(1, 3, 1, 1, -1).copy())             # one row per plane: the layout is the identity
    got = viz.code_plane_rgb(code, code_range, flip_z=True).numpy().reshape(-1, 3)[:x.size]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("flip_z", [False, True])
def test_plane_layout_is_the_references(fixture, flip_z):
    from ssdnerf_amd import viz
    g = np.random.default_rng(3)
    code = g.uniform(-1.2, 1.2, (2, 3, 2, 3, 5)).astype(np.float32)
    sheet = code[..., ::-1, :] if not flip_z else code
    sheet = sheet.transpose(0, 1, 3, 2, 4).reshape(2, 9, 10)               # triplane_decoder.py:188-191
    assert np.array_equal(R.plane_sheet_ref(code, flip_z), sheet)
    want = R.colour_map_ref(sheet, fixture["table"], -1, 1)
    got = viz.code_plane_rgb(torch.from_numpy(code), (-1, 1), flip_z=flip_z)
    assert tuple(got.shape) == (2, 9, 10, 3) and np.array_equal(got.numpy(), want)


# ---------------------------------------------------------------------------------------------- val_step / evaluate_3d on a CPU model
def _model(**test_cfg):
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.registry import MODELS
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 2, 5, 7), code_activation=dict(type="TanhCode", scale=2), grid_size=16,
                          decoder=dict(type="TriPlaneDecoder", base_layers=[6, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64]),
                          init_from_mean=True, train_cfg=dict(optimizer=dict(type="Adam", lr=0.01)), test_cfg=dict(test_cfg)))
    with torch.no_grad():
        m.init_code.copy_(torch.linspace(-1.5, 1.5, m.init_code.numel()).view_as(m.init_code))
    return m.eval()


def _stand_ins(m, monkeypatch, shift=0.0):
    """the two GPU-only calls of ``_eval_test_views``: a render that depends on the cameras only, and PSNR with a simple second score"""
    from ssdnerf_amd import models

    def render(decoder, code, density_bitfield, h, w, intrinsics, poses, cfg=dict()):
        S, V = poses.shape[:2]
        seed = poses.reshape(S, V, 16).sum(-1)[..., None, None, None]
        yy, xx, cc = torch.meshgrid(torch.arange(h), torch.arange(w), torch.arange(3), indexing="ij")
        return (torch.sin(seed + 0.37 * yy + 0.11 * xx + cc) * 0.6 + 0.5 + shift).to(torch.float32), None

    def image_metrics(pred, target):
        mse = (pred - target).square().flatten(2).mean(-1)
        return 10 * -torch.log10(mse + 1e-6), 1 - (pred - target).abs().flatten(2).mean(-1)

    monkeypatch.setattr(m, "render", render)
    monkeypatch.setattr(models, "image_metrics", image_metrics)


def _batch(scene_ids, m, with_imgs=True, step=2):
    from ssdnerf_amd import datasets as D
    ds = D.ShapeNetSRN(PREFIX, step=step, num_test_imgs=2)                   # step 2: alpha_01 and zeta_03, 4 conditioning + 2 test views of 8 x 8
    recs = [ds[i] for i in scene_ids]
    g = torch.Generator().manual_seed(5)
    code = torch.randn(len(recs), *m.code_size, generator=g).clamp(-1.4, 1.4)
    data = dict(scene_id=[r["scene_id"] for r in recs], scene_name=[r["scene_name"] for r in recs],
                test_poses=torch.stack([r["test_poses"] for r in recs]), test_intrinsics=torch.stack([r["test_intrinsics"] for r in recs]),
                code=[dict(param=dict(code=code[i], density_grid=m.get_init_density_grid(None), density_bitfield=m.get_init_density_bitfield(None)))
                      for i in range(len(recs))])
    if with_imgs:
        data.update(test_imgs=torch.stack([r["test_imgs"] for r in recs]), test_img_paths=[r["test_img_paths"] for r in recs])
    return data


def _read(path):
    from ssdnerf_amd.datasets import decode_png
    with open(path, "rb") as f:
        return decode_png(f.read(), path)


def _names(data, out):
    names = []
    for s, scene in enumerate(data["scene_name"]):
        for v, path in enumerate(data["test_img_paths"][s]):
            stem = os.path.splitext(os.path.basename(path))[0]
            names.append("scene_{}_{}_psnr{:02.1f}_ssim{:.2f}_lpips{:.3f}.png".format(scene, stem, out["test_metrics"]["psnr"][s, v],
                                                                                      out["test_metrics"]["ssim"][s, v], float("nan")))
    return names


def test_val_step_writes_views_and_code_planes(in_golden, tmp_path, monkeypatch):
    m = _model()
    _stand_ins(m, monkeypatch)
    data = _batch([0, 1], m)
    viz_dir = str(tmp_path / "viz")
    out = m.val_step(dict(data), viz_dir=viz_dir)
    names = _names(data, out)
    planes = ["scene_" + n + ".png" for n in data["scene_name"]] + ["scene_000_mean.png"]
    assert sorted(os.listdir(viz_dir)) == sorted(names + planes) and all("_lpipsnan.png" in n for n in names)
    pred = torch.round(out["pred_imgs"].permute(0, 1, 3, 4, 2) * 255).to(torch.uint8).numpy()
    target = (data["test_imgs"] * 255).to(torch.uint8).numpy()              # the reference's truncation (base_nerf.py:581-582)
    for i, name in enumerate(names):
        img = _read(os.path.join(viz_dir, name))
        assert img.shape == (8, 16, 3)
        assert np.array_equal(img[:, :8], target[i // 2, i % 2]) and np.array_equal(img[:, 8:], pred[i // 2, i % 2])
    table = np.load(os.path.join(GOLDEN, "viridis_map.npz"))["table"]
    for i, name in enumerate(planes[:2]):
        want = R.colour_map_ref(R.plane_sheet_ref(out["code"][i:i + 1].numpy(), False), table, -1, 1)[0]
        img = _read(os.path.join(viz_dir, name))
        assert img.shape == (3 * 5, 2 * 7, 3) and np.array_equal(img, want)
    mean = R.colour_map_ref(R.plane_sheet_ref(m.init_code[None].numpy(), False), table, -1, 1)[0]
    assert np.array_equal(_read(os.path.join(viz_dir, planes[2])), mean)
    # a second call with other scores replaces the files: exactly one per view
    _stand_ins(m, monkeypatch, shift=0.2)
    out2 = m.val_step(dict(data), viz_dir=viz_dir)
    names2 = _names(data, out2)
    assert set(names2).isdisjoint(names) and sorted(os.listdir(viz_dir)) == sorted(names2 + planes)


def test_val_step_viz_dir_from_test_cfg_and_unscored_names(in_golden, tmp_path, monkeypatch):
    """``test_cfg['viz_dir']`` stands in for the keyword, ``clip_range`` is the code range, ``viz_compress_level`` reaches zlib; a batch without
    ground truth gets the numbered names and the prediction alone"""
    viz_dir = str(tmp_path / "cfg")
    m = _model(viz_dir=viz_dir, clip_range=[-2, 2], viz_compress_level=0, img_size=(9, 5))
    _stand_ins(m, monkeypatch)
    data = _batch([0, 1], m, with_imgs=False)
    out = m.val_step(dict(data))
    views = ["scene_{}_{:03d}.png".format(n, v) for n in data["scene_name"] for v in range(2)]
    planes = ["scene_" + n + ".png" for n in data["scene_name"]] + ["scene_000_mean.png"]
    assert sorted(os.listdir(viz_dir)) == sorted(views + planes)
    pred = torch.round(out["pred_imgs"].permute(0, 1, 3, 4, 2) * 255).to(torch.uint8).numpy()
    for i, name in enumerate(views):
        assert np.array_equal(_read(os.path.join(viz_dir, name)), pred[i // 2, i % 2])
    table = np.load(os.path.join(GOLDEN, "viridis_map.npz"))["table"]
    want = R.colour_map_ref(R.plane_sheet_ref(out["code"][:1].numpy(), False), table, -2, 2)[0]
    assert np.array_equal(_read(os.path.join(viz_dir, planes[0])), want)
    size0 = os.path.getsize(os.path.join(viz_dir, views[0]))
    assert size0 > 9 * (1 + 15)                                             # stored, not deflated: at least the filtered rows themselves


def test_val_step_needs_scene_names_and_changes_nothing_without_viz_dir(in_golden, tmp_path, monkeypatch):
    m = _model()
    _stand_ins(m, monkeypatch)
    data = _batch([0, 1], m)
    with pytest.raises(KeyError, match="scene_name"):
        m.val_step({k: v for k, v in data.items() if k != "scene_name"}, viz_dir=str(tmp_path / "a"))
    before = (set(os.listdir(tmp_path)), set(os.listdir(".")))
    plain = m.val_step(dict(data))
    assert (set(os.listdir(tmp_path)), set(os.listdir("."))) == before     # nothing written, neither there nor in the working directory
    with_viz = m.val_step(dict(data), viz_dir=str(tmp_path / "b"))
    assert set(plain) == set(with_viz) == {"log_vars", "num_samples", "pred_imgs", "code", "density_grid", "density_bitfield", "test_metrics"}
    assert plain["log_vars"] == with_viz["log_vars"] and plain["num_samples"] == with_viz["num_samples"]
    for key in ("pred_imgs", "code", "density_grid", "density_bitfield"):
        assert torch.equal(plain[key], with_viz[key]), key
    for key in ("psnr", "ssim"):
        assert torch.equal(plain["test_metrics"][key], with_viz["test_metrics"][key])


def test_evaluate_3d_writes_every_viz_step_th_batch(in_golden, tmp_path, monkeypatch):
    from ssdnerf_amd import parallel
    m = _model()
    _stand_ins(m, monkeypatch)
    batches = [_batch([i], m, step=1) for i in (0, 1, 2)]                    # the tree's three scenes, one per batch
    viz_dir = str(tmp_path / "eval")
    res = parallel.evaluate_3d(m, batches, viz_dir=viz_dir, viz_step=2)
    assert np.isfinite(res["test_psnr"])
    written = {f.split("_psnr")[0].rsplit("_", 1)[0] for f in os.listdir(viz_dir) if "_psnr" in f}
    assert written == {"scene_" + batches[0]["scene_name"][0], "scene_" + batches[2]["scene_name"][0]}
    assert not glob.glob(os.path.join(viz_dir, "scene_" + batches[1]["scene_name"][0] + "*"))
    none_dir = tmp_path / "none"
    parallel.evaluate_3d(m, batches)                                       # no viz_dir: val_step gets no such keyword, nothing is written
    assert not none_dir.exists()


def test_write_views_escapes_names_for_glob(tmp_path):
    """a scene name with glob characters removes its own stale files only"""
    from ssdnerf_amd import viz
    pred = torch.rand(1, 1, 3, 4, 3, generator=torch.Generator().manual_seed(0))
    metrics = dict(psnr=torch.tensor([[21.26]]), ssim=torch.tensor([[0.876]]), lpips=torch.tensor([[0.12345]]))
    other = tmp_path / "scene_ab_000_old.png"
    other.write_bytes(b"x")
    stale = tmp_path / "scene_[ab]_000_psnr1.0_ssim0.10_lpipsnan.png"
    stale.write_bytes(b"x")
    paths = viz.write_views(str(tmp_path), ["[ab]"], pred, pred, img_paths=[["rgb/000.png"]], metrics=metrics)
    assert [os.path.basename(p) for p in paths] == ["scene_[ab]_000_psnr21.3_ssim0.88_lpips0.123.png"]
    assert other.exists() and not stale.exists() and os.path.exists(paths[0])
