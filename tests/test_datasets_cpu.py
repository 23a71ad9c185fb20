"""The host layers of ssdnerf_amd/datasets.py: ``ShapeNetSRN``'s ``ds[i]`` against what the reference's own ``parse_scene`` returned on the
fixture tree (tests/golden/srn_tiny, srn_tiny.npz; make_golden_srn.py), the scene list and its caches, the built-in PNG reader, the loader's
scene order, and the pixel cache.  No GPU and no library: every test fails at import without the feature."""
import importlib.util
import json
import os
import pickle
import random
import shutil
import zlib

import numpy as np
import pytest
import torch

from ssdnerf_amd import datasets as D
from ssdnerf_amd import parallel
from ssdnerf_amd.config import build_dataloader, build_dataset

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX = "srn_tiny/cars"
SORTED_SCENES = ["alpha_01", "mid_02", "zeta_03"]


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_srn", os.path.join(GOLDEN, "make_golden_srn.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "srn_tiny.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture()
def in_golden(monkeypatch):
    """the fixture's image paths are relative to tests/golden"""
    monkeypatch.chdir(GOLDEN)


def _equal(mine, recorded, what):
    if isinstance(mine, torch.Tensor):
        a = mine.contiguous().numpy()
        assert a.dtype == recorded.dtype and a.shape == recorded.shape, (what, a.dtype, a.shape, recorded.dtype, recorded.shape)
        assert np.array_equal(a.view(np.uint8), recorded.view(np.uint8)), what          # bit for bit
    elif isinstance(mine, (list, tuple)):
        assert list(mine) == recorded.tolist(), what
    else:
        assert type(mine) in (int, str) and mine == recorded.item(), what


def test_fixture_records_every_keyword_set(fixture):
    sets = json.loads(str(fixture["sets_json"]))
    assert {"train", "val_uncond", "val_cond", "val_cond_override", "num_train_3", "random_test", "code_only"} <= set(sets)
    assert int(fixture["train/n"]) == 3 and int(fixture["val_cond/n"]) == 2


def test_scene_dicts_equal_the_reference_key_for_key_bit_for_bit(fixture, in_golden):
    sets = json.loads(str(fixture["sets_json"]))
    for name, kwargs in sets.items():
        random.seed(0)
        ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **kwargs))
        assert len(ds) == int(fixture[name + "/n"]), name
        for i in range(len(ds)):
            mine = ds[i]
            assert sorted(mine) == fixture[f"{name}/{i}/__keys__"].tolist(), (name, i)         # a key absent there is absent here
            for key, value in mine.items():
                _equal(value, fixture[f"{name}/{i}/{key}"], (name, i, key))


def test_scene_dicts_are_the_same_through_the_builtin_png_reader(fixture, in_golden, monkeypatch):
    """a machine without Pillow: ``read_image`` falls to the built-in reader, and ``ds[i]`` is still the reference's, bit for bit"""
    monkeypatch.setattr(D, "_have_pil", lambda: False)
    ds = D.ShapeNetSRN(PREFIX)
    for i in range(3):
        mine = ds[i]
        for key in ("cond_imgs", "cond_poses", "cond_intrinsics"):
            _equal(mine[key], fixture[f"train/{i}/{key}"], (i, key))


def test_images_are_fp32_in_unit_range_and_poses_are_normalised(in_golden):
    d = D.ShapeNetSRN(PREFIX)[1]
    assert d["cond_imgs"].dtype == torch.float32 and tuple(d["cond_imgs"].shape) == (4, 8, 8, 3) and "test_imgs" not in d
    assert float(d["cond_imgs"].min()) >= 0 and float(d["cond_imgs"].max()) <= 1
    raw = D.load_pose(d["cond_img_paths"][0].replace("rgb", "pose").replace(".png", ".txt"))
    assert torch.equal(d["cond_poses"][0, :3, :3], raw[:3, :3]) and torch.equal(d["cond_poses"][0, :3, 3], raw[:3, 3] / 0.5)
    assert d["cond_poses"][0, 3].tolist() == [0, 0, 0, 1]
    assert D.load_intrinsics(os.path.join(PREFIX, "mid_02", "intrinsics.txt")) == (8.203125, 8.203125, 4.0, 4.0, 8, 8)


def test_scene_order_max_num_scenes_step_and_names(in_golden):
    def names(**kw):
        ds = D.ShapeNetSRN(PREFIX, load_imgs=False, **kw)
        return [ds[i]["scene_name"] for i in range(len(ds))]

    assert names() == SORTED_SCENES
    assert names(max_num_scenes=2) == SORTED_SCENES[:2]
    assert names(step=2) == SORTED_SCENES[::2]
    assert names(max_num_scenes=1, step=2) == SORTED_SCENES[:1]
    assert names(max_num_scenes=0) == []
    assert names(scene_id_as_name=True) == ["0000", "0001", "0002"]
    two = D.ShapeNetSRN([PREFIX, PREFIX], load_imgs=False)                                     # a list of prefixes: scenes of all of them
    assert len(two) == 6 and [two[i]["scene_name"] for i in range(6)] == sorted(SORTED_SCENES * 2)


def test_key_rules_without_the_fixture(in_golden):
    assert sorted(D.ShapeNetSRN(PREFIX, code_only=True)[0]) == ["scene_id", "scene_name"]
    d = D.ShapeNetSRN(PREFIX, load_cond_data=False, num_test_imgs=2)[0]
    assert not any(k.startswith("cond_") for k in d) and tuple(d["test_imgs"].shape) == (2, 8, 8, 3)
    d = D.ShapeNetSRN(PREFIX, load_test_data=False, num_test_imgs=2)[0]
    assert not any(k.startswith("test_") for k in d) and tuple(d["cond_imgs"].shape) == (4, 8, 8, 3)
    d = D.ShapeNetSRN(PREFIX, num_train_imgs=0)[1]                                             # an empty conditioning list: no cond keys at all
    assert not any(k.startswith("cond_") for k in d) and tuple(d["test_poses"].shape) == (4, 4, 4)


def test_cache_path_is_written_then_read_and_a_reference_pickle_loads(in_golden, tmp_path):
    cache = str(tmp_path / "cache.pkl")
    first = D.ShapeNetSRN(PREFIX, cache_path=cache)
    assert os.path.exists(cache)
    with open(cache, "rb") as f:
        scenes = pickle.load(f)
    assert [s["image_paths"][0].split("/")[-3] for s in scenes] == SORTED_SCENES and sorted(scenes[0]) == ["image_paths", "intrinsics", "poses"]
    assert scenes[0]["intrinsics"] == (8.203125, 8.203125, 4.0, 4.0, 8, 8) and scenes[1]["poses"][0].dtype == torch.float32
    again = D.ShapeNetSRN("no/such/folder", cache_path=cache)                                # read back: the folder is not looked at
    assert again.image_paths == first.image_paths and torch.equal(again.poses, first.poses)
    # a file in the reference's layout, built here: a list of dicts with a 6-tuple, a path list and 4 x 4 float32 tensors (mmcv.dump: protocol 2)
    theirs = [dict(intrinsics=(8.203125, 8.203125, 4.0, 4.0, 8, 8), image_paths=[f"{PREFIX}/zeta_03/rgb/00000{k}.png" for k in (0, 1)],
                   poses=[torch.eye(4), torch.eye(4) * 2])]
    with open(tmp_path / "theirs.pkl", "wb") as f:
        pickle.dump(theirs, f, protocol=2)
    d = D.ShapeNetSRN("no/such/folder", cache_path=str(tmp_path / "theirs.pkl"))[0]
    assert d["scene_name"] == "zeta_03" and tuple(d["cond_imgs"].shape) == (2, 8, 8, 3)
    assert torch.equal(d["cond_poses"][1, :3, 3], torch.full((3,), 0.0)) and torch.equal(d["cond_poses"][1, :3, :3], torch.eye(3) * 2)


def test_code_dir_loads_the_scenes_that_have_a_file(in_golden, tmp_path):
    torch.save(dict(param=dict(code_=torch.arange(6.0)), optimizer=None), tmp_path / "mid_02.pth")
    ds = D.ShapeNetSRN(PREFIX, code_dir=str(tmp_path), code_only=True)
    assert "code" not in ds[0] and "code" not in ds[2]
    assert torch.equal(ds[1]["code"]["param"]["code_"], torch.arange(6.0))


def test_ragged_view_sizes_raise(in_golden, tmp_path):
    gen = _generator()
    shutil.copytree(os.path.join(PREFIX, "mid_02"), tmp_path / "cars" / "mid_02")
    odd = np.zeros((4, 8, 3), np.uint8)
    with open(tmp_path / "cars" / "mid_02" / "rgb" / "000002.png", "wb") as f:
        f.write(gen.encode_png(odd, [0]))
    ds = D.ShapeNetSRN(str(tmp_path / "cars"))
    with pytest.raises(ValueError, match="different sizes"):
        ds.load_pixels()


# ---------------------------------------------------------------------------------------------- PNG
def _tree_pngs():
    return sorted(os.path.join(r, f) for r, _, fs in os.walk(os.path.join(GOLDEN, "srn_tiny")) for f in fs if f.endswith(".png"))


def test_builtin_png_reader_equals_the_pixels_the_tree_was_written_from(fixture):
    files = _tree_pngs()
    assert len(files) == 16
    channels = set()
    for path in files:
        with open(path, "rb") as f:
            got = D.decode_png(f.read(), path)
        raw = fixture["pixels/" + os.path.relpath(path, GOLDEN).replace(os.sep, "/")]
        channels.add(raw.shape[2])
        assert got.dtype == np.uint8 and np.array_equal(got, raw[:, :, :3]), path          # alpha dropped, not composited
    assert channels == {3, 4}


def test_builtin_png_reader_equals_pil_on_every_file():
    Image = pytest.importorskip("PIL.Image")
    for path in _tree_pngs():
        with open(path, "rb") as f:
            got = D.decode_png(f.read(), path)
        assert np.array_equal(got, np.asarray(Image.open(path).convert("RGB"))), path
        assert np.array_equal(D.read_image(path), got)


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("bpp", [3, 4])
def test_builtin_png_reader_undoes_every_filter(kind, bpp):
    gen = _generator()
    img = np.random.default_rng(kind * 2 + bpp).integers(0, 256, (5, 7, bpp), dtype=np.uint8)
    img[0, 0], img[1, 1] = 255, 0                                                            # wrap-around in both directions
    assert np.array_equal(D.decode_png(gen.encode_png(img, [kind])), img[:, :, :3])
    assert np.array_equal(D.decode_png(gen.encode_png(img, [kind, 4, 3, 2, 1, 0])), img[:, :, :3])


def test_builtin_png_reader_refuses_what_it_does_not_handle(tmp_path):
    gen = _generator()
    img = np.zeros((2, 2, 3), np.uint8)
    with pytest.raises(ValueError, match="sixteen.png.*bit depth 16"):
        D.decode_png(gen.encode_png(img, [0], bit_depth=16), "sixteen.png")
    with pytest.raises(ValueError, match="adam7.png.*interlace 1"):
        D.decode_png(gen.encode_png(img, [0], interlace=1), "adam7.png")
    with pytest.raises(ValueError, match="not a PNG"):
        D.decode_png(b"GIF89a", "x.gif")
    bad = bytearray(gen.encode_png(img, [0]))
    with pytest.raises(ValueError, match="filter type 7"):
        raw = zlib.compress(bytes([7, 0, 0, 0, 0, 0, 0] * 2))
        D.decode_png(bytes(bad[:33]) + gen._chunk(b"IDAT", raw) + gen._chunk(b"IEND", b""), "seven.png")


# ---------------------------------------------------------------------------------------------- scene order of the loader
class _Scenes:
    """a dataset as far as ``scene_indices`` looks at it"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


@pytest.mark.parametrize("n", [3, 16, 701])
@pytest.mark.parametrize("world", [1, 2, 8])
def test_evaluation_order_is_shard_scenes_with_a_ragged_last_batch(n, world):
    seen = []
    for rank in range(world):
        loader = build_dataloader(_Scenes(n), 4, rank=rank, world_size=world)
        order = loader.scene_indices()
        assert order == list(parallel.shard_scenes(n, rank, world))
        assert len(loader) == -(-len(order) // 4)                                             # no padding: the last batch is short
        seen += order
    assert seen == list(range(n))


@pytest.mark.parametrize("n,world,spg", [(3, 1, 2), (16, 2, 4), (701, 8, 8), (701, 2, 3), (5, 8, 2)])
def test_training_order_without_split(n, world, spg):
    num = -(-n // (world * spg)) * spg                                                       # ceil(n / world / spg) * spg: DESIGN.md section 16
    g = torch.Generator()
    g.manual_seed(7 + 2)
    perm = torch.randperm(n, generator=g).tolist()
    padded = (perm * (num * world // n + 1))[:num * world]                                   # the padding wraps from the front
    for rank in range(world):
        loader = build_dataloader(_Scenes(n), spg, shuffle=True, seed=7, rank=rank, world_size=world)
        a = loader.scene_indices(2)
        assert len(a) == num and len(a) % spg == 0 and a == padded[rank::world]
        assert a == loader.scene_indices(2)                                                  # same seed and epoch: the same order
        assert n <= 3 or a != loader.scene_indices(3)                                        # another epoch: a different one
        loader.set_epoch(2)
        assert loader.scene_indices() == a and len(loader) == num // spg


@pytest.mark.parametrize("n,world,spg", [(16, 2, 4), (701, 8, 8), (701, 2, 3), (11, 8, 2)])
def test_training_order_with_split_stays_in_the_shard(n, world, spg):
    bounds = parallel.shard_bounds(n, world)
    num = max(-(-int(bounds[r + 1] - bounds[r]) // spg) for r in range(world)) * spg
    for rank in range(world):
        loader = build_dataloader(_Scenes(n), spg, shuffle=True, split_data=True, seed=1, rank=rank, world_size=world)
        a, b = loader.scene_indices(0), loader.scene_indices(1)
        shard = list(parallel.shard_scenes(n, rank, world))
        assert len(a) == num and set(a) == set(shard) and set(b) == set(shard)               # every rank the same length, never outside its shard
        assert a[len(shard):] == (a[:len(shard)] * (num // len(shard) + 1))[:num - len(shard)]    # padding wraps from the front
        assert sorted(a[:len(shard)]) == shard and (a != b or len(shard) < 3)
        assert a == loader.scene_indices(0)


def test_one_rank_ignores_split_data():
    a = build_dataloader(_Scenes(16), 4, shuffle=True, split_data=True, rank=0, world_size=1).scene_indices(0)
    assert a == build_dataloader(_Scenes(16), 4, shuffle=True, rank=0, world_size=1).scene_indices(0) and sorted(a) == list(range(16))


# ---------------------------------------------------------------------------------------------- pixel cache
def test_pixel_cache_round_trip_and_rebuild_on_a_changed_path_list(in_golden, tmp_path, fixture):
    cache = str(tmp_path / "pixels.npy")
    ds = D.ShapeNetSRN(PREFIX, pixel_cache_path=cache)
    plain = D.ShapeNetSRN(PREFIX).load_pixels()
    assert plain.dtype == np.uint8 and plain.shape == (16, 8, 8, 3) and ds.image_offsets == [0, 6, 10, 16]
    for i, path in enumerate(ds.image_paths):
        assert np.array_equal(plain[i], fixture["pixels/" + path][:, :, :3])
    first = ds.load_pixels()
    assert isinstance(first, np.memmap) and np.array_equal(first, plain) and np.array_equal(np.load(cache), plain)
    stamp = os.stat(cache).st_mtime_ns
    reads = []
    real = D.read_image
    try:
        D.read_image = lambda p: reads.append(p) or real(p)
        again = D.ShapeNetSRN(PREFIX, pixel_cache_path=cache).load_pixels()                   # second start: memory-mapped, nothing decoded
        assert reads == [] and isinstance(again, np.memmap) and np.array_equal(again, plain) and os.stat(cache).st_mtime_ns == stamp
        fewer = D.ShapeNetSRN(PREFIX, pixel_cache_path=cache, step=2)                        # another path list: rebuilt
        got = fewer.load_pixels()
        assert len(reads) == 12 and got.shape == (12, 8, 8, 3) and np.array_equal(got, np.concatenate([plain[:6], plain[10:]]))
        assert np.load(cache).shape == (12, 8, 8, 3)
    finally:
        D.read_image = real


def test_scene_store_has_no_cpu_path(in_golden, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        D.SceneStore(np.zeros((1, 2, 2, 3), np.uint8))
    with pytest.raises(RuntimeError, match="HIP device"):
        next(iter(build_dataloader(D.ShapeNetSRN(PREFIX, step=2), 2)))


def test_scenes_of_a_batch_with_different_view_counts_raise(in_golden):
    with pytest.raises(ValueError, match="different numbers of cond views"):
        next(iter(build_dataloader(D.ShapeNetSRN(PREFIX), 2)))                                # alpha_01 has 6 views, mid_02 has 4
