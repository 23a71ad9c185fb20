"""The device layers of ssdnerf_amd/datasets.py: ``ssdnerf_gather_views_u8`` (csrc/scene_store.hip) bit for bit against numpy's
``store[idx].astype(np.float32) / 255``, ``SceneStore`` in both placements, ``SceneLoader``'s batches against what the reference's own
``parse_scene`` returned on the fixture tree (tests/golden/srn_tiny.npz), and one stage-1 ``train_step`` / ``val_step`` on a loader batch.
Every test fails at import without the feature."""
import json
import os
import random

import numpy as np
import pytest
import torch

from ssdnerf_amd import _cabi as C
from ssdnerf_amd import datasets as D
from ssdnerf_amd.config import build_dataloader, build_dataset

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PREFIX = "srn_tiny/cars"
GUARD = 64                                                               # sentinel floats on either side of `out`


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _raw_gather(store_dev, image_bytes, num_images, idx, out_pad=None):
    """one call of the C ABI on a flat uint8 device tensor; `out` sits between two runs of sentinel values, which are checked"""
    n = len(idx)
    index = torch.tensor(idx, dtype=torch.int32).cuda()
    padded = torch.full((2 * GUARD + n * image_bytes,), -7.25, device="cuda") if out_pad is None else out_pad
    out = padded[GUARD:GUARD + n * image_bytes]
    C.check(C.lib().ssdnerf_gather_views_u8(C.ptr(store_dev), image_bytes, num_images, C.ptr(index), n, C.ptr(out), C.stream()), "gather_views_u8")
    torch.cuda.synchronize()
    host = padded.cpu().numpy()
    assert np.all(host[:GUARD] == -7.25) and np.all(host[GUARD + n * image_bytes:] == -7.25), "written outside out"
    return host[GUARD:GUARD + n * image_bytes].reshape(n, image_bytes)


def _store(num_images, image_bytes, seed):
    return np.random.default_rng(seed).integers(0, 256, (num_images, image_bytes), dtype=np.uint8)


def test_all_256_byte_values_equal_numpys_quotient_bit_for_bit():
    """rejects a reciprocal multiply: x * (1 / 255.f) differs from x / 255.f at 126 of the 256 values"""
    values = np.arange(256, dtype=np.uint8)
    want = values.astype(np.float32) / 255
    assert int((_bits(want) != _bits(values.astype(np.float32) * np.float32(1 / 255))).sum()) == 126
    for image_bytes in (256, 1, 3):                                      # the vector path, and two element-path sizes
        store = np.resize(values, (-(-256 // image_bytes), image_bytes))  # (3: 86 images, the values wrap round into the last one)
        got = _raw_gather(torch.from_numpy(store).cuda(), image_bytes, store.shape[0], list(range(store.shape[0])))
        assert np.array_equal(_bits(got.reshape(-1)[:256]), _bits(want)), image_bytes


@pytest.mark.parametrize("hw", [(1, 1), (5, 7), (8, 8), (128, 128)])
@pytest.mark.parametrize("count", [1, 3, 15])
def test_gather_equals_numpy(hw, count):
    image_bytes = hw[0] * hw[1] * 3
    num = 9
    store = _store(num, image_bytes, hw[0] * 100 + count)
    idx = np.random.default_rng(count).integers(0, num, count).tolist()
    dev = torch.from_numpy(store).cuda()
    before = int(dev.sum(dtype=torch.int64))
    got = _raw_gather(dev, image_bytes, num, idx)
    assert np.array_equal(_bits(got), _bits(store[idx].astype(np.float32) / 255))
    assert int(dev.sum(dtype=torch.int64)) == before and np.array_equal(dev.cpu().numpy(), store)          # the store is untouched
    assert np.array_equal(_bits(_raw_gather(dev, image_bytes, num, idx)), _bits(got))                         # two calls: identical bits


def test_gather_of_2008_small_views_walks_the_grid_and_the_image_lookup():
    """8 x 251 views of 8 x 8: 47 blocks of 8192 elements, every one of which spans 42 images and ends inside one"""
    image_bytes, num, count = 192, 300, 8 * 251
    store = _store(num, image_bytes, 5)
    idx = np.random.default_rng(6).integers(0, num, count).tolist()
    got = _raw_gather(torch.from_numpy(store).cuda(), image_bytes, num, idx)
    assert np.array_equal(_bits(got), _bits(store[idx].astype(np.float32) / 255))


@pytest.mark.parametrize("image_bytes", [105, 192])
def test_repeated_reversed_and_equal_indices(image_bytes):
    num = 7
    store = _store(num, image_bytes, image_bytes)
    dev = torch.from_numpy(store).cuda()
    for idx in ([2, 2, 5, 5, 2], list(range(num))[::-1], [4] * 11, [0], [num - 1]):
        got = _raw_gather(dev, image_bytes, num, idx)
        assert np.array_equal(_bits(got), _bits(store[idx].astype(np.float32) / 255)), idx


@pytest.mark.parametrize("image_bytes", [105, 192, 3 * 128 * 128])
def test_store_that_starts_one_byte_into_a_buffer(image_bytes):
    num = 5
    store = _store(num, image_bytes, 11)
    big = torch.zeros(num * image_bytes + 32, dtype=torch.uint8, device="cuda")
    big[1:1 + num * image_bytes] = torch.from_numpy(store.reshape(-1)).cuda()
    view = big[1:1 + num * image_bytes]
    assert view.data_ptr() % 2 == 1
    idx = [4, 0, 3]
    got = _raw_gather(view, image_bytes, num, idx)
    assert np.array_equal(_bits(got), _bits(store[idx].astype(np.float32) / 255))
    assert int(big[0]) == 0 and int(big[1 + num * image_bytes:].sum()) == 0


def test_out_that_is_only_4_byte_aligned_takes_the_element_path():
    image_bytes, num, idx = 192, 4, [3, 1]
    store = _store(num, image_bytes, 12)
    padded = torch.full((2 * GUARD + len(idx) * image_bytes + 1,), -7.25, device="cuda")[1:]
    assert padded.data_ptr() % 16 == 4
    got = _raw_gather(torch.from_numpy(store).cuda(), image_bytes, num, idx, out_pad=padded)
    assert np.array_equal(_bits(got), _bits(store[idx].astype(np.float32) / 255))


def test_argument_errors_surface_as_exceptions():
    lib = C.lib()
    store = torch.zeros(192, dtype=torch.uint8, device="cuda")
    index = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(192, device="cuda")
    null = C.ctypes.c_void_p(0)
    good = [C.ptr(store), 192, 1, C.ptr(index), 1, C.ptr(out), C.stream()]
    for at, value, match in ((0, null, "null pointer"), (3, null, "null pointer"), (5, null, "null pointer"), (4, 0, "count == 0"),
                             (1, 0, "image_bytes == 0"), (4, (1 << 40) // 192 + 1, "2\\^40"), (1, (1 << 40) + 1, "2\\^40")):
        args = list(good)
        args[at] = value
        with pytest.raises(RuntimeError, match=match):
            C.check(lib.ssdnerf_gather_views_u8(*args), "gather_views_u8")
    C.check(lib.ssdnerf_gather_views_u8(*good), "gather_views_u8")
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0


# ---------------------------------------------------------------------------------------------- SceneStore
def test_scene_store_validates_indices_on_the_host():
    pixels = _store(6, 5 * 7 * 3, 3).reshape(6, 5, 7, 3)
    store = D.SceneStore(pixels)
    assert store.pixels.is_cuda and store.pixels.dtype == torch.uint8 and store.offsets == [0, 6]
    for bad in ([0, 6], [-1], [2, 1 << 31], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            store.gather(bad)
    with pytest.raises(ValueError, match="host"):
        store.gather(torch.tensor([0]).cuda())
    got = store.gather(torch.tensor([5, 0]))
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (2, 5, 7, 3)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(pixels[[5, 0]].astype(np.float32) / 255))
    with pytest.raises(ValueError, match="uint8"):
        D.SceneStore(pixels.astype(np.int32))
    with pytest.raises(ValueError, match="store must be"):
        D.SceneStore(pixels, store="disk")


def test_host_store_equals_device_store_over_consecutive_batches_with_one_synchronisation():
    """the staging-reuse case: the second gather refills the staging buffer while the first one's kernel may still be reading it"""
    pixels = _store(40, 64 * 64 * 3, 8).reshape(40, 64, 64, 3)
    dev, host = D.SceneStore(pixels, store="device"), D.SceneStore(pixels, store="host")
    assert host.pixels.is_pinned() and not host.pixels.is_cuda
    first, second, third = list(range(3, 27)), [39, 0, 1, 2, 17, 17, 30, 31], list(range(40))[::-1]
    a = [host.gather(first), host.gather(second), host.gather(third)]                        # the third one grows the staging buffer
    b = [dev.gather(first), dev.gather(second), dev.gather(third)]
    torch.cuda.synchronize()
    for x, y, idx in zip(a, b, (first, second, third)):
        assert torch.equal(x, y)
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(pixels[idx].astype(np.float32) / 255))


def test_host_store_staging_reuse_across_streams():
    """two gathers on two streams: nothing but the event behind the first kernel keeps the second call's copies out of the staging buffer
    while that kernel reads it"""
    pixels = _store(240, 128 * 128 * 3, 9).reshape(240, 128, 128, 3)
    host = D.SceneStore(pixels, store="host")
    first, second = list(range(0, 120)), list(range(239, 119, -1))
    side = torch.cuda.Stream()
    a = host.gather(first)
    with torch.cuda.stream(side):
        b = host.gather(second)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(pixels[first].astype(np.float32) / 255))
    assert np.array_equal(_bits(b.cpu().numpy()), _bits(pixels[second].astype(np.float32) / 255))


# ---------------------------------------------------------------------------------------------- SceneLoader
@pytest.fixture(scope="module")
def fixture():
    z = np.load(os.path.join(GOLDEN, "srn_tiny.npz"))
    return {k: z[k] for k in z.files}


@pytest.fixture()
def in_golden(monkeypatch):
    monkeypatch.chdir(GOLDEN)


def _check_batch(batch, fixture, name, scenes):
    keys = fixture[f"{name}/{scenes[0]}/__keys__"].tolist()
    assert sorted(batch) == keys, (sorted(batch), keys)
    for key in keys:
        rec = [fixture[f"{name}/{i}/{key}"] for i in scenes]
        if key in ("scene_id", "scene_name"):
            assert batch[key] == [r.item() for r in rec] and all(type(v) in (int, str) for v in batch[key])
        elif key.endswith("_img_paths"):
            assert batch[key] == [r.tolist() for r in rec]
        else:
            t = batch[key]
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), key
            want = np.stack(rec)
            assert tuple(t.shape) == want.shape, (key, tuple(t.shape), want.shape)
            assert np.array_equal(_bits(t.cpu().numpy()), _bits(want)), key


@pytest.mark.parametrize("store", ["device", "host"])
def test_loader_batches_equal_the_reference_scenes_stacked(fixture, in_golden, store):
    sets = json.loads(str(fixture["sets_json"]))
    # val_cond (2 scenes of 6 views: 2 conditioning, 4 test) in one batch, and one scene per batch
    ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **sets["val_cond"]))
    batches = list(build_dataloader(ds, 2, store=store))
    assert len(batches) == 1 and tuple(batches[0]["cond_imgs"].shape) == (2, 2, 8, 8, 3) and tuple(batches[0]["test_imgs"].shape) == (2, 4, 8, 8, 3)
    assert tuple(batches[0]["cond_poses"].shape) == (2, 2, 4, 4) and tuple(batches[0]["cond_intrinsics"].shape) == (2, 2, 4)
    _check_batch(batches[0], fixture, "val_cond", [0, 1])
    # train: all views are conditioning views; the scenes have 6, 4 and 6 of them, so one scene per batch (ragged counts in one batch raise)
    ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **sets["train"]))
    batches = list(build_dataloader(ds, 1, store=store))
    assert len(batches) == 3
    for i, batch in enumerate(batches):
        _check_batch(batch, fixture, "train", [i])
    with pytest.raises(ValueError, match="different numbers of cond views"):
        list(build_dataloader(ds, 2, store=store))
    # test_pose_override: the override's 3 poses replace every scene's test poses (the scenes keep their 5, 3 and 5 test images)
    ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **sets["val_cond_override"]))
    loader = build_dataloader(ds, 1, store=store)
    batches = list(loader)
    assert [b["scene_id"] for b in batches] == [[0], [1], [2]]
    assert tuple(batches[1]["test_poses"].shape) == (1, 3, 4, 4) and tuple(batches[1]["test_imgs"].shape) == (1, 3, 8, 8, 3)
    for i, batch in enumerate(batches):
        _check_batch(batch, fixture, "val_cond_override", [i])
    _check_batch(loader.batch([2, 0]), fixture, "val_cond_override", [2, 0])
    with pytest.raises(ValueError, match="different numbers of test views"):
        loader.batch([0, 1])
    # a ragged last batch, not padded
    ds = D.ShapeNetSRN(PREFIX, num_train_imgs=3, load_test_data=False)
    batches = list(build_dataloader(ds, 2, store=store))
    assert [b["scene_id"] for b in batches] == [[0, 1], [2]] and [tuple(b["cond_imgs"].shape) for b in batches] == [(2, 3, 8, 8, 3), (1, 3, 8, 8, 3)]
    for key in ("cond_imgs", "cond_poses", "cond_intrinsics"):
        want = np.stack([fixture[f"num_train_3/{i}/{key}"] for i in (0, 1)])
        assert np.array_equal(_bits(batches[0][key].cpu().numpy()), _bits(want)), key


def test_loader_without_images_and_with_codes(fixture, in_golden, tmp_path):
    sets = json.loads(str(fixture["sets_json"]))
    ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **sets["val_uncond"]))
    loader = build_dataloader(ds, 2)
    batch = next(iter(loader))
    _check_batch(batch, fixture, "val_uncond", [0, 1])
    assert loader._store is None and "test_imgs" not in batch                                 # load_imgs=False: no store is built
    for name in ("alpha_01", "zeta_03"):
        torch.save(dict(param=dict(code_=torch.zeros(2))), tmp_path / (name + ".pth"))
    ds = D.ShapeNetSRN(PREFIX, code_dir=str(tmp_path), code_only=True)
    loader = build_dataloader(ds, 2)
    assert "code" not in loader.batch([0, 1]) and [sorted(c) for c in loader.batch([0, 2])["code"]] == [["param"], ["param"]]


def test_random_test_views_follow_the_reference_draws(fixture, in_golden):
    sets = json.loads(str(fixture["sets_json"]))
    random.seed(0)
    ds = build_dataset(dict(type="ShapeNetSRN", data_prefix=PREFIX, **sets["random_test"]))
    for i, batch in enumerate(build_dataloader(ds, 1)):
        _check_batch(batch, fixture, "random_test", [i])


# ---------------------------------------------------------------------------------------------- end to end
def test_stage1_train_step_and_val_step_run_on_a_loader_batch(in_golden):
    """Only that the loader's batch is what the model's steps take, unchanged, and that what they log is finite."""
    import test_tv_loss_gpu as TV
    train_cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=1, n_inverse_rays=2 ** 8, n_decoder_rays=2 ** 8,
                     loss_coef=0.1 / (8 * 8), optimizer=dict(type="Adam", lr=1e-2, weight_decay=0.))
    test_cfg = dict(density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 8, loss_coef=0.1 / (8 * 8), n_inverse_steps=2,
                    optimizer=dict(type="Adam", lr=0.08, weight_decay=0.), lr_scheduler=dict(type="ExponentialLR", gamma=0.998))
    m = TV._stage1_model(train_cfg=train_cfg, test_cfg=test_cfg).train()
    ds = D.ShapeNetSRN(PREFIX, step=2, num_test_imgs=2)                                       # alpha_01 and zeta_03: 4 conditioning + 2 test views
    batch = next(iter(build_dataloader(ds, 2)))
    assert batch["scene_id"] == [0, 1] and tuple(batch["cond_imgs"].shape) == (2, 4, 8, 8, 3) and tuple(batch["test_imgs"].shape) == (2, 2, 8, 8, 3)
    opt = dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    torch.manual_seed(1)
    out = m.train_step(batch, opt)
    assert out["num_samples"] == 2 and bool(torch.isfinite(torch.as_tensor(out["log_vars"]["loss"]).float()).all())
    lv = m.eval().val_step(batch)["log_vars"]
    assert np.isfinite(lv["test_psnr"]) and np.isfinite(lv["test_ssim"]), lv
