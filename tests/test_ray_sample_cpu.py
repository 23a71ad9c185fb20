"""What a machine without a GPU can check of the store-backed ray sampling: the dense ``Conditioning`` / ``RayBatcher`` path still gives, on CPU
tensors, exactly what its three indexed gathers gave before it learned about ``datasets.StoredViews``; the new entry point is declared in the
header with as many parameters as the ctypes binding passes; the handle and the loader refuse what they cannot do before they touch a device."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays(S=2, V=3, h=5, w=7, seed=0):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.rand(S, V, h, w, 3, generator=g) for _ in range(3))


def _plain_take(images, rays_o, rays_d, inds):
    """the three advanced-index gathers, restated: (rays_o, rays_d, images)[s, inds[s, r]] over the flattened pixels"""
    S, P = images.size(0), images.shape[1:4].numel()
    rows = torch.arange(S)[:, None]
    return tuple(t.reshape(S, P, 3)[rows, inds] for t in (rays_o, rays_d, images))


def _equal(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("rays_per_step", [32, 35])                      # 105 pixels: three chunks and a tail of 9; three chunks exactly
def test_dense_ray_batcher_on_cpu_tensors_is_the_three_indexed_gathers(rays_per_step):
    from ssdnerf_amd.fitting import Conditioning, RayBatcher
    images, rays_o, rays_d = _arrays()
    cond = Conditioning(images, rays_o, rays_d, torch.tensor([0.1, 0.2]))
    assert cond.stored is None and cond.images is images and cond.rays_o is rays_o and cond.rays_d is rays_d
    assert cond.ray_args() == (images, rays_o, rays_d)
    assert (cond.num_scenes, cond.pixels_per_scene, cond.device) == (2, 105, torch.device("cpu"))
    # fixed=True: one permutation per scene, drawn at construction, cut into chunks of rays_per_step, cycled
    torch.manual_seed(11)
    batcher = RayBatcher(cond, rays_per_step, fixed=True)
    torch.manual_seed(11)
    perms = torch.stack([torch.randperm(105) for _ in range(2)], dim=0)
    chunks = perms.split(rays_per_step, dim=1)
    assert len(batcher.chunks) == len(chunks) and all(torch.equal(a, b) for a, b in zip(batcher.chunks, chunks))
    for k in range(len(chunks) + 2):
        assert torch.equal(batcher.indices(k), chunks[k % len(chunks)])
        assert _equal(batcher.batch(k), _plain_take(images, rays_o, rays_d, chunks[k % len(chunks)])), k
    # fixed=False: nothing drawn at construction, a fresh subset per take
    torch.manual_seed(12)
    batcher = RayBatcher(cond, rays_per_step, fixed=False)
    got = [batcher.take(None), batcher.take(None)]
    torch.manual_seed(12)
    for g in got:
        inds = torch.stack([torch.randperm(105)[:rays_per_step] for _ in range(2)], dim=0)
        assert _equal(g, _plain_take(images, rays_o, rays_d, inds))
    assert batcher.chunks is None and batcher.indices(0) is None
    given = torch.tensor([[0, 104, 7, 7], [3, 2, 1, 0]])
    assert _equal(batcher.take(given), _plain_take(images, rays_o, rays_d, given))


def test_dense_ray_batcher_hands_out_the_flat_arrays_when_the_views_are_small():
    from ssdnerf_amd.fitting import Conditioning, RayBatcher
    from ssdnerf_amd.models import BaseNeRF
    images, rays_o, rays_d = _arrays(seed=1)
    cond = Conditioning(images, rays_o, rays_d, None)
    for rays_per_step in (105, 4096):
        state = torch.get_rng_state()
        batcher = RayBatcher(cond, rays_per_step, fixed=True)
        assert batcher.chunks is None and torch.equal(torch.get_rng_state(), state)                       # nothing is drawn
        for got in (batcher.batch(2), batcher.take(None)):
            assert _equal(got, (rays_o.reshape(2, 105, 3), rays_d.reshape(2, 105, 3), images.reshape(2, 105, 3)))
    # the reference-shaped entry points on top of it
    torch.manual_seed(4)
    got = BaseNeRF.ray_sample(rays_o, rays_d, images, n_samples=16)
    torch.manual_seed(4)
    inds = torch.stack([torch.randperm(105)[:16] for _ in range(2)], dim=0)
    assert _equal(got, _plain_take(images, rays_o, rays_d, inds))
    torch.manual_seed(5)
    chunks, n = BaseNeRF.get_raybatch_inds(images, 50)
    torch.manual_seed(5)
    want = torch.stack([torch.randperm(105) for _ in range(2)], dim=0).split(50, dim=1)
    assert n == 3 and all(torch.equal(a, b) for a, b in zip(chunks, want))
    assert BaseNeRF.get_raybatch_inds(images, 105) == (None, None)


def test_a_handle_takes_no_ray_arrays_beside_it():
    from ssdnerf_amd import datasets as D
    from ssdnerf_amd.fitting import Conditioning
    views = D.StoredViews.__new__(D.StoredViews)                         # (a real one needs a device store)
    with pytest.raises(ValueError, match="rays_o = rays_d = None"):
        Conditioning(views, torch.zeros(1), None, None)
    assert Conditioning(views, None, None, None).stored is views


def _c_parameters(declaration: str):
    inside = declaration[declaration.index("(") + 1:declaration.rindex(")")]
    return [p.strip() for p in re.sub(r"/\*.*?\*/", "", inside, flags=re.S).split(",")]


def test_the_entry_point_is_declared_and_bound_with_the_same_parameters(monkeypatch):
    import ctypes
    from ssdnerf_amd import _cabi as C
    with open(os.path.join(ROOT, "include", "ssdnerf_hip.h")) as f:
        header = f.read()
    found = re.findall(r"^int ssdnerf_sample_rays_u8\([^;]*\);", header, flags=re.M)
    assert len(found) == 1, found
    params = _c_parameters(found[0])
    assert "ssdnerf_sample_rays_u8" in C.EXPORTS
    with open(os.path.join(ROOT, "ssdnerf_amd", "csrc", "scene_store.hip")) as f:
        source = f.read()
    defined = re.findall(r'^extern "C" int ssdnerf_sample_rays_u8\([^{]*\)\s*\{', source, flags=re.M)
    assert len(defined) == 1 and [p.split()[-1] for p in _c_parameters(defined[0])] == [p.split()[-1] for p in params]

    class Fn:                                                            # what ctypes.CDLL hands out, without a library to load
        argtypes = restype = None

    class Lib:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, name):
            return self.__dict__["fns"].setdefault(name, Fn())

    fake = Lib()
    fake.fns["ssdnerf_abi_version"] = lambda: C.ABI_VERSION
    monkeypatch.setattr(C, "_lib", None)
    monkeypatch.setattr(C.os.path, "exists", lambda p: True)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: fake)
    C.lib()
    argtypes = fake.fns["ssdnerf_sample_rays_u8"].argtypes
    assert argtypes is not None and len(argtypes) == len(params) == 15
    for kind, text in zip(argtypes, params):
        want = ctypes.c_void_p if "*" in text else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[text.split()[0]]
        assert kind is want, (text, kind)


def test_stored_conditioning_views_need_the_device_store():
    from ssdnerf_amd import datasets as D
    golden = os.path.join(ROOT, "tests", "golden", "srn_tiny", "cars")
    ds = D.ShapeNetSRN(golden, num_train_imgs=3, load_test_data=False)
    with pytest.raises(ValueError, match="host memory"):
        D.build_dataloader(ds, 2, store="host", cond_imgs="stored")
    with pytest.raises(ValueError, match="'dense' or 'stored'"):
        D.build_dataloader(ds, 2, cond_imgs="sparse")
    loader = D.build_dataloader(ds, 2, cond_imgs="stored")               # building it needs no device; scene_indices() neither
    assert loader.cond_imgs == "stored" and D.build_dataloader(ds, 2).cond_imgs == "dense" and loader.scene_indices() == [0, 1, 2]
    with pytest.raises(ValueError, match="store='device'"):
        D.StoredViews(object(), np.zeros((1, 1), np.int64), torch.zeros(1, 1, 4, 4), torch.zeros(1, 1, 4))
