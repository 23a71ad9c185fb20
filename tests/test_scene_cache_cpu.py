"""The device-resident scene cache without a GPU: the conversions of csrc/cache_cvt.h (a gcc build, tests/host/cache_host.c) against torch's
``_clamp_to(x, dtype).to(dtype)`` bit for bit over every 16-bit pattern, every rounding tie and its neighbours; the refusals of the C ABI; the
host logic of ``MultiSceneNeRF(cache_store=...)`` and ``scene_cache.DeviceSceneCache``."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _cache_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host") / "cache_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "cache_host.c"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for name in ("f32_to_f16_clamped", "f32_to_bf16_clamped", "f16_to_f32", "bf16_to_f32"):
        getattr(lib, name).restype = None
        getattr(lib, name).argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
    return lib


def _run(fn, x, out_dtype):
    x = np.ascontiguousarray(x)
    y = np.empty(x.shape, out_dtype)
    fn(x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), x.size)
    return y


@pytest.mark.parametrize("dtype,narrow,widen", [(torch.float16, "f32_to_f16_clamped", "f16_to_f32"), (torch.bfloat16, "f32_to_bf16_clamped", "bf16_to_f32")])
def test_header_conversions_equal_torch_bit_for_bit(host, dtype, narrow, widen):
    x = R.inputs(dtype)
    n_pairs = (0x7C00 if dtype == torch.float16 else 0x7F80) - 1           # neighbouring finite values of one sign, zero included
    assert x.size == 65536 + 6 * n_pairs + R.SPECIALS.size
    want = R.expected(x, dtype)
    got = _run(getattr(host, narrow), x, np.uint16)
    R.assert_same_bits(got, want, dtype, narrow)
    # every finite pattern comes back as itself through widen -> narrow, and the widening is torch's
    every = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    wide = _run(getattr(host, widen), every, np.uint32)
    torch_wide = torch.from_numpy(every.view(np.int16).copy()).view(dtype).float().numpy().view(np.uint32)
    finite = np.isfinite(torch_wide.view(np.float32))
    nan = np.isnan(torch_wide.view(np.float32))
    assert np.array_equal(wide[~nan], torch_wide[~nan]) and np.isnan(wide.view(np.float32)[nan]).all()
    back = _run(getattr(host, narrow), wide, np.uint16)
    assert np.array_equal(back[finite], every[finite])
    inf = ~finite & ~nan
    top = 0x7BFF if dtype == torch.float16 else 0x7F7F
    assert set(back[inf].tolist()) == {top, top | 0x8000}                  # +-Inf is clamped to +-max


def test_the_specials_one_by_one(host):
    f = lambda v: np.array([v], dtype=np.float32).view(np.uint32)
    h = lambda v: int(_run(host.f32_to_f16_clamped, f(v), np.uint16)[0])
    b = lambda v: int(_run(host.f32_to_bf16_clamped, f(v), np.uint16)[0])
    assert h(np.inf) == 0x7BFF and h(-np.inf) == 0xFBFF and b(np.inf) == 0x7F7F and b(-np.inf) == 0xFF7F
    assert h(3.4028234663852886e38) == 0x7BFF and b(3.4028234663852886e38) == 0x7F7F and b(-3.4028234663852886e38) == 0xFF7F
    assert h(65504.0) == h(65519.9) == h(65520.0) == h(70000.0) == 0x7BFF
    assert h(0.0) == 0 and h(-0.0) == 0x8000 and b(0.0) == 0 and b(-0.0) == 0x8000
    assert h(2.0 ** -24) == 1 and h(2.0 ** -25) == 0 and h(-2.0 ** -25) == 0x8000 and h(1e-10) == 0       # the smallest subnormal; a tie to zero
    assert h(np.float32(2.0 ** -25) * np.float32(1.0000001)) == 1 and h(1.5 * 2.0 ** -24) == 2            # just above the tie; a tie to even
    assert h(2.0 ** -14) == 0x0400 and h(2.0 ** -14 - 2.0 ** -25) == 0x0400                               # rounding up into the smallest normal
    assert (h(np.nan) & 0x7C00) == 0x7C00 and (h(np.nan) & 0x3FF) != 0 and (b(np.nan) & 0x7F80) == 0x7F80 and (b(np.nan) & 0x7F) != 0
    assert b(2.0 ** -133) == 0x0001 and b(2.0 ** -134) == 0 and b(1.5 * 2.0 ** -133) == 0x0002            # bf16 subnormals


# ---------------------------------------------------------------------------------------------- the C ABI, without a device
def test_abi_declarations_and_capacity():
    from ssdnerf_amd import _cabi as C, build, scene_cache
    header = open(os.path.join(ROOT, "include", "ssdnerf_hip.h")).read()
    assert f"#define SSDNERF_CACHE_MAX_SCENES {scene_cache.CACHE_CAPACITY}\n" in header
    assert "scene_cache.hip" in build.SOURCES and "cache_cvt.h" in build.HEADERS
    for name in ("ssdnerf_cache_load_multi", "ssdnerf_cache_store_multi", "ssdnerf_cache_max_scenes"):
        assert name in C.EXPORTS and f" {name}(" in header
    assert C.lib().ssdnerf_cache_max_scenes() == scene_cache.CACHE_CAPACITY == 32
    assert ctypes.sizeof(C.CacheRow) == 16 and ctypes.sizeof(C.CacheStore) == 5 * 8 + 4 * 8 + 2 * 4


def test_library_refuses_bad_calls_before_any_hip_call():
    """no device needed: the pointers below are never dereferenced"""
    from ssdnerf_amd import _cabi as C
    lib = C.lib()
    N = 40

    def call(fn, rows, S=None, store=None, bufs=(4096, 8192, 12288, 16384, 20480), **desc):
        d = dict(code=256, exp_avg=512, exp_avg_sq=768, density_grid=1024, density_bitfield=1280, slots=N, numel=7, grid_bytes=2, bits_bytes=1,
                 code_dtype=0, moment_dtype=0)
        d.update(desc)
        st = C.CacheStore(**d)
        tab = (C.CacheRow * max(len(rows), 1))()
        for e, (slot, row, has_state) in zip(tab, rows):
            e.slot, e.row, e.has_state = slot, row, has_state
        rc = fn(st if store is None else store, tab, len(rows) if S is None else S, *bufs, None)
        return rc, lib.ssdnerf_last_error().decode()

    ok = [(5, 0, 1), (3, 1, 0)]
    for fn, name in ((lib.ssdnerf_cache_load_multi, "cache_load_multi"), (lib.ssdnerf_cache_store_multi, "cache_store_multi")):
        cases = [
            (dict(rows=ok, S=0), "S == 0"),
            (dict(rows=[(k, k, 0) for k in range(33)]), "at most"),
            (dict(rows=[(N, 0, 0)]), f"slot {N} of {N}"),
            (dict(rows=[(1, 2, 0), (2, 0, 0)]), "batch row 2 of 2"),
            (dict(rows=ok, numel=0), "zero size"), (dict(rows=ok, grid_bytes=0), "zero size"), (dict(rows=ok, bits_bytes=0), "zero size"),
            (dict(rows=ok, slots=0), "zero size"),
            (dict(rows=ok, code=0), "null pointer"), (dict(rows=ok, exp_avg_sq=0), "null pointer"), (dict(rows=ok, density_bitfield=0), "null pointer"),
            (dict(rows=ok, bufs=(0, 8192, 12288, 16384, 20480)), "null pointer"), (dict(rows=ok, bufs=(4096, 8192, 12288, 0, 20480)), "null pointer"),
            (dict(rows=ok, bufs=(4096, 8192, 12288, 16384, 0)), "null pointer"),
            (dict(rows=ok, bufs=(4096, 0, 12288, 16384, 20480)), "null pointer (m or v)"),            # entry 0 has has_state set
            (dict(rows=ok, bufs=(4098, 8192, 12288, 16384, 20480)), "4-byte aligned"),
            (dict(rows=ok, code=258), "aligned"), (dict(rows=ok, code=257, code_dtype=1, moment_dtype=2), "aligned"),
            (dict(rows=[(5, 0, 2)]), "has_state"),
        ]
        for pair in [(a, b) for a in range(-1, 4) for b in range(-1, 4) if (a, b) not in ((0, 0), (1, 2))]:
            cases.append((dict(rows=ok, code_dtype=pair[0], moment_dtype=pair[1]), "dtype pair"))
        for kw, cause in cases:
            rc, msg = call(fn, **kw)
            assert rc == -1 and msg.startswith(name) and cause in msg, (name, kw, msg)
        st = C.CacheStore(256, 512, 768, 1024, 1280, N, 7, 2, 1, 0, 0)
        tab = (C.CacheRow * 1)()
        assert fn(None, tab, 1, 4096, 8192, 12288, 16384, 20480, None) == -1 and "null pointer" in lib.ssdnerf_last_error().decode()
        assert fn(st, None, 1, 4096, 8192, 12288, 16384, 20480, None) == -1 and "null pointer" in lib.ssdnerf_last_error().decode()
    # what only one direction refuses: the same slot twice on store (two rows race for it), the same batch row twice on load
    rc, msg = call(lib.ssdnerf_cache_store_multi, [(5, 0, 0), (3, 1, 0), (5, 2, 0)])
    assert rc == -1 and "slot 5 twice" in msg
    rc, msg = call(lib.ssdnerf_cache_load_multi, [(5, 0, 0), (3, 0, 0)])
    assert rc == -1 and "batch row 0 twice" in msg


# ---------------------------------------------------------------------------------------------- host logic on a CPU model
def _model(**kw):
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.registry import MODELS
    return MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 2, 5, 7), code_activation=dict(type="TanhCode", scale=2), grid_size=16,
                             decoder=dict(type="TriPlaneDecoder", base_layers=[6, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64]),
                             train_cfg=dict(optimizer=dict(type="Adam", lr=0.01)), **kw))


def test_cache_store_argument():
    import ssdnerf_amd
    from ssdnerf_amd.scene_cache import DeviceSceneCache
    assert ssdnerf_amd.DeviceSceneCache is DeviceSceneCache
    with pytest.raises(ValueError, match="cache_size"):
        _model(cache_store="device")
    with pytest.raises(ValueError, match="cache_size"):
        _model(cache_store="device", cache_size=0)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        _model(cache_store="pinned", cache_size=3)
    m = _model(cache_store="device", cache_size=5, cache_16bit=True)
    assert isinstance(m.cache, DeviceSceneCache) and sorted(m.cache) == [0, 1, 2, 3, 4] and len(m.cache) == 5
    assert m.cache.code_ is None and m.cache[3] is None and m.cache.host_copies == 0                  # nothing is allocated before the first use
    assert (m.cache.code_dtype, m.cache.state_dtype) == (torch.float16, torch.bfloat16)
    with pytest.raises(TypeError):
        m.cache[3] = {}                                                                               # read-only
    data = dict(scene_id=[1, 3], scene_name=["a", "b"])
    with pytest.raises(ValueError, match="no CPU path"):
        m.load_cache(data)
    leaves = [torch.zeros(3, 2, 5, 7, requires_grad=True) for _ in range(2)]
    opts = m.build_optimizer(leaves, m.train_cfg)
    with pytest.raises(ValueError, match="no CPU path"):
        m.save_cache(leaves, opts, m.get_init_density_grid(2), m.get_init_density_bitfield(2), data["scene_id"], data["scene_name"])


def test_host_mode_is_the_dict_cache_as_before():
    for kw in (dict(), dict(cache_store="host")):
        m = _model(cache_size=4, **kw)
        assert m.cache_store == "host" and type(m.cache) is dict and sorted(m.cache) == [0, 1, 2, 3] and all(v is None for v in m.cache.values())
        data = dict(scene_id=[2, 0], scene_name=["s2", "s0"])
        torch.manual_seed(3)
        codes, opts, grid, bits = m.load_cache(data)
        for c, o in zip(codes, opts):
            o.zero_grad(); (c ** 2).sum().backward(); o.step()
        m.save_cache(codes, opts, grid, bits, data["scene_id"], data["scene_name"])
        e = m.cache[2]
        assert type(e) is dict and set(e) == {"scene_id", "scene_name", "param", "optimizer"} and m.cache[1] is None
        assert torch.equal(e["param"]["code_"], codes[0].detach()) and e["param"]["code_"].dtype == torch.float32
        assert float(e["optimizer"]["state"][0]["step"]) == 1.0
    assert _model().cache is None and _model().cache_store == "host"


def test_slots_follow_the_shard_and_duplicate_rows_are_dropped():
    from ssdnerf_amd.parallel import shard_scenes
    from ssdnerf_amd.scene_cache import DeviceSceneCache, last_occurrences
    shard = shard_scenes(11, 1, 3)
    assert len(shard) in (3, 4) and shard[0] > 0
    cache = DeviceSceneCache(shard, (3, 2, 5, 7), 16, cache_16bit=False)
    assert list(cache) == list(shard) and cache.slots(list(shard)) == list(range(len(shard))) and cache.slot_of[shard[1]] == 1
    assert (cache.numel, cache.grid_bytes, cache.bits_bytes) == (210, 2 * 16 ** 3, 16 ** 3 // 8)
    with pytest.raises(KeyError):
        cache[shard[-1] + 1]
    assert last_occurrences([4, 7, 4, 9, 7, 7]) == [2, 3, 5]
    assert last_occurrences([torch.tensor(1), torch.tensor(0)]) == [0, 1]
    assert last_occurrences([]) == []
