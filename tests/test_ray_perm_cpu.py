"""CPU tests of the device-side pixel permutation (csrc/keyed_perm.h): the gcc build of the header against the numpy restatement
of its comment (tests/_perm_ref.py) bit for bit, bijection, the statistics of the leading positions over many draws -- which a network cut to 4 rounds
must fail -- the separation of scenes, draws and seeds, and the host layer's defaults and refusals (``fitting.RayBatcher(index_source=...)``,
``cfg['ray_index_source']``).  The kernels themselves are held to the same restatement in tests/test_ray_perm_gpu.py."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import _perm_ref as KP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = (1, 2, 3, 4, 5, 12, 16, 50, 64, 96, 4097, 16384)                        # every position
LARGE = (819200, 2 ** 31 + 11)                                                 # the first and last 4096 positions
KEYS = ((0, 0, 0), (1234, 2, 0), (0xFEDCBA9876543210, 7, 3), (2 ** 64 - 1, 2 ** 32 - 1, 2 ** 32 - 1))       # (seed, scene, draw)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host") / "keyed_perm_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "keyed_perm_host.c"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.perm_rounds.restype = lib.perm_half_bits.restype = ctypes.c_uint32
    lib.perm_half_bits.argtypes = [ctypes.c_uint64]
    lib.perm_round_keys.restype = lib.perm_range.restype = lib.perm_draws.restype = None
    lib.perm_round_keys.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p]
    lib.perm_range.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p,
                               ctypes.c_void_p]
    lib.perm_draws.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def _host_range(host, seed, scene, draw, P, start, n):
    out, evals = np.full(n, -1, np.int64), np.zeros(n, np.uint32)
    host.perm_range(seed, scene, draw, P, start, n, out.ctypes.data, evals.ctypes.data)
    return out, evals


def test_gcc_build_of_keyed_perm_h_equals_the_restatement(host):
    assert host.perm_rounds() == KP.ROUNDS
    for P in SMALL + LARGE + (2 ** 32 - 1, 17, 256, 257, 65536, 65537):
        assert host.perm_half_bits(P) == KP.half_bits(P), P
    for seed, scene, draw in KEYS:
        keys = np.zeros(KP.ROUNDS, np.uint32)
        host.perm_round_keys(seed, scene, draw, keys.ctypes.data)
        assert np.array_equal(keys, KP.round_keys(seed, scene, draw))
        for P in SMALL:
            got, evals = _host_range(host, seed, scene, draw, P, 0, P)
            want, want_evals = KP.walk(KP.round_keys(seed, scene, draw), P, np.arange(P, dtype=np.uint32))
            assert np.array_equal(got, want) and np.array_equal(evals, want_evals), (P, seed, scene, draw)
        for P in LARGE:
            for start in (0, P - 4096):
                got, _ = _host_range(host, seed, scene, draw, P, start, 4096)
                assert np.array_equal(got, KP.perm_range(seed, scene, draw, P, start, 4096)), (P, start, seed, scene, draw)
                assert got.min() >= 0 and got.max() < P


def test_every_value_once(host):
    for seed, scene, draw in KEYS:
        for P in SMALL:
            assert np.array_equal(np.sort(KP.perm_range(seed, scene, draw, P)), np.arange(P)), (P, seed, scene, draw)
            assert np.array_equal(np.sort(_host_range(host, seed, scene, draw, P, 0, P)[0]), np.arange(P))
    assert KP.perm_range(5, 0, 0, 1).tolist() == [0]


def test_the_walk_stays_under_its_bound(host):
    """all P walks together pass through the network at most 2^b times (once per element of the domain), and 2^b < 4 P"""
    for P in SMALL + (819200,):
        _, evals = _host_range(host, 42, 1, 0, P, 0, P)
        domain = 4 ** KP.half_bits(P)
        assert evals.min() >= 1 and int(evals.sum()) <= domain < 4 * max(P, 2), (P, int(evals.sum()), domain)


# ------------------------------------------------------------------------------------------------ statistics
# a sum of chi-square terms with df degrees of freedom has mean df and variance 2 df: the threshold is df + 6 sqrt(2 df)
def _threshold(df):
    return df + 6 * math.sqrt(2 * df)


def _marginals_chi2(draws):
    """P = 50: the values of pi(0) .. pi(7) over the draws, eight chi-squares of 49 degrees of freedom each, summed"""
    n = draws.shape[0]
    return sum(float((((np.bincount(draws[:, k], minlength=50) - n / 50) ** 2) / (n / 50)).sum()) for k in range(8))


def _pairs_chi2(draws):
    """P = 12: (pi(0), pi(1)) over the 132 ordered pairs of different values -> (chi-square of 131 degrees of freedom, the count on the diagonal)"""
    counts = np.zeros((12, 12))
    np.add.at(counts, (draws[:, 0], draws[:, 1]), 1)
    off, expect = counts[~np.eye(12, dtype=bool)], draws.shape[0] / 132
    return float((((off - expect) ** 2) / expect).sum()), int(np.trace(counts))


def test_marginals_of_the_leading_positions_are_uniform(host):
    got = np.zeros((64000, 8), np.int64)
    host.perm_draws(99, 0, 0, 64000, 50, 8, got.ctypes.data)
    assert np.array_equal(got, KP.perm_draws(99, 0, 0, 64000, 50, 8))
    chi2, df = _marginals_chi2(got), 8 * 49
    print(f"marginals: chi2 = {chi2:.1f}, df = {df}, threshold = {_threshold(df):.1f}")
    assert chi2 < _threshold(df)


def test_pairs_of_the_leading_positions_are_uniform_and_four_rounds_are_not(host):
    got = np.zeros((132000, 2), np.int64)
    host.perm_draws(1234, 0, 0, 132000, 12, 2, got.ctypes.data)
    assert np.array_equal(got, KP.perm_draws(1234, 0, 0, 132000, 12, 2))
    chi2, diagonal = _pairs_chi2(got)
    weak, weak_diagonal = _pairs_chi2(KP.perm_draws(1234, 0, 0, 132000, 12, 2, rounds=4))
    print(f"pairs: chi2 = {chi2:.1f} with {KP.ROUNDS} rounds, {weak:.1f} with 4; df = 131, threshold = {_threshold(131):.1f}")
    assert diagonal == 0 and weak_diagonal == 0                               # a permutation never repeats a value
    assert chi2 < _threshold(131)
    assert weak > _threshold(131), "the pair test does not tell a 4-round network from a sound one"


def test_scene_draw_and_seed_each_change_the_permutation():
    P, base = 4096, (77, 3, 5)
    ref = KP.perm_range(*base, P)
    for other in ((77, 4, 5), (77, 3, 6), (78, 3, 5), (77 + 2 ** 32, 3, 5)):
        agree = float((KP.perm_range(*other, P) == ref).mean())
        assert agree < 0.01, (other, agree)
    # the tag word: the round keys are not the noise generator's words under the same key and counter prefix
    import _philox_ref as PR
    noise = np.stack(PR.philox4x32_10(np.uint64(3), np.uint64(5), np.uint64(0), np.uint64(0), 77, 0))
    assert not np.any(KP.round_keys(77, 3, 5)[:4] == noise)


# ------------------------------------------------------------------------------------------------ the host layer
def _cpu_conditioning():
    from ssdnerf_amd.fitting import Conditioning
    g = torch.Generator().manual_seed(0)
    arrays = [torch.rand((2, 2, 4, 4, 3), generator=g) for _ in range(3)]
    return Conditioning(*arrays, None)


def test_ray_batcher_defaults_to_the_host_and_refuses_the_device_on_cpu_tensors(monkeypatch):
    import inspect
    from ssdnerf_amd.fitting import RayBatcher
    params = inspect.signature(RayBatcher.__init__).parameters
    assert list(params)[:4] == ["self", "cond", "rays_per_step", "fixed"] and params["fixed"].default is True
    assert params["index_source"].default == "host" and params["seed"].default is None
    cond = _cpu_conditioning()
    calls = []
    real = torch.randperm
    monkeypatch.setattr(torch, "randperm", lambda *a, **k: calls.append(a) or real(*a, **k))
    b = RayBatcher(cond, 10)
    assert b.index_source == "host" and len(calls) == 2 and len(b.chunks) == 4      # 32 pixels: three chunks of 10 and one of 2
    assert [tuple(t.shape) for t in b.batch(3)] == [(2, 2, 3)] * 3
    with pytest.raises(ValueError, match="no CPU path"):
        RayBatcher(cond, 10, index_source="device")
    with pytest.raises(ValueError, match="no CPU path"):
        RayBatcher(cond, 10, fixed=False, index_source="device", seed=1)
    with pytest.raises(ValueError, match="ray_index_source"):
        RayBatcher(cond, 10, index_source="gpu")
    assert len(calls) == 2


def test_models_refuse_an_unknown_index_source():
    from ssdnerf_amd.fitting import check_index_source
    from ssdnerf_amd.models import BaseNeRF
    assert check_index_source("host") == "host" and check_index_source("device") == "device"
    for cfgs in (dict(train_cfg=dict(ray_index_source="cuda")), dict(test_cfg=dict(ray_index_source=None))):
        with pytest.raises(ValueError, match="ray_index_source"):
            BaseNeRF(code_size=(3, 2, 8, 8), grid_size=8, **cfgs)


def test_nothing_shipped_sets_the_key():
    """the device draw is opt-in: outside the code that reads the key, its tests, its benchmark and the documents, no file names it"""
    own = {os.path.join("ssdnerf_amd", "fitting.py"), os.path.join("ssdnerf_amd", "models.py"), os.path.join("tools", "bench_ray_perm.py"),
           os.path.join("tests", "test_ray_perm_cpu.py"), os.path.join("tests", "test_ray_perm_gpu.py")}
    found = []
    for top in ("ssdnerf_amd", "tools", "tests", "oracle", "."):
        for folder, _, files in (os.walk(os.path.join(ROOT, top)) if top != "." else [(ROOT, [], os.listdir(ROOT))]):
            if "__pycache__" in folder or os.path.join("ssdnerf_amd", "lib") in folder or os.path.join("oracle", "_") in folder:
                continue
            for name in files:
                path = os.path.join(folder, name)
                if not name.endswith((".py", ".json", ".yaml", ".yml", ".cfg", ".toml")) or not os.path.isfile(path):
                    continue
                if os.path.relpath(path, ROOT) in own or os.path.getsize(path) > 1 << 20:
                    continue
                with open(path, errors="ignore") as f:
                    if "ray_index_source" in f.read():
                        found.append(os.path.relpath(path, ROOT))
    assert found == [], found
    for source in ("fitting.py", "models.py"):
        with open(os.path.join(ROOT, "ssdnerf_amd", source)) as f:
            assert 'get("ray_index_source", "host")' in f.read(), source


@pytest.mark.parametrize("name,count", [("ssdnerf_perm_indices", 8), ("ssdnerf_sample_rays_perm_u8", 17)])
def test_the_entry_points_are_declared_defined_and_bound_with_the_same_parameters(monkeypatch, name, count):
    import re
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd import build

    def parameters(text):
        inside = text[text.index("(") + 1:text.rindex(")")]
        return [p.strip() for p in inside.split(",")]

    with open(os.path.join(ROOT, "include", "ssdnerf_hip.h")) as f:
        declared = re.findall(r"^int %s\([^;]*\);" % name, f.read(), flags=re.M)
    with open(os.path.join(ROOT, "ssdnerf_amd", "csrc", "scene_store.hip")) as f:
        defined = re.findall(r'^extern "C" int %s\([^{]*\)\s*\{' % name, f.read(), flags=re.M)
    assert len(declared) == 1 and len(defined) == 1
    params = parameters(declared[0])
    assert [p.split()[-1] for p in parameters(defined[0])] == [p.split()[-1] for p in params]
    assert name in C.EXPORTS and C.ABI_VERSION == 3 and "keyed_perm.h" in build.HEADERS

    class Fn:                                                            # what ctypes.CDLL hands out, without a library to load
        argtypes = restype = None

    class Lib:
        def __init__(self):
            self.fns = {}

        def __getattr__(self, attr):
            return self.__dict__["fns"].setdefault(attr, Fn())

    fake = Lib()
    fake.fns["ssdnerf_abi_version"] = lambda: C.ABI_VERSION
    monkeypatch.setattr(C, "_lib", None)
    monkeypatch.setattr(C.os.path, "exists", lambda p: True)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: fake)
    C.lib()
    argtypes = fake.fns[name].argtypes
    assert argtypes is not None and len(argtypes) == len(params) == count
    for kind, text in zip(argtypes, params):
        want = ctypes.c_void_p if "*" in text else {"uint64_t": ctypes.c_uint64, "uint32_t": ctypes.c_uint32}[text.split()[0]]
        assert kind is want, (text, kind)
