"""ExponentialMovingAverageHook without a GPU: the arithmetic of csrc/ema_math.h (a gcc build, tests/host/ema_host.c) against the numpy
three-rounding restatement of tests/_ema_ref.py, bit for bit; the ``rampup`` policy against its closed form; the schedule; a CPU model
through the hook's eager path against the plain-torch restatement; the refusals; the build from the configs' ``custom_hooks[0]``; and the
C ABI's declarations and host-side plan validation (no device needed: the pointers are never dereferenced)."""
import ctypes
import json
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import _ema_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOMENTA = [E.rampup(i, **E.CFG_MOMENTUM) for i in (0, 1, 10, 499, 5000, 100000)] + [0.0, 1.0, 0.999]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host") / "ema_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "ema_host.c"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.ema_update.restype = None
    lib.ema_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float]
    return lib


def _same_bits_or_both_nan(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("m", MOMENTA)
def test_host_build_of_the_kernel_arithmetic_is_the_three_rounding_restatement(host, m):
    ema, src = E.make_values(1 << 16, seed=3)
    want = E.update32(ema, src, m)
    got, src_before = ema.copy(), src.copy()
    host.ema_update(got.ctypes.data_as(ctypes.c_void_p), src.ctypes.data_as(ctypes.c_void_p), got.size, m)
    assert _same_bits_or_both_nan(got, want)
    assert np.array_equal(src.view(np.uint32), src_before.view(np.uint32))
    assert np.isnan(want).any() and (np.abs(want[np.isfinite(want)]) < 1.2e-38).any()            # the planted values are there


@pytest.mark.parametrize("m", MOMENTA)
def test_eager_torch_formula_is_the_restatement_and_lerp_is_not(m):
    """what makes bit identity discriminating: the eager expression agrees with the three roundings, ``torch.lerp`` does not"""
    ema, src = E.make_values(1 << 16, seed=4)
    te, ts = torch.from_numpy(ema), torch.from_numpy(src)
    want = E.update32(ema, src, m)
    assert _same_bits_or_both_nan((ts + (te - ts) * m).numpy(), want)
    if 0.5 <= m < 1.0:                                                          # (below 0.5 torch.lerp is this very expression)
        fin = np.isfinite(want)
        assert int((torch.lerp(ts, te, m).numpy()[fin] != want[fin]).sum()) > 0


def test_rampup_momentum_closed_form():
    from ssdnerf_amd.ema import rampup_momentum
    cfg = E.CFG_MOMENTUM
    for it in (0, 1, 10, 499, 4999, 5000, 10 ** 6):
        want = 0.5 ** (16 / max(min(4000, (it + 1) * 16 * 0.05), 1e-8))
        assert rampup_momentum(it, **cfg) == want == E.rampup(it, **cfg), it
        if it >= 4999:
            assert rampup_momentum(it, **cfg) == 0.5 ** (16 / 4000)
    assert rampup_momentum(0, **cfg) == 9.5367431640625e-07 and rampup_momentum(5000, **cfg) == 0.9972312513520695
    ramp = [rampup_momentum(it, **cfg) for it in range(0, 4999)]                # cur_nimg * 0.05 < 4000  <=>  iteration < 4999
    assert all((it + 1) * 16 * 0.05 < 4000 for it in range(0, 4999)) and all(a < b for a, b in zip(ramp, ramp[1:]))
    assert ramp[-1] < rampup_momentum(4999, **cfg)
    # the defaults are mmgen's, and ema_rampup=None switches the ramp off
    assert rampup_momentum(7) == 0.5 ** (4 / max(min(10000, 8 * 4 * 0.05), 1e-8)) and rampup_momentum(0, ema_rampup=None) == 0.5 ** (4 / 10000)


def _tiny(seed):
    """a source network with a buffer, an integer buffer and a frozen parameter"""
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3))
    net[2].bias.requires_grad_(False)
    return net


def _model(seed=0):
    from copy import deepcopy
    m = torch.nn.Module()
    m.net = _tiny(seed)
    m.net_ema = deepcopy(m.net)
    return m


def _perturb(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
        net[1].running_mean.add_(torch.randn(7, generator=g))
        net[1].num_batches_tracked.add_(3)


@pytest.mark.parametrize("interval", [1, 3])
@pytest.mark.parametrize("start_iter", [0, 5])
def test_schedule_and_cpu_model_on_the_eager_path(interval, start_iter):
    from ssdnerf_amd import ema
    hook = ema.ExponentialMovingAverageHook(("net_ema",), interval=interval, start_iter=start_iter, momentum_policy="rampup",
                                            momentum_cfg=E.CFG_MOMENTUM, interp_cfg=dict(momentum_nontrainable=0.25))
    m = _model()
    n_entries = len(m.net.state_dict())
    launches, eager = ema.launches, ema.eager_tensors
    acted = []
    for it in range(12):
        _perturb(m.net, 100 + it)
        src, trainable = E.snapshot(m.net)
        before, _ = E.snapshot(m.net_ema)
        want = E.hook_step(src, trainable, before, it, interval=interval, start_iter=start_iter, momentum_policy="rampup", momentum_cfg=E.CFG_MOMENTUM,
                           momentum_nontrainable=0.25)
        hook.after_train_iter(types.SimpleNamespace(iter=it, model=m))
        E.assert_state_bits_equal(m.net_ema, want, f"iteration {it}")
        E.assert_state_bits_equal(m.net, src, f"source at iteration {it}")
        changed = any(not torch.equal(before[k], want[k]) for k in want)
        acted.append(changed)
        assert hook.acts_at(it) == changed
        if it < start_iter:                                                     # a copy, whatever the interval
            E.assert_state_bits_equal(m.net_ema, src, f"copy at iteration {it}")
    assert acted == [it < start_iter or (it + 1 - start_iter) % interval == 0 for it in range(12)]
    assert ema.launches == launches                                             # a CPU model: no library call
    updates = sum(1 for it in range(12) if it >= start_iter and acted[it])
    assert ema.eager_tensors == eager + updates * n_entries
    assert m.net_ema[1].num_batches_tracked.dtype == torch.int64                # the formula's float result went back through copy_'s cast


def test_fixed_policy_defaults_and_update_entry_point():
    from ssdnerf_amd import ema
    hook = ema.ExponentialMovingAverageHook("net_ema", interval=1)
    assert hook.module_keys == ("net_ema",) and hook.momenta(123) == (0.999, 0.0) and hook.priority == "NORMAL"
    assert not ema.ExponentialMovingAverageHook("net_ema").acts_at(0)           # interval=-1 (the default): never after start_iter
    m = types.SimpleNamespace(module=_model(1))                                 # a wrapper: unwrapped through .module
    _perturb(m.module.net, 5)
    src, trainable = E.snapshot(m.module.net)
    before, _ = E.snapshot(m.module.net_ema)
    hook.after_train_iter(types.SimpleNamespace(iter=0, model=m))
    E.assert_state_bits_equal(m.module.net_ema, E.hook_step(src, trainable, before, 0), "through .module")
    before, _ = E.snapshot(m.module.net_ema)
    assert hook.update(m.module, 1) is True
    E.assert_state_bits_equal(m.module.net_ema, E.hook_step(src, trainable, before, 1), "update()")
    # frozen: the whole source is copied (momentum_nontrainable = 0.0)
    m.module.net.requires_grad_(False)
    hook.update(m.module, 2)
    for k, v in m.module.net.state_dict().items():
        assert torch.equal(m.module.net_ema.state_dict()[k], v), k


def test_half_and_noncontiguous_entries_and_rebuild_on_cpu():
    from ssdnerf_amd import ema
    hook = ema.ExponentialMovingAverageHook(("net_ema",), interval=1, interp_cfg=dict(momentum=0.5))
    m = _model(2)
    hook.update(m, 0)
    m.net[0].half()
    m.net_ema[0].half()
    m.net[2].weight = torch.nn.Parameter(torch.randn(7, 3).t())                  # swapped Parameter, non-contiguous
    _perturb(m.net, 9)
    src, trainable = E.snapshot(m.net)
    before, _ = E.snapshot(m.net_ema)
    hook.update(m, 1)
    E.assert_state_bits_equal(m.net_ema, E.hook_step(src, trainable, before, 1, momentum=0.5), "half + non-contiguous")
    assert m.net_ema[0].weight.dtype == torch.float16


def test_before_run_creates_a_missing_ema_module():
    from ssdnerf_amd import ema
    m = torch.nn.Module()
    m.net = _tiny(3)
    hook = ema.ExponentialMovingAverageHook(("net_ema",), interval=1)
    with pytest.warns(UserWarning):
        hook.before_run(types.SimpleNamespace(iter=0, model=m))
    assert isinstance(m.net_ema, torch.nn.Sequential) and m.net_ema is not m.net
    assert all(a.data_ptr() != b.data_ptr() and torch.equal(a, b) for a, b in zip(m.net.state_dict().values(), m.net_ema.state_dict().values()))
    kept = m.net_ema
    hook.before_run(types.SimpleNamespace(iter=0, model=m))                      # an existing one is left alone
    assert m.net_ema is kept


def test_errors():
    from ssdnerf_amd import ema
    H = ema.ExponentialMovingAverageHook
    with pytest.raises(ValueError, match="_ema"):
        H(("net_ema", "decoder"))
    with pytest.raises(ValueError, match="_ema"):
        H("net")
    with pytest.raises(TypeError):
        H(3)
    with pytest.raises(NotImplementedError, match="slerp"):
        H("net_ema", interp_mode="slerp")
    with pytest.raises(NotImplementedError, match="cosine"):
        H("net_ema", momentum_policy="cosine")
    with pytest.raises(TypeError):
        H("net_ema", momentum_policy="rampup", momentum_cfg=dict(no_such_key=1))
    empty = torch.nn.Module()
    with pytest.raises(RuntimeError, match="Cannot find"):
        H("net_ema", interval=1).before_run(types.SimpleNamespace(iter=0, model=empty))
    with pytest.raises(RuntimeError, match="Cannot find"):
        H("net_ema", interval=1).update(empty, 0)
    only_src = torch.nn.Module()
    only_src.net = _tiny(0)
    with pytest.raises(RuntimeError, match="net_ema"):
        H("net_ema", interval=1).update(only_src, 0)                             # before_run was skipped
    bad = _model()
    bad.net_ema[0] = torch.nn.Linear(5, 8)
    with pytest.raises(RuntimeError, match="size mismatch"):
        H("net_ema", interval=1).update(bad, 0)
    fewer = _model()
    del fewer.net_ema[1]
    with pytest.raises(KeyError):
        H("net_ema", interval=1).update(fewer, 0)


def test_builds_from_the_configs_custom_hook():
    import ssdnerf_amd
    from ssdnerf_amd import ema
    from ssdnerf_amd.registry import HOOKS, build_hook
    with open(os.path.join(ROOT, "tests", "golden", "ema_hook_cfg.json")) as f:
        cfg = json.load(f)["custom_hooks_0"]
    cfg["module_keys"] = tuple(cfg["module_keys"])
    assert cfg == dict(type="ExponentialMovingAverageHook", module_keys=("diffusion_ema", "decoder_ema"), interp_mode="lerp", interval=1, start_iter=0,
                       momentum_policy="rampup", momentum_cfg=dict(ema_kimg=4, ema_rampup=0.05, batch_size=16, eps=1e-8), priority="VERY_HIGH")
    hook = build_hook(cfg)
    assert isinstance(hook, ema.ExponentialMovingAverageHook) and "ExponentialMovingAverageHook" in HOOKS and ssdnerf_amd.build_hook is build_hook
    assert hook.module_keys == ("diffusion_ema", "decoder_ema") and hook.priority == "VERY_HIGH" and hook.interval == 1 and hook.start_iter == 0
    assert all(hook.acts_at(i) for i in range(5))
    assert hook.momenta(0) == (9.5367431640625e-07, 0.0) and hook.momenta(5000) == (0.5 ** (16 / 4000), 0.0)


def test_abi_declarations():
    from ssdnerf_amd import _cabi as C, build
    header = open(os.path.join(ROOT, "include", "ssdnerf_hip.h")).read()
    assert "int ssdnerf_ema_plan_build(ssdnerf_ema_row* rows, uint32_t T, uint32_t* blocks_out);" in header
    assert ("int ssdnerf_ema_update_multi(const ssdnerf_ema_row* plan, uint32_t T, uint32_t blocks, float momentum, float momentum_nontrainable, "
            "void* stream);") in header
    assert "ema.hip" in build.SOURCES and "ema_math.h" in build.HEADERS
    for name in ("ssdnerf_ema_plan_build", "ssdnerf_ema_update_multi", "ssdnerf_ema_chunk"):
        assert name in C.EXPORTS
    assert ctypes.sizeof(C.EmaRow) == 32 and C.lib().ssdnerf_ema_chunk() == 4096


def _plan(rows):
    from ssdnerf_amd import _cabi as C
    tab = (C.EmaRow * max(len(rows), 1))()
    for e, (src, dst, numel, trainable) in zip(tab, rows):
        e.src, e.dst, e.numel, e.trainable, e.first_block = src, dst, numel, trainable, 0xdeadbeef
    blocks = ctypes.c_uint32(0)
    return C.lib().ssdnerf_ema_plan_build(tab, len(rows), ctypes.byref(blocks)), tab, blocks.value


def test_plan_build_fills_the_prefix_sums_and_refuses_bad_rows():
    from ssdnerf_amd import _cabi as C
    lib, K = C.lib(), 4096
    MB = 1 << 20
    status, tab, blocks = _plan([(1 * MB, 11 * MB, 1, 1), (2 * MB, 12 * MB, K, 0), (3 * MB, 13 * MB, K + 1, 1), (1 * MB, 14 * MB, 3 * K + 7, 0),
                                 (2 * MB + 4, 15 * MB + 4, 5, 1)])                # sources may repeat and overlap each other
    assert status == 0, lib.ssdnerf_last_error().decode()
    assert [e.first_block for e in tab] == [0, 1, 2, 4, 8] and blocks == 9
    ok = (1 * MB, 11 * MB, 8, 1)
    for rows, cause in [([], "T == 0"), ([(0, 11 * MB, 8, 1)], "null pointer in row 0"), ([ok, (2 * MB, 0, 8, 1)], "null pointer in row 1"),
                        ([(1 * MB + 2, 11 * MB, 8, 1)], "4-byte aligned"), ([(1 * MB, 11 * MB + 1, 8, 1)], "4-byte aligned"),
                        ([(1 * MB, 11 * MB, 0, 1)], "numel == 0"), ([(1 * MB, 11 * MB, (1 << 40) + 1, 1)], "2^40"), ([(1 * MB, 11 * MB, 8, 2)], "trainable"),
                        ([ok, (2 * MB, 11 * MB, 8, 1)], "appears twice"), ([ok, (2 * MB, 11 * MB, 4, 0)], "appears twice"),
                        ([ok, (2 * MB, 11 * MB + 16, 8, 1)], "overlaps dst"), ([(1 * MB, 11 * MB, 2 * MB, 1), (2 * MB, 11 * MB + 4 * MB, 8, 1)], "overlaps dst"),
                        ([ok, (11 * MB + 28, 12 * MB, 8, 1)], "overlaps src"), ([ok, (3 * MB, 1 * MB + 28, 8, 1)], "overlaps src"),
                        ([(1 * MB, 1 * MB, 8, 1)], "overlaps src"), ([(1 * MB, 1 * MB + 16, 8, 1)], "overlaps src"),
                        ([ok, (11 * MB - 32, 12 * MB, 9, 1)], "overlaps src")]:
        status, tab, _ = _plan(rows)
        msg = lib.ssdnerf_last_error().decode()
        assert status == -1 and msg.startswith("ema_plan_build") and cause in msg, (rows, cause, msg)
        with pytest.raises(RuntimeError, match="ema_plan_build"):
            C.check(status, "ema_plan_build")
    # neighbours that only touch are fine
    assert _plan([(1 * MB, 11 * MB, 8, 1), (1 * MB + 32, 11 * MB + 32, 8, 1), (11 * MB - 32, 12 * MB, 8, 0)])[0] == 0
    assert lib.ssdnerf_ema_plan_build(None, 1, ctypes.byref(ctypes.c_uint32(0))) == -1 and "null pointer" in lib.ssdnerf_last_error().decode()
    # the launch entry point refuses before any HIP call what no plan_build returns
    for args, cause in [((None, 1, 1), "null pointer"), ((4, 1, 1), "8-byte aligned"), ((256, 0, 1), "T = 0"), ((256, 2, 1), "blocks")]:
        assert lib.ssdnerf_ema_update_multi(*args, 0.5, 0.0, None) == -1 and cause in lib.ssdnerf_last_error().decode(), cause


def test_plan_build_agrees_with_a_brute_force_overlap_check():
    """random tables, some with a dst thrown among the sources: accepted exactly when no dst range meets another dst or any src range"""
    rng = np.random.default_rng(11)
    accepted = refused = 0
    for trial in range(400):
        T = int(rng.integers(1, 24))
        rows = []
        for k in range(T):
            clash = trial % 2 == 0 and rng.integers(0, 8) == 0
            src = 0x100000 + int(rng.integers(0, 64)) * 4096 + int(rng.integers(0, 4)) * 4
            dst = 0x100000 + int(rng.integers(0, 64)) * 4096 if clash else 0x40000000 + k * 0x100000 + int(rng.integers(0, 4)) * 4
            rows.append((src, dst, int(rng.integers(1, 20000)), int(rng.integers(0, 2))))
        span = lambda a, n: (a, a + 4 * n)
        meet = lambda p, q: p[0] < q[1] and q[0] < p[1]
        bad = any(meet(span(d, n), span(s2, n2)) or (i != j and meet(span(d, n), span(d2, n2)))
                  for i, (_, d, n, _) in enumerate(rows) for j, (s2, d2, n2, _) in enumerate(rows))
        status, tab, blocks = _plan(rows)
        assert (status != 0) == bad, (trial, rows)
        if status == 0:
            accepted += 1
            counts = [(n + 4095) // 4096 for _, _, n, _ in rows]
            assert [e.first_block for e in tab] == [sum(counts[:k]) for k in range(T)] and blocks == sum(counts)
            assert all((e.src, e.dst, e.numel, e.trainable) == r for e, r in zip(tab, rows))          # the rows themselves are left as given
        else:
            refused += 1
    assert accepted > 50 and refused > 50, (accepted, refused)
