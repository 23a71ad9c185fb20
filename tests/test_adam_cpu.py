"""HIPAdam without a GPU: the arithmetic of csrc/adam_math.h (a gcc build, tests/host/adam_host.c) and torch's own CPU Adam against the float64
step and the per-element bounds of tests/_adam_ref.py over 40 steps; wrong variants of the step against the same bounds; the factory, the
refusals of the Python class and of the C ABI, and ``step_all`` over plain torch optimizers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import _adam_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUMEL, STEPS, LR = 4099, 40, 1e-2


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("host") / "adam_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "adam_host.c"), "-o", so, "-lm"],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.adam_step.restype = None
    lib.adam_step.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_size_t] + [ctypes.c_double] * 3 + [ctypes.c_float] * 3
    return lib


@pytest.fixture(scope="module")
def problem():
    return A.make_problem(NUMEL, STEPS, seed=1)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _worst(trace):
    return tuple(max(t[k] for t in trace) for k in range(3))


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_host_build_of_the_kernel_arithmetic_meets_the_bounds(host, problem, wd):
    p0, grads = problem
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    trace = []
    for k in range(STEPS):
        before = (p.copy(), grads[k], m.copy(), v.copy())
        step_size, bc2_sqrt = A.scalars(k + 1, LR)
        host.adam_step(_p(p), _p(grads[k]), _p(m), _p(v), NUMEL, 0.9, 0.999, 1e-8, step_size, bc2_sqrt, wd)
        trace.append(A.excess((p, m, v), before, k + 1, LR, wd=wd))
    print("worst error / bound (param, exp_avg, exp_avg_sq):", _worst(trace))
    assert max(_worst(trace)) <= 1, _worst(trace)
    assert np.all(p[:A.ZEROS] != p0[:A.ZEROS]) and np.all(v >= 0)              # every block has moved after 40 steps


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_torch_cpu_adam_meets_the_same_bounds(problem, wd):
    p0, grads = problem
    p = torch.from_numpy(p0.copy()).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=LR, weight_decay=wd)
    trace = []
    for k in range(STEPS):
        st = opt.state[p]
        m0, v0 = (st[key].numpy().copy() if st else np.zeros_like(p0) for key in ("exp_avg", "exp_avg_sq"))
        before = (p.detach().numpy().copy(), grads[k], m0, v0)
        p.grad = torch.from_numpy(grads[k].copy())
        opt.step()
        st = opt.state[p]
        trace.append(A.excess((p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()), before, k + 1, LR, wd=wd))
    print("worst error / bound (param, exp_avg, exp_avg_sq):", _worst(trace))
    assert max(_worst(trace)) <= 1, _worst(trace)


def _trajectory(problem, wd):
    """states along the float64 step rounded to fp32 after every step: [(param, grad, exp_avg, exp_avg_sq) before step k + 1]"""
    p0, grads = problem
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    out = []
    for k in range(STEPS):
        out.append((p, grads[k], m, v))
        p, m, v = (a.astype(np.float32) for a in A.step64(p, grads[k], m, v, k + 1, LR, wd=wd))
    return out


@pytest.mark.parametrize("variant", A.VARIANTS)
def test_wrong_variants_break_the_bounds(problem, variant):
    """from every state of the 40-step trajectory, the wrong step rounded to fp32 lies outside the bounds (the right one inside).  The step
    count off by one has no first step; decoupled decay is Adam itself without weight decay."""
    for wd in ([0.01] if variant == "adamw" else [0.0, 0.01]):
        for k, before in enumerate(_trajectory(problem, wd)):
            step = k + 1
            right = tuple(a.astype(np.float32) for a in A.step64(*before, step, LR, wd=wd))
            assert max(A.excess(right, before, step, LR, wd=wd)) <= 1
            if variant == "step_off_by_one" and step == 1:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                wrong = tuple(a.astype(np.float32) for a in A.step64(*before, step, LR, wd=wd, variant=variant))
            assert max(A.excess(wrong, before, step, LR, wd=wd)) > 1, (variant, wd, step, A.excess(wrong, before, step, LR, wd=wd))


@pytest.mark.parametrize("variant", ["eps_in_sqrt_raw", "eps_in_sqrt_corrected"])
def test_eps_variants_are_caught_by_the_small_gradient_block(problem, variant):
    """after the first step only the elements whose gradients stay at the 10^-6 scale tell eps under the square root from eps outside it"""
    before = _trajectory(problem, 0.0)[20]
    wrong = tuple(a.astype(np.float32) for a in A.step64(*before, 21, LR, variant=variant))
    cut = lambda t, sl: tuple(a[sl] for a in t)
    small = slice(0, A.SMALL)
    assert A.excess(cut(wrong, small), cut(before, small), 21, LR)[0] > 1


def test_factory_builds_hipadam():
    from ssdnerf_amd.models import BaseNeRF, _torch_factory
    from ssdnerf_amd.optim import HIPAdam
    cls, kw = _torch_factory(torch.optim, dict(type="HIPAdam", lr=0.02, weight_decay=0.0))
    assert cls is HIPAdam and kw == dict(lr=0.02, weight_decay=0.0)
    assert _torch_factory(torch.optim, dict(type="Adam", lr=0.02))[0] is torch.optim.Adam                   # the default stays torch's
    assert _torch_factory(torch.optim.lr_scheduler, dict(type="ExponentialLR", gamma=0.9))[0] is torch.optim.lr_scheduler.ExponentialLR
    with pytest.raises(ValueError, match="GPU"):                                                           # the class is built: it refuses a CPU leaf
        BaseNeRF.build_optimizer([torch.zeros(4, requires_grad=True)], dict(optimizer=dict(type="HIPAdam", lr=0.02)))


def test_hipadam_refuses_what_it_does_not_implement():
    from ssdnerf_amd.optim import HIPAdam
    cpu = torch.zeros(8, requires_grad=True)
    with pytest.raises(ValueError, match="GPU"):
        HIPAdam([cpu], lr=1e-3)
    with pytest.raises(ValueError, match="GPU"):
        HIPAdam([dict(params=[cpu], lr=1e-3)])
    with pytest.raises(TypeError):
        HIPAdam([torch.zeros(8, dtype=torch.float64, requires_grad=True)])
    with pytest.raises(TypeError):
        HIPAdam([torch.zeros(8, dtype=torch.float16, requires_grad=True)])
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            HIPAdam([cpu], **{flag: True})
    with pytest.raises(TypeError):
        HIPAdam([cpu], momentum=0.9)
    with pytest.raises(ValueError):
        HIPAdam([cpu], betas=(1.0, 0.999))


def test_step_all_over_torch_optimizers_is_the_loop():
    from ssdnerf_amd import optim
    g = torch.Generator().manual_seed(0)
    start = [torch.randn(33, generator=g) for _ in range(3)]
    grads = [[torch.randn(33, generator=g) for _ in range(3)] for _ in range(5)]

    def run(stepper):
        ps = [s.clone().requires_grad_(True) for s in start]
        opts = [torch.optim.Adam([ps[0]], lr=0.01), torch.optim.SGD([ps[1]], lr=0.1, momentum=0.9), torch.optim.Adam([ps[2]], lr=0.02, weight_decay=0.01)]
        for step_grads in grads:
            for p, gr in zip(ps, step_grads):
                p.grad = gr.clone()
            stepper(opts)
        return ps, opts

    before = optim.launches
    a, oa = run(optim.step_all)
    b, ob = run(lambda opts: [o.step() for o in opts])
    assert optim.launches == before                                                                        # no library call for torch optimizers
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.equal(oa[0].state[a[0]]["exp_avg_sq"], ob[0].state[b[0]]["exp_avg_sq"]) and float(oa[2].state[a[2]]["step"]) == 5.0
    optim.step_all([])                                                                                     # an empty list is a no-op


def test_abi_declarations_and_capacity():
    from ssdnerf_amd import _cabi as C, build, optim
    header = open(os.path.join(ROOT, "include", "ssdnerf_hip.h")).read()
    assert ("int ssdnerf_adam_step_multi(const ssdnerf_adam_tensor* tensors, uint32_t T, double beta1, double beta2, double eps, void* stream);") in header
    assert f"#define SSDNERF_ADAM_MAX_TENSORS {optim.CAPACITY}\n" in header
    assert "adam.hip" in build.SOURCES and "adam_math.h" in build.HEADERS
    for name in ("ssdnerf_adam_step_multi", "ssdnerf_adam_max_tensors"):
        assert name in C.EXPORTS
    assert C.lib().ssdnerf_adam_max_tensors() == optim.CAPACITY
    assert ctypes.sizeof(C.AdamTensor) == 56


def test_library_refuses_bad_tables_before_any_hip_call():
    """no device needed: the pointers below are never dereferenced"""
    from ssdnerf_amd import _cabi as C, optim
    lib = C.lib()

    def call(rows, T=None):
        tab = (C.AdamTensor * max(len(rows), 1))()
        for e, (ptrs, numel) in zip(tab, rows):
            e.param, e.grad, e.exp_avg, e.exp_avg_sq = ptrs
            e.numel, e.step_size, e.bc2_sqrt, e.weight_decay = numel, 1e-3, 1.0, 0.0
        return lib.ssdnerf_adam_step_multi(tab, len(rows) if T is None else T, 0.9, 0.999, 1e-8, None)

    ok = (256, 512, 768, 1024)
    for rows, T, cause in [([(ok, 8)], 0, "T == 0"), ([(ok, 0)], None, "numel == 0"), ([(ok, 8), ((256, 0, 768, 1024), 8)], None, "null pointer in tensor 1"),
                           ([((0, 512, 768, 1024), 8)], None, "null pointer"), ([((256, 512, 768, 1026), 8)], None, "4-byte aligned"),
                           ([(ok, 8)] * (optim.CAPACITY + 1), None, "at most"), ([(ok, (1 << 40) + 1)], None, "2^40")]:
        assert call(rows, T) == -1, cause
        msg = lib.ssdnerf_last_error().decode()
        assert msg.startswith("adam_step_multi") and cause in msg, msg
    assert lib.ssdnerf_adam_step_multi(None, 1, 0.9, 0.999, 1e-8, None) == -1 and "null pointer" in lib.ssdnerf_last_error().decode()
