"""The composite kernels (csrc/raymarching_ops.hip, through ``ssdnerf_amd.raymarching``) and the DDIM step (csrc/sampler_step.hip, through the C ABI as
the sampler calls it) against the float64 references and per-element bounds of tests/_composite_ref.py, on the seeded families that
tests/test_composite_bounds_cpu.py proves the bounds on: ray ids that are not record numbers, shuffled offsets, thin and vanishing media,
opaque samples, records past the end of the sample arrays, padding rows, ragged block tails.  Oracle parity stays in tests/test_hip_ops_gpu.py.

``python tests/test_composite_fp64_gpu.py OUT.json`` runs every case and writes the worst error / bound ratio per output and family
(profiles/composite_bounds.json is such a run)."""
import json
import sys

import numpy as np
import pytest
import torch

import _composite_ref as CR

pytestmark = pytest.mark.gpu


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rm():
    import ssdnerf_amd.raymarching as rm
    return rm


def _train_loss(ws, dep, img, gw, gi):
    return (ws * gw).sum() + (img * gi).sum() + dep.sum() * 3.0            # the depth cotangent must contribute nothing


def run_train(c, T_thresh):
    sig, rgb = cu(c.sigmas).requires_grad_(True), cu(c.rgbs).requires_grad_(True)
    ws, dep, img = _rm().composite_rays_train(sig, rgb, cu(c.deltas), cu(c.rays), T_thresh)
    _train_loss(ws, dep, img, cu(c.grad_ws), cu(c.grad_image)).backward()
    return dict(weights_sum=ws.detach().cpu(), depth=dep.detach().cpu(), image=img.detach().cpu(), grad_sigmas=sig.grad.cpu(), grad_rgbs=rgb.grad.cpu())


def run_infer(c, T_thresh):
    al, rt, ws, dep, img = cu(c.rays_alive), cu(c.rays_t), cu(c.weights_sum), cu(c.depth), cu(c.image)
    assert _rm().composite_rays(c.n_alive, c.n_step, al, rt, cu(c.sigmas), cu(c.rgbs), cu(c.deltas), ws, dep, img, T_thresh) == ()
    return dict(rays_alive=al.cpu(), rays_t=rt.cpu(), weights_sum=ws.cpu(), depth=dep.cpu(), image=img.cpu())


def run_ddim(x_t, v, a, b, c, d, x0_out, xprev_out):
    """the call of diffusion.py's ``_run_plan``"""
    from ssdnerf_amd import _cabi as C
    C.check(C.lib().ssdnerf_ddim_step_v(C.ptr(x_t), C.ptr(v), C.ctypes.c_uint64(v.numel()), C.f32(a), C.f32(b), C.f32(c), C.f32(d), C.f32(-1.0),
                                        C.f32(1.0), C.ptr(x0_out), C.ptr(xprev_out), C.stream()), "ddim_step_v")


# ------------------------------------------------------------------------------------------------ train branch
@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("n_rays", CR.RAY_COUNTS)
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_composite_train_meets_the_fp64_bounds(family, n_rays, T_thresh):
    c, ref = CR.train_reference(family, n_rays, T_thresh)
    assert int(ref.undecided.sum()) <= CR.MAX_UNDECIDED * n_rays
    res = CR.train_failures(run_train(c, T_thresh), ref)
    print(family, n_rays, T_thresh, {k: round(v[1], 3) for k, v in res.items()})
    assert CR.n_failures(res) == 0, res


def test_batch_composite_train_on_two_unequal_scenes_meets_the_same_bounds():
    T_thresh = 1e-4
    # (a record past the end of its own scene's samples lies inside the next scene's once they are concatenated: only the last scene has such)
    cases = [CR.train_reference("wide", 257, T_thresh, n_overflow=0), CR.train_reference("opaque", 255, T_thresh)]
    singles = [run_train(c, T_thresh) for c, _ in cases]
    sig = cu(np.concatenate([c.sigmas for c, _ in cases])).requires_grad_(True)
    rgb = cu(np.concatenate([c.rgbs for c, _ in cases])).requires_grad_(True)
    ws, dep, img = _rm().batch_composite_rays_train(sig, rgb, [cu(c.deltas) for c, _ in cases], [cu(c.rays) for c, _ in cases],
                                                    [c.M for c, _ in cases], T_thresh)
    assert [tuple(w.shape) for w in ws] == [(257,), (255,)]
    sum(_train_loss(ws[i], dep[i], img[i], cu(c.grad_ws), cu(c.grad_image)) for i, (c, _) in enumerate(cases)).backward()
    row = 0
    for i, (c, ref) in enumerate(cases):
        got = dict(weights_sum=ws[i].detach().cpu(), depth=dep[i].detach().cpu(), image=img[i].detach().cpu(),
                   grad_sigmas=sig.grad[row:row + c.M].cpu(), grad_rgbs=rgb.grad[row:row + c.M].cpu())
        row += c.M
        res = CR.train_failures(got, ref)
        assert CR.n_failures(res) == 0, (i, res)
        for k, v in got.items():                                           # a ray's arithmetic does not depend on where its record lies
            assert torch.equal(v, singles[i][k]), (i, k)


# ------------------------------------------------------------------------------------------------ inference branch
@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("n_step", [1, 4, 8])
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_composite_rays_meets_the_fp64_bounds(family, n_step, T_thresh):
    c, ref = CR.infer_reference(family, n_step, T_thresh)
    assert int(ref.undecided.sum()) <= CR.MAX_UNDECIDED * c.n_alive
    res = CR.infer_failures(run_infer(c, T_thresh), ref, c)
    print(family, n_step, T_thresh, {k: round(v[1], 3) for k, v in res.items()})
    assert CR.n_failures(res) == 0, res


# ------------------------------------------------------------------------------------------------ DDIM step
def ddim_results(n, a, b, c, d, seed=7):
    """(x0, x_prev) out of place, and the failures of the two in-place aliasings of the sampler against them, bit for bit"""
    x_np, v_np = CR.ddim_case(n, seed)
    x, v = cu(x_np), cu(v_np)
    x0, xp = torch.full_like(x, float("nan")), torch.full_like(x, float("nan"))
    run_ddim(x, v, a, b, c, d, x0, xp)
    assert torch.equal(x.cpu(), torch.from_numpy(x_np)) and torch.equal(v.cpu(), torch.from_numpy(v_np))       # inputs are left alone
    xa, x0a = x.clone(), torch.full_like(x, float("nan"))                  # the latent updated in place, x0 kept
    run_ddim(xa, v, a, b, c, d, x0a, xa)
    xb, vb = x.clone(), v.clone()                                          # ... and x0 written over the network output
    run_ddim(xb, vb, a, b, c, d, vb, xb)
    bits = lambda t: t.view(torch.int32)
    aliased = sum(int((bits(g) != bits(w)).sum()) for g, w in ((xa, xp), (x0a, x0), (xb, xp), (vb, x0)))
    return x_np, v_np, x0.cpu(), xp.cpu(), aliased


@pytest.mark.parametrize("n", CR.DDIM_SIZES)
def test_ddim_step_meets_the_fp64_bounds_out_of_place_and_in_place(n):
    for name, a, b, c, d in CR.ddim_coefficients():
        x_np, v_np, x0, xp, aliased = ddim_results(n, a, b, c, d)
        p, Bp, ref, Bref = CR.ddim_step_ref(x_np, v_np, a, b, c, d, -1.0, 1.0)
        if n >= 1000:
            assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01
        r0, r1 = CR.check_le(x0, p, Bp), CR.check_le(xp, ref, Bref)
        print(name, n, "x0", round(r0[1], 3), "x_prev", round(r1[1], 3))
        assert r0[0] == 0 and r1[0] == 0, (name, r0, r1)
        assert aliased == 0, name


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}

    def note(key, res):
        for k, v in res.items():
            worst.setdefault(key, {})[k] = max(worst.get(key, {}).get(k, 0.0), round(v[1], 4))

    for family in CR.FAMILIES:
        for T_thresh in CR.THRESHOLDS:
            for n_rays in CR.RAY_COUNTS:
                c, ref = CR.train_reference(family, n_rays, T_thresh)
                res = CR.train_failures(run_train(c, T_thresh), ref)
                note("composite_train/" + family, {k: v for k, v in res.items() if k not in ("unowned", "sane")})
            for n_step in (1, 4, 8):
                c, ref = CR.infer_reference(family, n_step, T_thresh)
                res = CR.infer_failures(run_infer(c, T_thresh), ref, c)
                note("composite_rays/" + family, {k: res[k] for k in ("weights_sum", "depth", "image")})
    for name, a, b, c, d in CR.ddim_coefficients():
        for n in CR.DDIM_SIZES:
            x_np, v_np, x0, xp, _ = ddim_results(n, a, b, c, d)
            p, Bp, ref, Bref = CR.ddim_step_ref(x_np, v_np, a, b, c, d, -1.0, 1.0)
            note("ddim_step/" + name, dict(x0=CR.check_le(x0, p, Bp), x_prev=CR.check_le(xp, ref, Bref)))
    return worst


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = dict(what="worst |kernel - fp64 reference| / bound per output, over every seeded case of tests/test_composite_fp64_gpu.py",
               device=torch.cuda.get_device_name(0), c_exp=CR.C_EXP, worst_ratio=measure())
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
