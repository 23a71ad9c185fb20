"""The per-element bounds of tests/_composite_ref.py without a GPU: fp32 emulations of the composite kernels and of the DDIM step (same order of
operations, an fma where the kernel has one, numpy's fp32 exp for the hardware one) must meet every bound on every input family, and emulations
of subtly wrong kernels must not.  Each mutation is an error that the flat tolerances of tests/test_hip_ops_gpu.py, its ray-ordered records
or its single input distribution let through.  The share of rays the reference leaves undecided is asserted here for every seeded case."""
import numpy as np
import pytest
import torch

import _composite_ref as CR

F32 = np.float32


def _fma(a, b, c):
    """fl32(a b + c): the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)


def _bf16(x):
    return torch.from_numpy(np.ascontiguousarray(x)).bfloat16().float().numpy()


# ------------------------------------------------------------------------------------------------ emulations
def emu_train(c, T_thresh, by_record=False, out_by_record=False, write_trip=False, skip_alpha0=False, stale=0.0, bf16_ws=False):
    """k_composite_train_fwd + k_composite_train_bwd in fp32, all rays at once, one step of every ray per iteration.  Mutations: ``by_record``: the
    backward reads grad_image / grad_ws / image / weights_sum at the record number, not the ray id; ``out_by_record``: the forward writes its outputs
    at the record number; ``write_trip``: the tripping sample's gradient
    is written; ``skip_alpha0``: the backward skips samples whose fp32 alpha is 0; ``stale``: the gradient buffers start from this value instead
    of 0; ``bf16_ws``: weights_sum is rounded to bf16 after every addition."""
    sig, rgb, dl, rays, M = c.sigmas, c.rgbs, c.deltas, c.rays.astype(np.int64), c.M
    N, thr = rays.shape[0], F32(T_thresh)
    rid, off, cnt = rays[:, 0], rays[:, 1], rays[:, 2]
    live = (cnt > 0) & (off + cnt <= M)
    L = int(cnt[live].max()) if live.any() else 0
    ws, d, img = np.zeros(N, F32), np.zeros(N, F32), np.zeros((N, 3), F32)
    g_sig, g_rgb = np.full(M, stale, F32), np.full((M, 3), stale, F32)

    def sample(k, act):
        i = np.where(act, off + k, 0)
        dt = dl[i, 0]
        alpha = F32(1) - np.exp(-sig[i] * dt)
        return i, dt, alpha

    T, alive = np.ones(N, F32), live.copy()
    for k in range(L):                                                     # forward
        act = alive & (k < cnt)
        i, dt, alpha = sample(k, act)
        w = alpha * T
        for ch in range(3):
            img[:, ch] = np.where(act, _fma(w, rgb[i, ch], img[:, ch]), img[:, ch])
        d = np.where(act, _fma(w, dl[i, 1], d), d)
        wsn = ws + w
        ws = np.where(act, _bf16(wsn) if bf16_ws else wsn, ws)
        T = np.where(act, T * (F32(1) - alpha), T)
        alive &= ~(act & (T < thr))
    out_ws, out_d, out_img = np.zeros(N, F32), np.zeros(N, F32), np.zeros((N, 3), F32)
    if out_by_record:
        out_ws, out_d, out_img = ws.copy(), d.copy(), img.copy()
    else:
        out_ws[rid], out_d[rid], out_img[rid] = ws, d, img

    key = np.arange(N) if by_record else rid                               # backward: what it reads per ray
    g3, gw, F3, wsF = c.grad_image[key], c.grad_ws[key], out_img[key], out_ws[key]
    T, alive, p = np.ones(N, F32), live.copy(), np.zeros((N, 3), F32)
    for k in range(L):
        act = alive & (k < cnt)
        i, dt, alpha = sample(k, act)
        w = alpha * T
        for ch in range(3):
            p[:, ch] = np.where(act, _fma(w, rgb[i, ch], p[:, ch]), p[:, ch])
        T = np.where(act, T * (F32(1) - alpha), T)
        trip = act & (T < thr)
        alive &= ~trip
        wr = act if write_trip else act & ~trip
        if skip_alpha0:
            wr = wr & (alpha != 0)
        acc = g3[:, 0] * _fma(T, rgb[i, 0], -(F3[:, 0] - p[:, 0]))
        acc = _fma(g3[:, 1], _fma(T, rgb[i, 1], -(F3[:, 1] - p[:, 1])), acc)
        acc = _fma(g3[:, 2], _fma(T, rgb[i, 2], -(F3[:, 2] - p[:, 2])), acc)
        acc = _fma(gw, F32(1) - wsF, acc)
        g_sig[i[wr]] = (dt * acc)[wr]
        g_rgb[i[wr]] = (g3 * w[:, None])[wr]
    return dict(weights_sum=out_ws, depth=out_d, image=out_img, grad_sigmas=g_sig, grad_rgbs=g_rgb)


def emu_infer(c, T_thresh, post_T=False):
    """k_composite_rays in fp32.  ``post_T``: the threshold is tested on the transmittance after the sample"""
    na, ns, thr = c.n_alive, c.n_step, F32(T_thresh)
    ids = c.rays_alive[:na].astype(np.int64)
    sig, rgb, dl = c.sigmas.reshape(na, ns), c.rgbs.reshape(na, ns, 3), c.deltas.reshape(na, ns, 2)
    ws_all, d_all, img_all, rt = c.weights_sum.copy(), c.depth.copy(), c.image.copy(), c.rays_t.copy()
    ws, d, img = ws_all[ids], d_all[ids], img_all[ids]
    run, early = np.ones(na, bool), np.zeros(na, bool)
    for k in range(ns):
        dt = dl[:, k, 0]
        empty = run & (dt == 0)
        early |= empty
        run &= ~empty
        alpha = F32(1) - np.exp(-sig[:, k] * dt)
        T = F32(1) - ws
        w = alpha * T
        ws = np.where(run, ws + w, ws)
        d = np.where(run, _fma(w, dl[:, k, 1], d), d)
        for ch in range(3):
            img[:, ch] = np.where(run, _fma(w, rgb[:, k, ch], img[:, ch]), img[:, ch])
        trip = run & (((F32(1) - ws) if post_T else T) < thr)
        early |= trip
        run &= ~trip
    alive = np.where(early, -1, ids)
    rt[ids[~early]] = (dl[:, ns - 1, 1] + dl[:, ns - 1, 0])[~early]
    ws_all[ids], d_all[ids], img_all[ids] = ws, d, img
    return dict(rays_alive=alive, rays_t=rt, weights_sum=ws_all, depth=d_all, image=img_all)


def emu_ddim(x, v, a, b, c, d, lo=-1.0, hi=1.0, eps_unclamped=False, bf16_b=False):
    a, b, c, d = F32(a), F32(b), F32(c), F32(d)
    if bf16_b:
        b = F32(_bf16(np.array([b], F32))[0])
    p0 = a * x - b * v
    p = np.clip(p0, F32(lo), F32(hi))
    eps = (x - a * (p0 if eps_unclamped else p)) * (F32(1) / b)
    return p, c * p + d * eps


# ------------------------------------------------------------------------------------------------ checks
_train, _infer, train_failures, infer_failures = CR.train_reference, CR.infer_reference, CR.train_failures, CR.infer_failures


@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("n_rays", CR.RAY_COUNTS)
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_train_bounds_accept_the_kernel_arithmetic(family, n_rays, T_thresh):
    c, ref = _train(family, n_rays, T_thresh)
    assert int(ref.undecided.sum()) <= CR.MAX_UNDECIDED * n_rays
    res = train_failures(emu_train(c, T_thresh), ref)
    print(family, n_rays, T_thresh, {k: round(v[1], 3) for k, v in res.items()})
    assert CR.n_failures(res) == 0, res
    if n_rays >= 255:                                                       # the case exercises what it is meant to
        assert int(ref.owned.sum()) > 0 and int((~ref.live).sum()) >= 4    # a count of 0 and three records with off + cnt > M
        live_rec = ref.live[torch.from_numpy(c.rays[:, 0].astype(np.int64))].numpy()
        tripped = int(ref.owned.sum()) < int(c.rays[live_rec, 2].sum())    # some ray stops before its last sample
        assert tripped == (family in ("wide", "opaque"))


@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("family", ["wide", "opaque"])
def test_train_bounds_reject_a_gradient_for_the_tripping_sample(family, T_thresh):
    c, ref = _train(family, 257, T_thresh)
    res = train_failures(emu_train(c, T_thresh, write_trip=True), ref)
    assert res["unowned"][0] > 0
    old = np.abs(emu_train(c, T_thresh, write_trip=True)["grad_sigmas"] - ref.grad_sigmas.numpy())
    if T_thresh == 1e-4:
        assert old.max() < 2e-5                                             # ... and the old absolute tolerance did not see it


def test_train_bounds_reject_a_backward_that_skips_zero_alpha_samples():
    c, ref = _train("vanishing", 257, 1e-4)
    alpha = F32(1) - np.exp(-c.sigmas * c.deltas[:, 0])
    owned = ref.owned.numpy()
    assert int((owned & (alpha == 0) & (c.sigmas > 0)).sum()) > 100 and int((owned & (c.sigmas == 0)).sum()) > 100    # the family has such samples
    res = train_failures(emu_train(c, 1e-4, skip_alpha0=True), ref)
    assert res["grad_sigmas"][0] > 0


def test_train_reference_on_an_empty_scene():
    """M == 0: every record says zero samples; zeros for every ray, no gradient rows"""
    rays = np.stack([np.arange(5), np.zeros(5), np.zeros(5)], 1).astype(np.int32)
    ref = CR.composite_train_ref(np.zeros(0, F32), np.zeros((0, 3), F32), np.zeros((0, 2), F32), rays, 1e-4, np.ones(5, F32), np.ones((5, 3), F32))
    assert ref.weights_sum.shape == (5,) and float(ref.weights_sum.abs().max()) == 0 and float(ref.B_image.max()) == 0
    assert ref.grad_sigmas.shape == (0,) and ref.grad_rgbs.shape == (0, 3) and not bool(ref.live.any())


@pytest.mark.parametrize("family", CR.FAMILIES)
def test_train_bounds_reject_per_ray_inputs_read_by_record_number(family):
    c, ref = _train(family, 257, 1e-4)
    res = train_failures(emu_train(c, 1e-4, by_record=True), ref)
    assert res["grad_sigmas"][0] > 0 and res["grad_rgbs"][0] > 0
    res = train_failures(emu_train(c, 1e-4, out_by_record=True), ref)      # ... and the reverse, for the forward's outputs
    assert res["weights_sum"][0] > 0 and res["depth"][0] > 0 and res["image"][0] > 0


@pytest.mark.parametrize("family", ["wide", "opaque"])
def test_train_bounds_reject_stale_gradient_rows_past_the_trip(family):
    c, ref = _train(family, 257, 1e-4)
    res = train_failures(emu_train(c, 1e-4, stale=1e-7), ref)
    assert res["unowned"][0] > 0


@pytest.mark.parametrize("family", ["thin", "wide"])
def test_train_bounds_reject_weights_sum_accumulated_in_bf16_steps(family):
    c, ref = _train(family, 257, 1e-4)
    res = train_failures(emu_train(c, 1e-4, bf16_ws=True), ref)
    assert res["weights_sum"][0] > 0


# ------------------------------------------------------------------------------------------------ inference composite
@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("n_step", [1, 4, 8])
@pytest.mark.parametrize("family", CR.FAMILIES)
def test_inference_bounds_accept_the_kernel_arithmetic(family, n_step, T_thresh):
    c, ref = _infer(family, n_step, T_thresh)
    assert int(ref.undecided.sum()) <= CR.MAX_UNDECIDED * c.n_alive
    res = infer_failures(emu_infer(c, T_thresh), ref, c)
    print(family, n_step, T_thresh, {k: round(v[1], 3) for k, v in res.items()})
    assert CR.n_failures(res) == 0, res
    dead = int((ref.rays_alive < 0).sum())
    assert 0 < dead < c.n_alive or n_step == 1                              # both ends of the alive flag occur


@pytest.mark.parametrize("T_thresh", CR.THRESHOLDS)
@pytest.mark.parametrize("n_step", [1, 4, 8])
def test_inference_bounds_reject_the_threshold_on_the_post_sample_transmittance(n_step, T_thresh):
    c, ref = _infer("opaque", n_step, T_thresh)                             # (a dense sample in every ray: the two conventions part there)
    res = infer_failures(emu_infer(c, T_thresh, post_T=True), ref, c)
    assert res["rays_alive"][0] > 0 or res["weights_sum"][0] > 0


# ------------------------------------------------------------------------------------------------ DDIM step
@pytest.mark.parametrize("n", CR.DDIM_SIZES)
def test_ddim_bounds_accept_the_kernel_arithmetic_and_reject_two_wrong_ones(n):
    x, v = CR.ddim_case(n, 7)
    coeffs = CR.ddim_coefficients()
    assert coeffs[0][1] < 0.01 and coeffs[-1][2] < 0.011 and coeffs[-2][2] < 0.02
    for name, a, b, c, d in coeffs:
        p, Bp, xp, Bxp = CR.ddim_step_ref(x, v, a, b, c, d, -1.0, 1.0)
        if n >= 1000:
            assert float((p == -1).double().mean()) > 0.01 and float((p == 1).double().mean()) > 0.01
        gp, gx = emu_ddim(x, v, a, b, c, d)
        assert CR.check_le(gp, p, Bp)[0] == 0 and CR.check_le(gx, xp, Bxp)[0] == 0, name
        if n >= 1000:
            gp, gx = emu_ddim(x, v, a, b, c, d, bf16_b=True)
            assert CR.check_le(gp, p, Bp)[0] + CR.check_le(gx, xp, Bxp)[0] > 0, name
            if d != 0:                                                      # (the very last step lands on x0: eps is multiplied by 0)
                gp, gx = emu_ddim(x, v, a, b, c, d, eps_unclamped=True)
                assert CR.check_le(gx, xp, Bxp)[0] > 0, name
