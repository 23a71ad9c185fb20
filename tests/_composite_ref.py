"""float64 references of the volume-rendering composite kernels (csrc/raymarching_ops.hip: k_composite_train_fwd, k_composite_train_bwd,
k_composite_rays) and of the DDIM update (csrc/sampler_step.hip: k_step_v, form 0 without noise), with per-element error bounds derived from them, and the seeded input
families both test modules draw from: tests/test_composite_bounds_cpu.py (the bounds accept an fp32 emulation of each kernel and reject subtly
wrong ones) and tests/test_composite_fp64_gpu.py (the kernels meet them).

The semantics are the kernels' and oracle/raymarching_oracle.c's, not autograd of the continuous formula: the sample that takes the
transmittance below ``T_thresh`` is composited but receives no gradient, nothing after it is touched, a record with ``cnt == 0`` or
``off + cnt > M`` gives zeros and writes no gradient.  Every input (an fp32 tensor, a threshold or coefficient passed as a C float) is taken as
the exact value the kernel read and upcast.  A bound is a forward error analysis of the fp32 kernel, u = 2^-24: ``c * u * (sum of the magnitudes
that an fp32 computation of the same expression rounds)``, carried from step to step by recursion, with the derivation next to each term.
Second-order products of two error terms are kept where they cost nothing and dropped otherwise.

The only constant that is not IEEE arithmetic is ``C_EXP``, the allowance for the hardware exponential in alpha = 1 - exp(-sigma dt) (see
``alpha_terms``).  Measured on an MI355X over every seeded case (profiles/composite_bounds.json, written by ``python
tests/test_composite_fp64_gpu.py OUT.json``), the worst error / bound ratio with C_EXP = 3 is, per family (wide / thin / vanishing / opaque):
train branch weights_sum 0.17 / 0.19 / 0.21 / 0.05, depth 0.45 / 0.19 / 0.21 / 0.07, image 0.54 / 0.20 / 0.21 / 0.15, grad_sigmas 0.18 / 0.12 /
0.19 / 0.09, grad_rgbs 0.48 / 0.23 / 0.23 / 0.21 -- below the 0.64 of the IEEE emulation with a correctly rounded exp, so the constant stays
at 3; ``composite_rays`` weights_sum 0.50, depth 0.89 - 0.96, image 0.93 - 0.98 (a single fma onto a non-zero incoming value errs by up to
u times that value, which is the whole bound there); DDIM x0 0.96 - 0.99, x_prev 0.37 - 0.74 (2 M elements find the worst case of three
roundings).  None of these bounds has a constant fitted to the kernels.

Nothing here needs a GPU: numpy arrays and tensors of any device are accepted, the results are float64 tensors on the CPU."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

U32 = 2.0 ** -24           # unit roundoff of fp32
C_EXP = 3.0                # ulps-of-exp allowance of the hardware exponential (alpha_terms)


def _t(a):
    return (a.detach().cpu() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a)))


def _f64(a):
    return _t(a).double()


def f32_exact(v) -> float:
    """a Python float as the C float the library receives"""
    return float(np.float32(v))


def check_le(got, ref, bound, mask=None):
    """(number of elements with |got - ref| > bound, worst |got - ref| / bound), over ``mask`` when given.  A zero bound demands equality."""
    err = (_f64(got) - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp(min=1e-300), torch.zeros_like(err))
    bad = ~(err <= bound)                                                  # (a NaN is bad)
    if mask is not None:
        m = mask.reshape(mask.shape + (1,) * (err.dim() - mask.dim())).expand_as(err)
        bad, ratio = bad & m, torch.where(m, ratio, torch.zeros_like(ratio))
    return int(bad.sum()), float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ alpha
def alpha_terms(x, c_exp=C_EXP):
    """(a, q, da, dq) for x = sigma dt >= 0: a = 1 - e^-x = -expm1(-x), q = e^-x, and the bounds of the fp32 alpha and of the fp32 1 - alpha.
    The kernel forms x' = fl(sigma dt) (relative error u, which moves e^-x by x e^-x u), scales it by log2(e) for the hardware exp2 (one more
    rounded product: another x e^-x u) and takes the hardware exponential, allowed c_exp u e^-x (c_exp = 3: about three ulps of exp, which also
    holds the 0.22 u relative error of the fp32 constant log2(e) for every x <= 20; beyond, e^-x is below u anyway).  The subtraction 1 - e
    rounds once: u a.  So |da| <= u ((c_exp + 2 x) e^-x + a) -- an ABSOLUTE term: for x < 2^-25 the fp32 alpha is 0 and its relative error is
    1.  q' = fl(1 - alpha') adds one rounding: dq = da + u q."""
    a, q = -torch.expm1(-x), torch.exp(-x)
    da = U32 * ((c_exp + 2 * x) * q + a)
    return a, q, da, da + U32 * q


# ------------------------------------------------------------------------------------------------ train branch
def composite_train_ref(sigmas, rgbs, deltas, rays, T_thresh, grad_ws=None, grad_image=None, c_exp=C_EXP):
    """k_composite_train_fwd and, when the cotangents are given, k_composite_train_bwd, in float64, with bounds.

    ``rays`` [N, 3] int = (ray id, first sample, sample count); M = len(sigmas); per-ray outputs are indexed by ray id, gradients by sample row.
    Per ray, x_i = sigma_i dt_i, a_i, q_i as in ``alpha_terms``; T_pre_k = prod_{i<k} q_i, T_post_k = T_pre_k q_k; the trip index is the first k
    with T_post_k < T_thresh; samples <= trip are composited with w_i = a_i T_pre_i; samples < trip own a gradient row.

    Forward bounds, by recursion over the composited samples (B_T = 0, every sum bound = 0 at the start):
      w' = fl(a' T'):                 B_w   = da T_pre + (a + da) B_T,pre + u w
      T' = fl(T' q'):                 B_T,k = B_T,k-1 (q_k + dq_k) + T_pre_k dq_k + u T_post_k
      ws' = fl(ws' + w'):             B_ws,k = B_ws,k-1 + B_w,k + u ws_k                       (ws_k the partial sum: all terms are >= 0)
      r' = fma(w', c, r') (one rounding of the new partial sum, whose magnitude is at most the running sum of |w c|):
                                      B_r,k = B_r,k-1 + B_w,k |c_k| + u sum_{i<=k} |w_i c_i|      (depth: the same with |t| for |c|)
    Backward, for an owning sample i (F the final colour / weights_sum the kernel reads back from the forward, p_i the partial colour sum
    including sample i, both recomputed with the forward's arithmetic):
      grad_rgb' = fl(g w'):           |g| (B_w + u w)
      term_ch = fma(T_post, c, -fl(F - p)):  B_term = B_T |c| + B_F + B_p + u |F - p| (the subtraction) + u (|T_post c| + |F - p|) (the fma)
      one' = fl(1 - ws_F):            B_one = B_ws,F + u |1 - ws_F|
      acc = g0 term0, then three fmas: B_acc = sum_ch |g_ch| B_term_ch + |g_ws| B_one + u (|s1| + |s2| + |s3| + |acc|), s_j the partial sums
      grad_sigma' = fl(dt acc'):      dt B_acc + u |dt acc|

    ``undecided`` (by ray id): at some composited step |T_post_k - T_thresh| <= B_T,k, so an fp32 kernel may legitimately trip one sample earlier
    or later than this reference; such rays are left out of the per-element check.

    Returns a namespace: weights_sum, depth, image and B_weights_sum, B_depth, B_image (by ray id), undecided, live (by ray id: the record is
    composited at all) and, with cotangents, grad_sigmas, grad_rgbs, B_grad_sigmas, B_grad_rgbs (by row), owned (by row: a live sample before its
    ray's trip writes this row; every other row must stay exactly 0) and row_undecided (by row: the row belongs to an undecided ray)."""
    sig, rgb, dl = _f64(sigmas), _f64(rgbs).reshape(-1, 3), _f64(deltas).reshape(-1, 2)
    rays = _t(rays).long()
    M, N = sig.shape[0], rays.shape[0]
    thr = f32_exact(T_thresh)
    rid, off, cnt = rays.unbind(1)
    live = (cnt > 0) & (off + cnt <= M)
    L = int(cnt[live].max()) if bool(live.any()) else 0
    steps = torch.arange(L)
    valid = live[:, None] & (steps[None] < cnt[:, None])                   # [N, L]
    idx = torch.where(valid, off[:, None] + steps[None], torch.zeros(1, dtype=torch.long))
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    if M > 0:
        x = torch.where(valid, sig[idx] * dl[idx, 0], z(1))
        dt, tt, col = dl[idx, 0], dl[idx, 1], rgb[idx]                     # [N, L], [N, L], [N, L, 3]
    else:
        x, dt, tt, col = z(N, 0), z(N, 0), z(N, 0), z(N, 0, 3)
    a, q, da, dq = alpha_terms(x, c_exp)

    T, BT, ws, Bws, d, Bd, md = torch.ones(N, dtype=torch.float64), z(N), z(N), z(N), z(N), z(N), z(N)
    c3, Bc3, mc3 = z(N, 3), z(N, 3), z(N, 3)
    alive, undec = live.clone(), torch.zeros(N, dtype=torch.bool)
    W, BW, TP, BTP, P, BP = z(N, L), z(N, L), z(N, L), z(N, L), z(N, L, 3), z(N, L, 3)
    owner = torch.zeros(N, L, dtype=torch.bool)
    for k in range(L):
        act = valid[:, k] & alive
        w = a[:, k] * T
        Bw = da[:, k] * T + (a[:, k] + da[:, k]) * BT + U32 * w
        Tn = T * q[:, k]
        BTn = BT * (q[:, k] + dq[:, k]) + T * dq[:, k] + U32 * Tn
        wsn = ws + w
        Bwsn = Bws + Bw + U32 * wsn
        ck, tk = col[:, k], tt[:, k]
        mdn, mc3n = md + (w * tk).abs(), mc3 + (w[:, None] * ck).abs()
        dn, Bdn = d + w * tk, Bd + Bw * tk.abs() + U32 * mdn
        c3n, Bc3n = c3 + w[:, None] * ck, Bc3 + Bw[:, None] * ck.abs() + U32 * mc3n
        a1, a3 = act, act[:, None]
        T, BT, ws, Bws = torch.where(a1, Tn, T), torch.where(a1, BTn, BT), torch.where(a1, wsn, ws), torch.where(a1, Bwsn, Bws)
        d, Bd, md = torch.where(a1, dn, d), torch.where(a1, Bdn, Bd), torch.where(a1, mdn, md)
        c3, Bc3, mc3 = torch.where(a3, c3n, c3), torch.where(a3, Bc3n, Bc3), torch.where(a3, mc3n, mc3)
        undec |= act & ((Tn - thr).abs() <= BTn)
        trip = act & (Tn < thr)
        owner[:, k] = act & ~trip
        alive &= ~trip
        W[:, k], BW[:, k], TP[:, k], BTP[:, k], P[:, k], BP[:, k] = w, Bw, Tn, BTn, c3n, Bc3n

    out = SimpleNamespace(live=torch.zeros(N, dtype=torch.bool), undecided=torch.zeros(N, dtype=torch.bool))
    out.live[rid], out.undecided[rid] = live, undec
    for name, v, b in (("weights_sum", ws, Bws), ("depth", d, Bd), ("image", c3, Bc3)):
        o, ob = torch.zeros_like(v), torch.zeros_like(b)
        o[rid], ob[rid] = v, b
        setattr(out, name, o)
        setattr(out, "B_" + name, ob)
    if grad_ws is None:
        return out

    g3, gw = _f64(grad_image).reshape(-1, 3)[rid], _f64(grad_ws)[rid]     # per record, read by ray id
    rem = c3[:, None, :] - P                                               # F - p_i  [N, L, 3]
    term = TP[..., None] * col - rem
    Bterm = BTP[..., None] * col.abs() + Bc3[:, None, :] + BP + U32 * ((TP[..., None] * col).abs() + 2 * rem.abs())
    one = 1.0 - ws
    Bone = Bws + U32 * one.abs()
    gt = g3[:, None, :] * term
    s1, s2, s3 = gt[..., 0], gt[..., 0] + gt[..., 1], gt.sum(-1)
    acc = s3 + (gw * one)[:, None]
    Bacc = (g3.abs()[:, None, :] * Bterm).sum(-1) + (gw.abs() * Bone)[:, None] + U32 * (s1.abs() + s2.abs() + s3.abs() + acc.abs())
    gs, Bgs = dt * acc, dt.abs() * Bacc + U32 * (dt * acc).abs()
    gc, Bgc = g3[:, None, :] * W[..., None], g3.abs()[:, None, :] * (BW + U32 * W)[..., None]
    rows = idx[owner]
    out.grad_sigmas, out.B_grad_sigmas, out.grad_rgbs, out.B_grad_rgbs = z(M), z(M), z(M, 3), z(M, 3)
    out.owned, out.row_undecided = torch.zeros(M, dtype=torch.bool), torch.zeros(M, dtype=torch.bool)
    out.grad_sigmas[rows], out.B_grad_sigmas[rows] = gs[owner], Bgs[owner]
    out.grad_rgbs[rows], out.B_grad_rgbs[rows] = gc[owner], Bgc[owner]
    out.owned[rows] = True
    out.row_undecided[idx[valid & undec[:, None]]] = True
    return out


# ------------------------------------------------------------------------------------------------ inference branch
def composite_rays_ref(n_alive, n_step, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, T_thresh, c_exp=C_EXP):
    """k_composite_rays in float64, with bounds.  Alive ray n (id = rays_alive[n]) owns slots [n n_step, (n + 1) n_step).  It differs from the train
    branch: the transmittance is T = 1 - weights_sum taken BEFORE the sample and tested against the threshold AFTER the sample was added; the sums
    continue from the incoming weights_sum / depth / image (exact fp32 values: bound 0 at the start); the ray stops at the first slot with dt == 0.
    A ray that stopped before its last slot was passed gets alive flag -1; otherwise rays_t[id] = fl32(t_last + dt_last), one fp32 addition of two
    inputs, so that value is bit-exact.

      T' = fl(1 - ws'):          B_T = B_ws + u T
      w' = fl(a' T'):            B_w = da T + (a + da) B_T + u w
      ws' = fl(ws' + w'):        B_ws <- B_ws + B_w + u ws_new
      r' = fma(w', c, r'):       B_r <- B_r + B_w |c| + u (|r_in| + running sum of |w c|)          (depth: |t| for |c|)

    ``undecided``: at some processed step |T - T_thresh| <= B_T.  Returns a namespace: rays_alive (int64 [n_alive]), rays_t (fp32, all rays),
    weights_sum, depth, image, B_* (all rays; rays not in the alive list keep their input and a zero bound), undecided and touched (all rays)."""
    na, ns = int(n_alive), int(n_step)
    ids = _t(rays_alive).long()[:na]
    sig = _f64(sigmas).reshape(-1)[:na * ns].reshape(na, ns)
    col = _f64(rgbs).reshape(-1, 3)[:na * ns].reshape(na, ns, 3)
    dl32 = _t(deltas).float().reshape(-1, 2)[:na * ns].reshape(na, ns, 2)
    dl = dl32.double()
    thr = f32_exact(T_thresh)
    ws_all, d_all, c_all = _f64(weights_sum).clone(), _f64(depth).clone(), _f64(image).reshape(-1, 3).clone()
    ws, d, c3 = ws_all[ids], d_all[ids], c_all[ids]
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    Bws, Bd, Bc3, md, mc3 = z(na), z(na), z(na, 3), d.abs(), c3.abs()
    run, early, undec = torch.ones(na, dtype=torch.bool), torch.zeros(na, dtype=torch.bool), torch.zeros(na, dtype=torch.bool)
    a, q, da, dq = alpha_terms(sig * dl[..., 0], c_exp)
    for k in range(ns):
        empty = run & (dl[:, k, 0] == 0)
        early |= empty
        run = run & ~empty
        act = run
        T = 1.0 - ws
        BT = Bws + U32 * T.abs()
        w = a[:, k] * T
        Bw = da[:, k] * T.abs() + (a[:, k] + da[:, k]) * BT + U32 * w.abs()
        wsn = ws + w
        Bwsn = Bws + Bw + U32 * wsn.abs()
        ck, tk = col[:, k], dl[:, k, 1]
        mdn, mc3n = md + (w * tk).abs(), mc3 + (w[:, None] * ck).abs()
        dn, Bdn = d + w * tk, Bd + Bw * tk.abs() + U32 * mdn
        c3n, Bc3n = c3 + w[:, None] * ck, Bc3 + Bw[:, None] * ck.abs() + U32 * mc3n
        a1, a3 = act, act[:, None]
        ws, Bws = torch.where(a1, wsn, ws), torch.where(a1, Bwsn, Bws)
        d, Bd, md = torch.where(a1, dn, d), torch.where(a1, Bdn, Bd), torch.where(a1, mdn, md)
        c3, Bc3, mc3 = torch.where(a3, c3n, c3), torch.where(a3, Bc3n, Bc3), torch.where(a3, mc3n, mc3)
        undec |= act & ((T - thr).abs() <= BT)
        trip = act & (T < thr)
        early |= trip
        run = run & ~trip
    out = SimpleNamespace()
    out.rays_alive = torch.where(early, torch.full_like(ids, -1), ids)
    out.rays_t = _t(rays_t).float().clone()
    done = ~early
    out.rays_t[ids[done]] = dl32[done, ns - 1, 1] + dl32[done, ns - 1, 0]  # one fp32 addition
    n_rays = ws_all.shape[0]
    out.undecided, out.touched = torch.zeros(n_rays, dtype=torch.bool), torch.zeros(n_rays, dtype=torch.bool)
    out.undecided[ids], out.touched[ids] = undec, True
    ws_all[ids], d_all[ids], c_all[ids] = ws, d, c3
    out.weights_sum, out.depth, out.image = ws_all, d_all, c_all
    out.B_weights_sum, out.B_depth, out.B_image = z(n_rays), z(n_rays), z(n_rays, 3)
    out.B_weights_sum[ids], out.B_depth[ids], out.B_image[ids] = Bws, Bd, Bc3
    return out


# ------------------------------------------------------------------------------------------------ DDIM step
def ddim_step_ref(x_t, v, a, b, c, d, lo, hi):
    """The DDIM step (k_step_v<0, false, false>) in float64, with bounds: p = clamp(a x_t - b v, lo, hi), eps = (x_t - a p) / b, x_prev = c p + d eps; the coefficients as the
    C floats the library receives.
      p:      two products and a subtraction (or a product and an fma), each rounding at most u times one of the two magnitudes, twice at most:
              B_p = 2 u (|a x_t| + |b v|).  The clamp is 1-Lipschitz and monotone, and lo / hi are exact: it carries B_p and needs no exclusion.
      eps:    the kernel multiplies fl(x_t - fl(a p')) by the fp32 reciprocal fl(1 / b): B_eps = (|a| B_p + 2 u (|x_t| + |a p|)) / b + 2 u |eps| --
              the cancellation in x_t - a p is paid for by the 1 / b in front of the absolute terms, not by a relative bound.
      x_prev: B = |c| B_p + |d| B_eps + 2 u (|c p| + |d eps|).
    Returns (p, B_p, x_prev, B_xprev) as float64."""
    x, vv = _f64(x_t), _f64(v)
    a, b, c, d, lo, hi = (f32_exact(s) for s in (a, b, c, d, lo, hi))
    p0 = a * x - b * vv
    Bp = 2 * U32 * ((a * x).abs() + (b * vv).abs())
    p = p0.clamp(lo, hi)
    eps = (x - a * p) / b
    Beps = (abs(a) * Bp + 2 * U32 * (x.abs() + (a * p).abs())) / abs(b) + 2 * U32 * eps.abs()
    xp = c * p + d * eps
    Bxp = abs(c) * Bp + abs(d) * Beps + 2 * U32 * ((c * p).abs() + (d * eps).abs())
    return p, Bp, xp, Bxp


# ------------------------------------------------------------------------------------------------ seeded input families
FAMILIES = ("wide", "thin", "vanishing", "opaque")
THRESHOLDS = (1e-4, 1e-2)
RAY_COUNTS = (1, 255, 256, 257, 4097)     # one ray; one short of, exactly and one past a block of 256; 16 blocks and one ray
FIXED_COUNTS = (65, 1, 0, 2, 64, 255, 256)  # the sample counts of the first records of every case (a single ray gets 65)
MAX_UNDECIDED = 0.005                     # the share of rays a case may leave out of the per-element check
DT0 = 2 * 3 ** 0.5 / 256                  # the step of a 256-step march through the unit cube's diagonal


def _sigmas(rng, family, dt, first, last, n):
    """densities of ``n`` samples with steps ``dt``; ``first`` / ``last``: the [start, end) rows of every non-empty ray, for the opaque family"""
    if family == "wide":
        return np.exp(rng.normal(1.0, 2.0, n))
    if family in ("thin", "vanishing"):
        s = np.exp(rng.normal(-6.0, 2.0, n))
        if family == "vanishing":                                           # a tenth at sigma dt in [2^-30, 2^-24], a fiftieth exactly 0
            pick = rng.random(n)
            tiny = 2.0 ** rng.uniform(-30, -24, n) / np.maximum(dt, 1e-30)
            s = np.where(pick < 0.1, tiny, s)
            s = np.where(pick > 0.98, 0.0, s)
        return s
    if family == "opaque":
        s = np.exp(rng.normal(-2.0, 1.0, n))
        where = rng.integers(0, 3, len(first))                              # 0: the first sample, 1: the last, 2: anywhere
        pos = np.where(where == 0, first, np.where(where == 1, last - 1, rng.integers(first, np.maximum(last, first + 1))))
        s[pos] = 1e4
        return s
    raise ValueError(family)


def train_case(family, n_rays, seed, pad=32, n_overflow=3):
    """packed ray records as the train branch reads them, drawn directly (no march): sample counts in [0, 256] with ``FIXED_COUNTS`` first, ray
    ids a random permutation of the records, offsets handed out in another shuffled order (a ray's samples are contiguous, rays are not in order),
    dt = DT0 U(0.5, 2) with t its running sum, ``pad`` unowned rows at the end and, from 16 rays on, ``n_overflow`` records moved so that
    off + cnt > M (their former rows are owned by nobody).  Returns a namespace of numpy arrays: sigmas [M], rgbs [M, 3], deltas [M, 2],
    rays [N, 3] int32, grad_ws [N], grad_image [N, 3] (by ray id), M."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 257, n_rays)
    k = min(len(FIXED_COUNTS), n_rays)
    cnt[:k] = FIXED_COUNTS[:k]
    order = rng.permutation(n_rays)
    off = np.zeros(n_rays, np.int64)
    off[order] = np.cumsum(cnt[order]) - cnt[order]
    total = int(cnt.sum())
    M = total + pad
    ray_of = np.repeat(order, cnt[order])                                   # the record that owns each of the first ``total`` rows
    dt = np.zeros(M)
    dt[:total] = DT0 * rng.uniform(0.5, 2.0, total)
    dt = dt.astype(np.float32).astype(np.float64)
    run = np.cumsum(dt[:total]) - dt[:total]
    t = np.zeros(M)
    t[:total] = rng.uniform(0.2, 1.5, n_rays)[ray_of] + run - run[off[ray_of]] if total else 0.0
    some = cnt > 0
    sig = np.zeros(M)
    sig[:total] = _sigmas(rng, family, dt[:total], off[some], (off + cnt)[some], total)
    sig[total:] = 1.0                                                       # padding rows hold plausible values: reading them would show
    rgb = rng.random((M, 3))
    ids = rng.permutation(n_rays)
    if n_rays >= 16:
        cand = np.flatnonzero(cnt[len(FIXED_COUNTS):] >= 2)[:n_overflow] + len(FIXED_COUNTS)
        for j, r in enumerate(cand):
            off[r] = M - cnt[r] + 1 + j
    rays = np.stack([ids, off, cnt], 1).astype(np.int32)
    return SimpleNamespace(family=family, M=M, sigmas=sig.astype(np.float32), rgbs=rgb.astype(np.float32),
                           deltas=np.stack([dt, t], 1).astype(np.float32), rays=rays,
                           grad_ws=rng.normal(size=n_rays).astype(np.float32), grad_image=rng.normal(size=(n_rays, 3)).astype(np.float32))


def infer_case(family, n_step, T_thresh, seed, n_alive=1025, n_rays=3000):
    """inputs of one ``composite_rays`` call: ``n_alive`` ids out of ``n_rays`` in random order, ``n_step`` slots each; a third of the rays have an
    unused slot (dt == 0) at position 0, a third in the middle (the slots after it hold live-looking values), a third nowhere; incoming
    weights_sum uniform over [0, 1) with a third of the rays within 1e-3 of 1 - T_thresh on either side; incoming depth and image non-zero."""
    rng = np.random.default_rng(seed)
    n = n_alive * n_step
    alive = rng.permutation(n_rays)[:n_alive].astype(np.int32)
    dt = (DT0 * rng.uniform(0.5, 2.0, (n_alive, n_step))).astype(np.float32)
    hole = rng.integers(0, 3, n_alive)                                      # 0: slot 0, 1: the middle slot, 2: none
    dt[hole == 0, 0] = 0.0
    dt[hole == 1, n_step // 2] = 0.0
    t = (rng.uniform(0.2, 1.5, (n_alive, 1)) + np.cumsum(dt, 1) - dt).astype(np.float32)
    rows = np.arange(n_alive) * n_step
    sig = _sigmas(rng, family, dt.reshape(-1).astype(np.float64), rows, rows + n_step, n).astype(np.float32)
    ws = rng.random(n_rays)
    near = rng.random(n_rays) < 1 / 3
    ws = np.where(near, 1 - f32_exact(T_thresh) + rng.uniform(-1e-3, 1e-3, n_rays), ws).clip(0, 1 - 2.0 ** -24).astype(np.float32)
    return SimpleNamespace(family=family, n_alive=n_alive, n_step=n_step, n_rays=n_rays, rays_alive=alive,
                           rays_t=rng.uniform(0.2, 3.0, n_rays).astype(np.float32), sigmas=sig, rgbs=rng.random((n, 3)).astype(np.float32),
                           deltas=np.stack([dt, t], -1).reshape(n, 2), weights_sum=ws, depth=rng.uniform(0, 2, n_rays).astype(np.float32),
                           image=rng.random((n_rays, 3)).astype(np.float32))


DDIM_SIZES = (4, 1028, 4 * (2048 * 256 + 3))    # one float4; a ragged last block; one float4 group past a full grid of 2048 x 256 lanes


def ddim_coefficients():
    """(name, a, b, c, d) of the project's own linear 1000-step schedule: the first step of the 50-step DDIM plan (a ~ 0.006, b ~ 1), a middle one,
    its last (b ~ 0.08), and the last two of the 1000-step plan (b ~ 0.015 and b = 0.01, where x_t - a p cancels most)"""
    from ssdnerf_amd.diffusion import NoiseSchedule, SamplingPlan
    sched = NoiseSchedule(dict(type="linear"), 1000)
    p50, p1000 = SamplingPlan(sched, "ddim", 50).steps, SamplingPlan(sched, "ddim", 1000).steps
    pick = [("first", p50[0]), ("middle", p50[25]), ("last-of-50", p50[-1]), ("late", p1000[-2]), ("last", p1000[-1])]
    return [(n, s.a, s.b, s.c, s.d) for n, s in pick]


def ddim_case(n, seed):
    """(x_t, v): unit normals, so that p = a x_t - b v leaves [-1, 1] at either end for about a sixth of the elements each"""
    rng = np.random.default_rng(seed)
    return rng.normal(size=n).astype(np.float32), rng.normal(size=n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cases with their references, and the checks
@functools.lru_cache(maxsize=None)
def train_reference(family, n_rays, T_thresh, n_overflow=3):
    """(case, reference) of one seeded train-branch case; computed once per process and shared (treat both as read-only)"""
    c = train_case(family, n_rays, seed=FAMILIES.index(family) * 10 + n_rays, n_overflow=n_overflow)
    return c, composite_train_ref(c.sigmas, c.rgbs, c.deltas, c.rays, T_thresh, c.grad_ws, c.grad_image)


@functools.lru_cache(maxsize=None)
def infer_reference(family, n_step, T_thresh):
    c = infer_case(family, n_step, T_thresh, seed=100 + FAMILIES.index(family) * 10 + n_step)
    return c, composite_rays_ref(c.n_alive, c.n_step, c.rays_alive, c.rays_t, c.sigmas, c.rgbs, c.deltas, c.weights_sum, c.depth, c.image, T_thresh)


def _bits(a):
    return _t(a).float().contiguous().view(torch.int32)


def train_failures(got, ref):
    """{output: (elements outside their bound, worst error / bound)} of a dict of train-branch results.  Per-ray outputs and gradient rows of
    decided rays against their bounds; "unowned": gradient rows of decided rays that no live sample before the trip owns and that are not
    exactly 0; "sane": rays, undecided ones included, whose outputs are not finite or whose weights_sum leaves [0, 1 + B_ws]."""
    dec, row_dec = ~ref.undecided, ~ref.row_undecided
    res = {k: check_le(got[k], getattr(ref, k), getattr(ref, "B_" + k), dec) for k in ("weights_sum", "depth", "image")}
    res.update({k: check_le(got[k], getattr(ref, k), getattr(ref, "B_" + k), row_dec & ref.owned) for k in ("grad_sigmas", "grad_rgbs")})
    unowned = ~ref.owned & row_dec
    res["unowned"] = (int((_t(got["grad_sigmas"])[unowned] != 0).sum() + (_t(got["grad_rgbs"])[unowned] != 0).sum()), 0.0)
    ws = _f64(got["weights_sum"])
    finite = all(bool(torch.isfinite(_f64(got[k])).all()) for k in ("weights_sum", "depth", "image", "grad_sigmas", "grad_rgbs"))
    res["sane"] = (int(((ws < 0) | (ws > 1 + ref.B_weights_sum)).sum()) + (0 if finite else 1), 0.0)
    return res


def infer_failures(got, ref, c):
    """the same for ``composite_rays``: outputs of decided rays against their bounds; alive flags and rays_t of decided rays exact (rays_t bit for
    bit); "untouched": values of rays outside the alive list that differ from what came in, bit for bit; "sane" as for the train branch."""
    dec = ~ref.undecided
    res = {k: check_le(got[k], getattr(ref, k), getattr(ref, "B_" + k), dec) for k in ("weights_sum", "depth", "image")}
    dec_alive = dec[_t(c.rays_alive).long()[:c.n_alive]]
    res["rays_alive"] = (int(((_t(got["rays_alive"]).long()[:c.n_alive] != ref.rays_alive) & dec_alive).sum()), 0.0)
    res["rays_t"] = (int(((_bits(got["rays_t"]) != _bits(ref.rays_t)) & dec).sum()), 0.0)
    untouched = ~ref.touched
    res["untouched"] = (sum(int((_bits(got[k])[untouched] != _bits(getattr(c, k))[untouched]).sum()) for k in ("weights_sum", "depth", "image", "rays_t")), 0.0)
    ws = _f64(got["weights_sum"])
    finite = all(bool(torch.isfinite(_f64(got[k])).all()) for k in ("weights_sum", "depth", "image", "rays_t"))
    res["sane"] = (int(((ws < 0) | (ws > 1 + ref.B_weights_sum)).sum()) + (0 if finite else 1), 0.0)
    return res


def n_failures(res) -> int:
    return sum(v[0] for v in res.values())
