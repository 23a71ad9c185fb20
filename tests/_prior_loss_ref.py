"""References of the prior-loss kernels (ssdnerf_amd/csrc/prior_loss.hip; ``GaussianDiffusion.forward_train`` with ``noise_source='device'``):
the kernels' own fp32 operations restated in numpy float32, in the kernels' order, and float64 references with first-order worst-case bounds.
Both test modules draw from here: tests/test_prior_loss_cpu.py proves the bounds on fp32 emulations (they accept two summation orders and reject six
wrong formulas) and tests/test_prior_loss_gpu.py holds the kernels to them.

As in tests/_philox_ref.py, every input (an fp32 tensor, a coefficient array, the kernel's own z read back from the fill, the k array handed to the
backward) is taken as the exact value the kernel read; u = 2^-24 is the unit roundoff of fp32; the library is built with -ffp-contract=off, so every
product and sum rounds once.  No constant is fitted to the kernels.

THE ELEMENT.  The kernels compute  diff' = fl(pred - fl(fl(a z) - fl(b x0))).  With d the float64 diff:
    fl(a z) = a z (1 + e1),  fl(b x0) = b x0 (1 + e2),  target' = (fl(a z) - fl(b x0)) (1 + e3),  diff' = (pred - target') (1 + e4),  |e| <= u
    |target' - target| <= u (|a z| + |b x0|) + u |a z - b x0| + O(u^2)
    |diff' - d|        <= u (|a z| + |b x0| + |a z - b x0| + |d|) + O(u^2)  =: delta        (pred is exact: a bf16 value widens exactly)
The O(u^2) terms are products of two of the four roundings, each below u times a first-order term: under the factor (1 + 8 u).

THE MEANS.  fl(diff'^2) = diff'^2 (1 + e); the kernel adds the squares along a tree whose longest chain of additions has m members
(``chain_length``), and divides once by n_per (in double, rounded once): for non-negative terms the result is  mean(diff'^2) (1 + theta),
|theta| <= gamma_(m+2) = (m + 2) u / (1 - (m + 2) u), whatever the order.  |diff'^2 - d^2| <= 2 |d| delta + delta^2.  Hence
    |msd' - msd64| <= (1 / n_per) sum_i (2 |d_i| delta_i + delta_i^2) + (m + 2) u msd64,
and what this leaves out -- gamma against (m + 2) u, and (m + 2) u times the first term -- is below 2^-17 of either term for m + 2 <= 128: the factor
(1 + 2^-16).  x0sq alike, with delta = 0:  |x0sq' - x0sq64| <= (m + 2) u x0sq64.

THE GRADIENT.  g' = fl(k diff'), against g = k d (what float64 autograd of the eager formula gives for the upstream gradient k n_per / 2):
    |g' - g| <= |k| delta + u |g| (1 + ...):  one rounding; the bound allows two (2 u |g|).  A bf16 output adds half a bf16 ulp at |g| + that bound.
    grad_x0' = fl(g' b):   |grad_x0' - g b| <= |b| (|k| delta + u |g|) + u |g b|.

Nothing here needs a GPU."""
import numpy as np
import torch

import _philox_ref as PR
from _composite_ref import U32, _f64, check_le  # noqa: F401  (check_le: used by the test modules through this one)

SLACK2 = 1 + 8 * U32                                                        # the O(u^2) terms of an element
SHAPES = ((1, 4), (2, 8), (3, 1020), (2, 1024), (3, 4100))                  # (B, n_per); the test modules add the shape beyond the block cap


def shapes(cap):
    """... and one whose per-sample block count exceeds ``cap`` blocks of 256 float4 lanes by one float4: the grid-stride loop's second trip has a
    single lane at work"""
    return SHAPES + ((2, 4 * (256 * cap + 1)),)


def blocks_per_sample(n_per, cap):
    """what ``ssdnerf_prior_blocks_per_sample`` returns (the CPU tests have no library to ask)"""
    return min((n_per // 4 + 255) // 256, cap)


def chain_length(n_per, bps):
    """m: the longest chain of additions from a square to its sample's sum -- 4 per trip of the lane's grid-stride loop (ceil(n4 / (256 bps)) trips),
    6 butterfly stages in the wave, 3 to add the block's four waves, ceil(bps / 64) per lane of the finishing wave, 6 butterfly stages there"""
    n4 = n_per // 4
    trips = -(-n4 // (256 * bps))
    return 4 * trips + 6 + 3 + -(-bps // 64) + 6


def normals32(seed, draw, n):
    """the float64 restatement's normals rounded to fp32: what stands in for the fill where there is no device (test_sde_cpu does the same)"""
    return PR.normals(PR.quad_words(seed, draw, 0, n // 4)).astype(np.float32)


def case(B, n_per, seed, schedule=None, timesteps=None):
    """(pred, x0, a, b, k): unit normals for pred and x0, the schedule's fp32 coefficients at ``timesteps`` (or generic ones), k of the size 2 G / n_per"""
    rng = np.random.default_rng(seed)
    pred, x0 = (rng.normal(size=(B, n_per)).astype(np.float32) for _ in range(2))
    if schedule is None:
        a = rng.uniform(0.05, 1.0, B)
        a, b = a.astype(np.float32), np.sqrt(1 - a * a).astype(np.float32)
    else:
        t = np.asarray(timesteps).reshape(-1)
        a, b = (np.asarray(schedule[k], np.float64)[t].astype(np.float32) for k in ("sqrt_alphas_bar", "sqrt_one_minus_alphas_bar"))
    k = (rng.uniform(0.25, 2.0, B) * rng.choice([-1.0, 1.0], B) * 2 / n_per).astype(np.float32)
    return pred, x0, a, b, k


# ------------------------------------------------------------------------------------------------ the fp32 restatement
def _col(v):
    return np.asarray(v, np.float32).reshape(-1, 1)


def q_sample32(x0, z, a, b):
    """fl(fl(x0 a) + fl(z b))"""
    x0, z = np.asarray(x0, np.float32), np.asarray(z, np.float32).reshape(np.shape(x0))
    return x0 * _col(a) + z * _col(b)


def diff32(pred, x0, z, a, b):
    """fl(pred - fl(fl(a z) - fl(b x0))); ``pred``: fp32 values (a bf16 prediction widened)"""
    x0, z = np.asarray(x0, np.float32), np.asarray(z, np.float32).reshape(np.shape(x0))
    return np.asarray(pred, np.float32) - (_col(a) * z - _col(b) * x0)


def target32(x0, z, a, b):
    x0, z = np.asarray(x0, np.float32), np.asarray(z, np.float32).reshape(np.shape(x0))
    return _col(a) * z - _col(b) * x0


def backward32(pred, x0, z, a, b, k):
    """(grad_pred, grad_x0) = (fl(k diff), fl(fl(k diff) b)) in fp32"""
    g = _col(k) * diff32(pred, x0, z, a, b)
    return g, g * _col(b)


def _sum32(v, order):
    v = np.asarray(v, np.float32)
    if order == "sequential":
        acc = np.zeros(v.shape[0], np.float32)
        for j in range(v.shape[1]):
            acc = acc + v[:, j]
        return acc
    while v.shape[1] > 1:                                                     # 'pairwise': neighbours, an odd one carried
        odd = v[:, -1:] if v.shape[1] % 2 else None
        v = v[:, 0:v.shape[1] - (v.shape[1] % 2):2] + v[:, 1::2]
        v = v if odd is None else np.concatenate([v, odd], 1)
    return v[:, 0]


def mean_sq32(v, order):
    """mean of squares per row in fp32: every square rounds, the sum in ``order`` ('sequential' or 'pairwise'), one division"""
    v = np.asarray(v, np.float32)
    return _sum32(v * v, order) / np.float32(v.shape[1])


def emulation_chain(n_per, order):
    """the m of ``mean_sq32``'s own tree (what the CPU test hands ``loss_ref`` in place of the kernel's)"""
    return n_per - 1 if order == "sequential" else int(np.ceil(np.log2(max(n_per, 2))))


# ------------------------------------------------------------------------------------------------ float64 and the bounds
def element_ref(pred, x0, z, a, b):
    """(d, delta) as float64 tensors (B, n_per): THE ELEMENT above"""
    p, x, zz = _f64(pred), _f64(x0), _f64(z).reshape(np.shape(x0))
    aa, bb = _f64(a).reshape(-1, 1), _f64(b).reshape(-1, 1)
    az, bx = aa * zz, bb * x
    d = p - (az - bx)
    return d, U32 * (az.abs() + bx.abs() + (az - bx).abs() + d.abs()) * SLACK2


def loss_ref(pred, x0, z, a, b, m):
    """(msd, B_msd, x0sq, B_x0sq), float64 (B,): THE MEANS above; ``m`` the chain length of whatever sums"""
    assert m + 2 <= 128
    d, delta = element_ref(pred, x0, z, a, b)
    msd = (d * d).mean(1)
    x0sq = (_f64(x0) ** 2).mean(1)
    slack = 1 + 2.0 ** -16
    return msd, ((2 * d.abs() * delta + delta * delta).mean(1) + (m + 2) * U32 * msd) * slack, x0sq, (m + 2) * U32 * x0sq * slack


def ulp_bf16(v):
    """spacing of bf16 (8 significant bits) at the float64 magnitudes ``v``"""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return torch.from_numpy(np.ldexp(1.0, np.maximum(e, -125) - 8))


def backward_ref(pred, x0, z, a, b, k, bf16=False):
    """(grad_pred, B, grad_x0, B), float64 (B, n_per): THE GRADIENT above.  grad_pred is float64 AUTOGRAD of the eager formula
    sum_s G_s mean_i (pred - (a z - b x0))^2 with G_s = k_s n_per / 2, with respect to pred and -- through the target alone -- to x0."""
    p, x = _f64(pred).requires_grad_(True), _f64(x0).requires_grad_(True)
    zz, aa, bb, kk = _f64(z).reshape(np.shape(x0)), _f64(a).reshape(-1, 1), _f64(b).reshape(-1, 1), _f64(k).reshape(-1, 1)
    n_per = p.shape[1]
    loss = ((kk[:, 0] * n_per / 2) * (p - (aa * zz - bb * x)).square().mean(1)).sum()
    g, gx = torch.autograd.grad(loss, (p, x))
    _, delta = element_ref(pred, x0, z, a, b)
    Bg = (kk.abs() * delta + 2 * U32 * g.abs()) * SLACK2
    Bx = (bb.abs() * (kk.abs() * delta + U32 * g.abs()) + U32 * gx.abs()) * SLACK2
    if bf16:
        Bg = Bg + 0.5 * ulp_bf16((g.abs() + Bg).numpy())
    return g, Bg, gx, Bx


# ------------------------------------------------------------------------------------------------ the whole chain with the analytic denoiser
def gaussian_chain_ref(x0, z, t, schedule, mu, s, x_t_detach, m):
    """The prior loss of ``forward_train`` with ``_dpmpp_ref.GaussianDenoiser(schedule, mu, s)`` as the network, default ``DDPMMSELoss`` (no timestep
    weights, reduction 'mean'): loss = mean_s 0.5 msd_s.  Float64 on the kernel's z; returns (loss, B_loss, grad_x0, B_grad).
    The chain, per element (a, b: the fp32 coefficients the kernels read; A, Bn: the denoiser's float64 tables):
      x_t' = fl(fl(x0 a) + fl(z b)):                 |x_t' - x_t| <= u (|a x0| + |b z| + |x_t|) =: e_x
      v    = L x_t + c,  L = (A - K) / Bn,  K = A s^2 / (A^2 s^2 + Bn^2),  c = (K A mu - mu) / Bn, evaluated by the denoiser in float64 on x_t' and
             rounded to fp32:                        |v' - v| <= |L| e_x + u |v| =: e_v             (its float64 roundings: 2^-29 of these)
      diff' = THE ELEMENT with pred = v':            |diff' - d| <= e_v + delta =: e_d
      msd:   THE MEANS with e_d for delta;  loss' = fl(mean_s fl(0.5 msd_s)): 0.5 is exact, a mean of B terms rounds at most B + 1 times:
             B_loss = mean_s 0.5 B_msd_s + (B + 1) u loss.
      k_s = fl(fl(0.5 / B) fl(2 / n_per)) is taken as read (``chain_k``); g' = fl(k diff'):  e_g = |k| e_d + u |g|
      grad through the target: fl(g' b): |b| e_g + u |g b|;  through x_t (not with x_t_detach): the denoiser's backward is fl(L g') (float64 product, one
      rounding to fp32): |L| e_g + u |L g|, then fl(. a): + u |a L g|; the two paths are added once: + u |total|.
    All under (1 + 8 u) for the second order."""
    x, zz = _f64(x0), _f64(z).reshape(np.shape(x0))
    B, n_per = x.shape[0], x[0].numel()
    x, zz = x.reshape(B, -1), zz.reshape(B, -1)
    t = np.asarray(t).reshape(-1)
    A, Bn = (torch.from_numpy(np.asarray(schedule[k], np.float64)[t]).reshape(-1, 1) for k in ("sqrt_alphas_bar", "sqrt_one_minus_alphas_bar"))
    a, b = A.float().double(), Bn.float().double()
    K = A * s * s / (A * A * s * s + Bn * Bn)
    L, c = (A - K) / Bn, (K * A * mu - mu) / Bn
    x_t = a * x + b * zz
    e_x = U32 * ((a * x).abs() + (b * zz).abs() + x_t.abs())
    v = L * x_t + c
    e_v = L.abs() * e_x + U32 * v.abs()
    d, delta = element_ref(v, x, zz, a, b)
    e_d = (e_v + delta) * SLACK2
    assert m + 2 <= 128
    msd =(d * d).mean(1)
    B_msd = ((2 * d.abs() * e_d + e_d * e_d).mean(1) + (m + 2) * U32 * msd) * (1 + 2.0 ** -16)
    loss = (0.5 * msd).mean()
    B_loss = (0.5 * B_msd).mean() + (B + 1) * U32 * loss
    k = float(chain_k(B, n_per))
    g = k * d
    e_g = abs(k) * e_d + U32 * g.abs()
    grad = g * b
    Bgrad = b.abs() * e_g + U32 * grad.abs()
    if not x_t_detach:
        through = a * L * g
        Bgrad = Bgrad + a.abs() * (L.abs() * e_g + U32 * (L * g).abs()) + U32 * through.abs()
        grad = grad + through
        Bgrad = Bgrad + U32 * grad.abs()
    return loss, B_loss * SLACK2, grad, Bgrad * SLACK2


def chain_k(B, n_per):
    """k_s as the loss's backward forms it for loss = mean_s 0.5 msd_s: the gradient arriving at msd_s is fl(0.5 fl(1 / B)) (autograd of a mean, then of
    the exact product with 0.5), times fl(2 / n_per), one rounding"""
    return np.float32(np.float32(0.5) * (np.float32(1.0) / np.float32(B))) * np.float32(2.0 / n_per)
