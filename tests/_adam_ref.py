"""float64 restatement of ONE Adam step (torch.optim.Adam, amsgrad=False, maximize=False: csrc/adam_math.h) and per-element error bounds for an
fp32 evaluation of it, shared by tests/test_adam_cpu.py (a gcc build of the header and torch's own CPU Adam meet the bounds; wrong variants
do not) and tests/test_adam_gpu.py (the kernel meets them).  Nothing here needs a GPU: everything is numpy.

The reference is computed in float64 from the exact fp32 values the step read (param, grad, exp_avg, exp_avg_sq) and from the hyper-parameters
as Python floats -- the scalars an fp32 implementation receives are roundings of those, and the bounds count that rounding.

With u = 2^-24, every fp32 operation returns x (1 + d), |d| <= u, and so does every scalar passed as float.  Write
    G  = g + wd p                        A = |g| + wd |p|      (the magnitudes the sum rounds; with wd == 0, G = g exactly and A = |g|)
    M' = m + (G - m) w1                  w1 = 1 - beta1
    V' = v beta2 + w2 G^2                w2 = 1 - beta2
    D  = sqrt(V') / c + eps              c = sqrt(1 - beta2^step)
    P' = p - s M' / D                    s = lr / (1 - beta1^step)
Errors of the computed values, to first order in u (second-order terms are ~ 10^-7 of the bounds; one spare u on |s M' / D| covers them):

  e_G <= K u A, K = 3 with weight decay (wd as float, the product, the sum), K = 0 without.
        This must be counted against A, not |G|: where g and wd p cancel, the computed G carries an error of u A however small G is.

  exp_avg:     G - m rounds once on top of e_G; (.) w1 rounds twice (w1 as float, the product); m + (.) rounds once:
        e_M <= w1 (e_G + u |G - m|) + 2 u w1 |G - m| + u |M'|  <=  (4 + K) u (|m| + w1 (A + |m|))          [``bound_m``]
        (|M'| <= |m| + w1 (A + |m|) and |G - m| <= A + |m|: the magnitudes the three operations round.)

  exp_avg_sq:  v beta2 rounds twice (beta2 as float, the product); w2 G G rounds three times (w2 as float, two products) and carries the error of
        G twice, 2 |G| e_G <= 2 K u A^2; the sum rounds once:
        e_V <= 3 u beta2 v + (4 + 2 K) u w2 A^2  <=  (4 + 2 K) u (beta2 v + w2 A^2)                         [``bound_v``]

  param:       r = sqrt(V') computed from the computed V': |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), plus its own rounding u r.
        r / c rounds up to three times (c as float, the division -- or a reciprocal and a product); + eps rounds twice (eps as float, the sum):
        e_D <= min(e_V / sqrt(V'), sqrt(e_V)) / c + 5 u D.
        The computed D is at least D_lo = max(D - e_D, eps (1 - 2 u)) (the first term of the sum is never negative), so the quotient
        M' / D errs by at most e_M / D_lo + |M'| e_D / (D D_lo) + u |M' / D|; the product with s rounds twice (s as float, the product),
        the subtraction once:
        e_P <= s (e_M / D_lo + |M'| e_D / (D D_lo)) + 4 u |s M' / D| + u |P'|                                [``bound_p``]
The constants are counts of roundings, not fits to any implementation."""
import numpy as np

U = 2.0 ** -24


def step64(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, variant=None):
    """(P', M', V') of one step in float64; ``step`` is the count AFTER the increment (1 for the first step).  ``variant`` names a deliberately
    wrong restatement (tests/test_adam_cpu.py: the bounds must reject each of them)."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    if variant == "betas_swapped":
        b1, b2 = b2, b1
    if variant == "step_off_by_one":
        step = step - 1
    G = g + wd * p if (wd != 0 and variant != "adamw") else g
    M = m + (G - m) * (1.0 - b1)
    V = v * b2 + (1.0 - b2) * G * G
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    if variant == "no_bias_correction":
        bc1 = bc2 = 1.0
    if variant == "eps_in_sqrt_raw":                    # sqrt(v + eps) / sqrt(bc2)
        D = np.sqrt(V + eps) / np.sqrt(bc2)
    elif variant == "eps_in_sqrt_corrected":            # sqrt(v / bc2 + eps)
        D = np.sqrt(V / bc2 + eps)
    else:
        D = np.sqrt(V) / np.sqrt(bc2) + eps
    p0 = p * (1.0 - lr * wd) if variant == "adamw" else p
    return p0 - (lr / bc1) * M / D, M, V


VARIANTS = ("no_bias_correction", "betas_swapped", "step_off_by_one", "adamw", "eps_in_sqrt_raw", "eps_in_sqrt_corrected")


def bounds(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """(bound_p, bound_m, bound_v): see the module docstring for the derivation of each"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    w1, w2 = 1.0 - b1, 1.0 - b2
    K = 3.0 if wd != 0 else 0.0
    P1, M1, V1 = step64(p, g, m, v, step, lr, betas, eps, wd)
    A = np.abs(g) + wd * np.abs(p)
    e_m = (4 + K) * U * (np.abs(m) + w1 * (A + np.abs(m)))
    e_v = (4 + 2 * K) * U * (b2 * v + w2 * A * A)
    c, s = np.sqrt(1.0 - b2 ** step), lr / (1.0 - b1 ** step)
    r = np.sqrt(V1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_r = np.where(r > 0, np.minimum(e_v / np.where(r > 0, r, 1.0), np.sqrt(e_v)), np.sqrt(e_v))
    D = r / c + eps
    e_d = e_r / c + 5 * U * D
    d_lo = np.maximum(D - e_d, eps * (1 - 2 * U))
    upd = s * M1 / D
    e_p = s * (e_m / d_lo + np.abs(M1) * e_d / (D * d_lo)) + 4 * U * np.abs(upd) + U * np.abs(P1)
    return e_p, e_m, e_v


def excess(got, before, step, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """worst |got - ref| / bound over the elements of (param, exp_avg, exp_avg_sq) after a step, as a triple; ``before`` = the fp32
    (param, grad, exp_avg, exp_avg_sq) the step read.  An element whose bound is 0 must be exact (counted as 0 if it is, inf if not);
    non-finite outputs count as inf."""
    p, g, m, v = before
    refs = step64(p, g, m, v, step, lr, betas, eps, wd)
    out = []
    for got_k, ref_k, bound_k in zip(got, refs, bounds(p, g, m, v, step, lr, betas, eps, wd)):
        err = np.abs(np.asarray(got_k, dtype=np.float64) - ref_k)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound_k > 0, err / np.where(bound_k > 0, bound_k, 1.0), np.where(err == 0, 0.0, np.inf))
        ratio = np.where(np.isfinite(err), ratio, np.inf)
        out.append(float(ratio.max()) if ratio.size else 0.0)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
SMALL = 128          # elements [0, SMALL): gradients at the 10^-6 scale in every step, exactly 0 in the first (sqrt(v) stays near eps)
ZEROS = 256          # elements [0, ZEROS): exactly 0 in the first step


def make_problem(numel, steps, seed=0):
    """(param (numel,), grads (steps, numel)) in fp32: parameters of unit scale, gradient magnitudes log-uniform over 10^-6 ... 10^1 with
    random signs; a block of exact zeros in the first step, and inside it a block that stays at the 10^-6 scale afterwards.  Blocks that
    do not fit into ``numel`` are cut."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(numel).astype(np.float32)
    mag = 10.0 ** rng.uniform(-6.0, 1.0, size=(steps, numel))
    g = mag * rng.choice([-1.0, 1.0], size=(steps, numel))
    small = rng.uniform(1e-6, 9e-6, size=(steps, min(SMALL, numel))) * rng.choice([-1.0, 1.0], size=(steps, min(SMALL, numel)))
    g[:, :small.shape[1]] = small
    g[0, :min(ZEROS, numel)] = 0.0
    return p, g.astype(np.float32)


def scalars(step, lr, betas=(0.9, 0.999)):
    """(step_size, bc2_sqrt) as the C ABI takes them: formed in double for the step being taken"""
    return lr / (1.0 - betas[0] ** step), float(np.sqrt(1.0 - betas[1] ** step))
