"""References of the counter-based noise and of the stochastic sampling steps (ssdnerf_amd/csrc/philox.h, csrc/sampler_step.hip; ssdnerf_amd/diffusion.py:
SamplingPlan 'dpmpp_2m_sde'): Philox4x32-10 restated in numpy, the float64 Box-Muller of its words with a per-element bound of the fp32 device
arithmetic, the kernel's three update forms in float64 with per-element bounds, and the plan's coefficients from the alphas_bar table alone.
Both test modules draw from here: tests/test_sde_cpu.py (known answers, the gcc build of philox.h, statistics, the bounds accept an fp32 emulation and
reject wrong ones, the plan, the sampler's generic branch) and tests/test_sde_gpu.py (the kernels meet the bounds; fused against generic).

As in tests/_dpmpp_ref.py, every input (an fp32 tensor, a coefficient passed as a C float, the kernel's own z read back from the fill) is taken as the
exact value the kernel read, and a bound is a forward error analysis of the fp32 kernel with u = 2^-24, the derivation next to each term.  No constant
is fitted to the kernels; the three ulp errors of the device library's log, sqrt and sinpi / cospi are measured over every argument the generator can
feed them (profiles/sde.json, ``device_function_ulp``; tools/bench_sde.py --ulp).

Nothing here needs a GPU."""
import json
import os

import numpy as np
import torch

from _composite_ref import U32, _f64, check_le, f32_exact  # noqa: F401  (check_le: used by the test modules through this one)

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
Z_MAX = float(np.sqrt(-2 * np.log(2.0 ** -24)))                             # 5.768: the largest |z| (u = 2^-24, the smallest uniform)

KNOWN_ANSWERS = (  # Random123's kat_vectors for philox4x32-10: (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


# ------------------------------------------------------------------------------------------------ the integer stream
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """ten rounds on uint64 arrays that hold 32-bit values (a 32 x 32 product fits); returns the four output words as uint32 arrays"""
    c = [np.asarray(x, np.uint64) & MASK for x in np.broadcast_arrays(c0, c1, c2, c3)]
    k = [np.uint64(int(k0) & 0xFFFFFFFF), np.uint64(int(k1) & 0xFFFFFFFF)]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def quad_words(seed, draw, first, n):
    """uint32 [n, 4]: the words of quads first .. first + n - 1 of draw ``draw`` under the 64-bit ``seed`` (key = seed, low word first; counter =
    {quad index low, high, draw, 0})"""
    i4 = np.uint64(int(first)) + np.arange(n, dtype=np.uint64)
    seed = int(seed) & ((1 << 64) - 1)
    return np.stack(philox4x32_10(i4 & MASK, i4 >> np.uint64(32), np.uint64(draw), np.uint64(0), seed & 0xFFFFFFFF, seed >> 32), 1)


def uniforms(words):
    """u = ((r >> 9) + 0.5) 2^-23 as float64 (exact there and in fp32)"""
    return ((np.asarray(words, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def sincos2pi(u):
    """(sin 2 pi u, cos 2 pi u) in float64 with an exact reduction: 2 u = k / 2 + f, |f| <= 1/4, so that the results keep float64's RELATIVE accuracy
    next to their zeros (u is never on one: 4 u is an odd multiple of 2^-22 ... never an integer)"""
    x = 2.0 * np.asarray(u, np.float64)
    k = np.rint(2.0 * x)
    f = x - 0.5 * k                                                          # exact
    s, c = np.sin(np.pi * f), np.cos(np.pi * f)
    q = k.astype(np.int64) & 3
    return np.choose(q, [s, c, -s, -c]), np.choose(q, [c, -s, -c, s])


def normals(words):
    """float64 Box-Muller of uint32 [n, 4] words, flattened to the element order of the latent: (r0, r1) -> elements 4 i4, 4 i4 + 1 as R cos, R sin;
    (r2, r3) -> 4 i4 + 2, 4 i4 + 3"""
    u = uniforms(words)
    out = np.empty(u.shape, np.float64)
    for k in (0, 2):
        R = np.sqrt(-2.0 * np.log(u[:, k]))
        s, c = sincos2pi(u[:, k + 1])
        out[:, k], out[:, k + 1] = R * c, R * s
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ the fp32 normals' bound
def ulp32(v):
    """spacing of fp32 at the float64 values ``v`` (the subnormal spacing 2^-149 below the normal range)"""
    _, e = np.frexp(np.abs(np.asarray(v, np.float64)))
    return np.ldexp(1.0, np.maximum(e, -125) - 24)


def device_function_ulp():
    """the measured worst errors, in ulps of the exact result, of the device library's logf, sqrtf and sinpif / cospif over the 2^23 arguments the
    generator can feed them (profiles/sde.json; the ROCm installation ships no accuracy table of its device library)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "sde.json")
    with open(path) as f:
        c = json.load(f)["device_function_ulp"]
    return dict(log=float(c["log"]), sqrt=float(c["sqrt"]), trig=float(c["trig"]))


def normal_bounds(words, ulps):
    """(z, B): ``normals(words)`` and the bound of the device's fp32 evaluation, by first-order propagation.  u is exact.  With E_log, E_sqrt, E_trig
    the ulp errors of the three functions:
      L' = logf(u):        |L' - L| <= dL = E_log ulp(L)
      t  = -2 L':          exact (a power of two)
      R' = sqrtf(t):       sqrt(t) = R sqrt(1 + dL / |L|), within R dL / (2 |L|) of R to first order; the function adds E_sqrt ulp(sqrt t) <= E_sqrt 2 u sqrt(t):
                           B_R = R (dL / (2 |L|) + 2 u E_sqrt)
      c' = cospif(2 u1):   2 u1 is exact;  |c' - c| <= dC = E_trig ulp(c)           (sinpif alike)
      z' = fl(R' c'):      |z' - R c| <= |c| B_R + R dC + u |z|
    and the second-order terms (products of two of these, each below 2^-20 of the first-order ones) under a factor 1 + 2^-16 on the whole."""
    u = uniforms(words)
    z, B = np.empty(u.shape, np.float64), np.empty(u.shape, np.float64)
    for k in (0, 2):
        L = np.log(u[:, k])
        R = np.sqrt(-2.0 * L)
        BR = R * (ulps["log"] * ulp32(L) / (2 * np.abs(L)) + 2 * U32 * ulps["sqrt"])
        s, c = sincos2pi(u[:, k + 1])
        for j, f in ((k, c), (k + 1, s)):
            z[:, j] = R * f
            B[:, j] = (np.abs(f) * BR + R * ulps["trig"] * ulp32(f) + U32 * np.abs(R * f)) * (1 + 2.0 ** -16)
    return z.reshape(-1), B.reshape(-1)


# ------------------------------------------------------------------------------------------------ the step kernel
FORMS = {"ddim": 0, "langevin": 1, "ddpm": 2, "dpmpp_sde": 2}


def sde_step_ref(form, x_t, v, q, z, a, b, c, d, e, nz, lo, hi):
    """k_step_v (csrc/sampler_step.hip, the noise-injecting forms) in float64, with bounds; the coefficients as the C floats the library receives, z the fp32 normals the kernel adds (exact inputs here:
    their own error is ``normal_bounds``' business).  p = clamp(a x_t - b v, lo, hi), eps = (x_t - a p) / b,
        form 0:  c p + d eps + nz z         form 1:  x_t - d eps + nz z         form 2:  c p + d x_t + e q + nz z   (q None: the NULL pointer, e == 0)
      p:    as in _dpmpp_ref.dpmpp_step_ref: B_p = 2 u (1 + u) (|a x_t| + |b v|); the clamp carries it.
      eps:  as in _composite_ref.ddim_step_ref (the kernel multiplies fl(x_t - fl(a p')) by fl(1 / b)):
            B_eps = (|a| B_p + 2 u (|x_t| + |a p|)) / b + 2 u |eps|.
      sum:  the kernel combines the ROUNDED p' and eps': |c| B_p and |d| B_eps before any further rounding.  Then every product rounds once (u times
            its magnitude) and every addition rounds at most u times the sum of the magnitudes it adds, whatever the order, and fused multiply-adds only
            remove roundings.  A term that is a product and passes through k additions collects (k + 1) u of its magnitude; x_t in form 1 is no
            product and collects k u.  Forms 0 and 1 add three terms (two additions: 3 u each); form 2 adds four with e (three additions: 4 u) and
            three without.  The magnitudes are those of p' and eps', not p and eps, and (1 + u)^4 - 1 - 4 u < 7 u^2: both under the factor (1 + 8 u).
    Returns (p, B_p, x_next, B_xnext) as float64."""
    x, vv, zz = _f64(x_t), _f64(v), _f64(z)
    a, b, c, d, e, nz, lo, hi = (f32_exact(s) for s in (a, b, c, d, e, nz, lo, hi))
    Bp = 2 * U32 * (1 + U32) * ((a * x).abs() + (b * vv).abs())
    p = (a * x - b * vv).clamp(lo, hi)
    noise = nz * zz
    if form == 2:
        if q is None:
            assert e == 0.0
            qq = torch.zeros_like(x)
        else:
            qq = _f64(q)
        k = 4 if e != 0 else 3
        xn = c * p + d * x + e * qq + noise
        B = abs(c) * Bp + k * U32 * ((c * p).abs() + (d * x).abs() + (e * qq).abs() + noise.abs())
    else:
        eps = (x - a * p) / b
        Beps = (abs(a) * Bp + 2 * U32 * (x.abs() + (a * p).abs())) / abs(b) + 2 * U32 * eps.abs()
        if form == 0:
            xn = c * p + d * eps + noise
            B = abs(c) * Bp + abs(d) * Beps + 3 * U32 * ((c * p).abs() + (d * eps).abs() + noise.abs())
        elif form == 1:
            xn = x - d * eps + noise
            B = abs(d) * Beps + 3 * U32 * (x.abs() + (d * eps).abs() + noise.abs())
        else:
            raise ValueError(form)
    return p, Bp, xn, B * (1 + 8 * U32)


def sde_case(n, seed):
    """(x_t, v, q): unit normals, so that p = a x_t - b v leaves [-1, 1] at either end for about a sixth of the elements each"""
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=n).astype(np.float32) for _ in range(3))


def sde_coefficients():
    """(name, form, a, b, c, d, e, nz) from the project's own linear 1000-step schedule: DDIM with eta = 0.5 (first and a late step of 20), a Langevin
    correction, the ancestral sampler (a step of 20), and 'dpmpp_2m_sde': step 0 (first order), a middle step, and the penultimate step of the
    1000-step plan (b ~ 0.015, the largest |c| + |e|)"""
    from ssdnerf_amd.diffusion import NoiseSchedule, SamplingPlan
    sched = NoiseSchedule(dict(type="linear"), 1000)
    ddim = SamplingPlan(sched, "ddim", 20, eta=0.5, langevin_steps=1, langevin_delta=0.1).steps
    lang = [s for s in ddim if s.kind == "langevin"]
    ddim = [s for s in ddim if s.kind == "ddim"]
    ddpm = SamplingPlan(sched, "ddpm", 20).steps
    sde20, sde1000 = SamplingPlan(sched, "dpmpp_2m_sde", 20).steps, SamplingPlan(sched, "dpmpp_2m_sde", 1000).steps
    pick = [("ddim_first", ddim[0]), ("ddim_late", ddim[-2]), ("langevin", lang[len(lang) // 2]), ("ddpm", ddpm[10]), ("sde_step0", sde20[0]),
            ("sde_middle", sde20[10]), ("sde_late", sde1000[-2])]
    return [(n, FORMS[s.kind], s.a, s.b, s.c, s.d, s.e, s.n) for n, s in pick]


def sde_sizes(cap):
    """one float4; two; a ragged block, a full block of 256 lanes and one float4 and a bit past it; one float4 past a full grid of ``cap`` blocks of 256
    lanes (the grid-stride loop's second trip has a single lane at work)"""
    return (4, 8, 1020, 1024, 4100, 4 * (256 * cap + 1))


# ------------------------------------------------------------------------------------------------ the plan
def sde_plan_coefficients_ref(alphas_bar, n, order=2):
    """[(t, c, d, e, nz)] of the 'dpmpp_2m_sde' plan with ``n`` steps from the float64 ``alphas_bar`` table alone: timesteps arange(T-1, -1, -T/n)
    truncated, lambda = log sqrt(abar) - log sqrt(1 - abar), h = lambda_prev - lambda_t, base = a_prev (1 - e^-2h), d = (b_prev / b_t) e^-h,
    nz = b_prev sqrt(1 - e^-2h), c = base (1 + 1/(2r)), e = -base / (2r) with r = h_before / h; first order (step 0, or every step with ``order`` 1):
    c = base, e = 0; the last step (t_prev = -1) is (1, 0, 0, 0)."""
    ab = np.asarray(alphas_bar, np.float64)
    T = len(ab)
    ts = [int(t) for t in np.arange(T - 1, -1, -(T / n))]
    a, b = np.sqrt(ab), np.sqrt(1 - ab)
    out, h_before = [], None
    for i, t in enumerate(ts):
        if i == len(ts) - 1:
            out.append((t, 1.0, 0.0, 0.0, 0.0))
            break
        tp = ts[i + 1]
        h = (np.log(a[tp]) - np.log(b[tp])) - (np.log(a[t]) - np.log(b[t]))
        base = a[tp] * (1 - np.exp(-2 * h))
        d, nz = b[tp] / b[t] * np.exp(-h), b[tp] * np.sqrt(1 - np.exp(-2 * h))
        if order == 2 and h_before is not None:
            r = h_before / h
            out.append((t, base * (1 + 0.5 / r), d, -base * 0.5 / r, nz))
        else:
            out.append((t, base, d, 0.0, nz))
        h_before = h
    return out
