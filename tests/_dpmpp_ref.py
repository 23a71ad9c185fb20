"""float64 references of the DPM-Solver++(2M) sampler (ssdnerf_amd/diffusion.py: SamplingPlan 'dpmpp_2m', csrc/sampler_step.hip: k_step_v, form 2 without noise): the
kernel's update with per-element error bounds, the plan's coefficients, and an analytic denoiser whose probability-flow ODE has a closed form.
Both test modules draw from here: tests/test_dpmpp_cpu.py (the bounds accept an fp32 emulation of the kernel and reject wrong ones; the plan; the
sampler's generic branch) and tests/test_dpmpp_gpu.py (the kernel meets the bounds; fused against generic).

As in tests/_composite_ref.py, every input (an fp32 tensor, a coefficient passed as a C float) is taken as the exact value the kernel read and
upcast, and a bound is a forward error analysis of the fp32 kernel with u = 2^-24, the derivation next to each term.  No constant is fitted to the
kernel.

Nothing here needs a GPU: numpy arrays and tensors of any device are accepted, the results are float64 tensors on the CPU."""
import numpy as np
import torch
import torch.nn as nn

from _composite_ref import U32, _f64, check_le, f32_exact  # noqa: F401  (check_le, f32_exact: used by the test modules through this one)


# ------------------------------------------------------------------------------------------------ the kernel
def dpmpp_step_ref(x_t, v, q, a, b, c, d, e, lo, hi):
    """The DPM-Solver++ step (k_step_v<2, HAS_PREV, false>) in float64, with bounds: p = clamp(a x_t - b v, lo, hi), x_next = c p + d x_t + e q (q: the x0 of the step before; ``None``
    stands for the NULL pointer of a first-order step and needs e == 0); the coefficients as the C floats the library receives.
      p:      two products and a subtraction (or a product and an fma), each rounding at most u times a magnitude it rounds:
              |fl(fl(a x) - fl(b v)) - (a x - b v)| <= u |a x| + u |b v| + u (1 + u) (|a x| + |b v|), so B_p = 2 u (1 + u) (|a x_t| + |b v|).
              The clamp is 1-Lipschitz and monotone, and lo / hi are exact: it carries B_p and needs no exclusion.
      x_next: the kernel combines the ROUNDED p' with |p' - p| <= B_p: that is |c| B_p before any further rounding.  Each of the three products
              rounds once (u times its magnitude) and passes through at most two additions, each of which rounds at most u times the sum of the
              magnitudes it adds -- in whatever order they are added, and fused multiply-adds only remove roundings.  First order:
              3 u (|c p| + |d x_t| + |e q|).  Second order: the magnitudes are those of p', not p (3 u |c| B_p), and (1 + u)^3 - 1 - 3 u < 4 u^2 per
              term; both are covered by the factor (1 + 4 u) on the whole.
              B = (|c| B_p + 3 u (|c p| + |d x_t| + |e q|)) (1 + 4 u).
    Returns (p, B_p, x_next, B_xnext) as float64."""
    x, vv = _f64(x_t), _f64(v)
    a, b, c, d, e, lo, hi = (f32_exact(s) for s in (a, b, c, d, e, lo, hi))
    if q is None:
        assert e == 0.0
        qq = torch.zeros_like(x)
    else:
        qq = _f64(q)
    Bp = 2 * U32 * (1 + U32) * ((a * x).abs() + (b * vv).abs())
    p = (a * x - b * vv).clamp(lo, hi)
    xn = c * p + d * x + e * qq
    Bxn = (abs(c) * Bp + 3 * U32 * ((c * p).abs() + (d * x).abs() + (e * qq).abs())) * (1 + 4 * U32)
    return p, Bp, xn, Bxn


def dpmpp_case(n, seed):
    """(x_t, v, q): unit normals, so that p = a x_t - b v leaves [-1, 1] at either end for about a sixth of the elements each"""
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(size=n).astype(np.float32) for _ in range(3))


def dpmpp_coefficients():
    """(name, a, b, c, d, e) of the project's own linear 1000-step schedule: step 0 (first order, e = 0), step 1, a middle step and the last step
    (c, d, e = 1, 0, 0) of the 20-step plan, and the penultimate step of the 1000-step plan (b ~ 0.015, the largest |c| + |e|)"""
    from ssdnerf_amd.diffusion import NoiseSchedule, SamplingPlan
    sched = NoiseSchedule(dict(type="linear"), 1000)
    p20, p1000 = SamplingPlan(sched, "dpmpp_2m", 20).steps, SamplingPlan(sched, "dpmpp_2m", 1000).steps
    pick = [("step0", p20[0]), ("step1", p20[1]), ("middle", p20[10]), ("last", p20[-1]), ("late", p1000[-2])]
    return [(n, s.a, s.b, s.c, s.d, s.e) for n, s in pick]


def dpmpp_sizes(cap):
    """one float4; two; a ragged block, a full block of 256 lanes and one float4 past it; one float4 past a full grid of ``cap`` blocks of 256 lanes
    (the grid-stride loop's second trip has a single lane at work)"""
    return (4, 8, 1020, 1024, 1028, 4 * (256 * cap + 1))


# ------------------------------------------------------------------------------------------------ the plan
def plan_coefficients_ref(alphas_bar, n, order=2):
    """[(t, c, d, e)] of the 'dpmpp_2m' plan with ``n`` steps from the float64 ``alphas_bar`` table alone: timesteps arange(T-1, -1, -T/n) truncated,
    lambda = log sqrt(abar) - log sqrt(1 - abar), h = lambda_prev - lambda_t, phi = -expm1(-h), d = b_prev / b_t, c = a_prev phi (1 + 1/(2r)),
    e = -a_prev phi / (2r) with r = h_before / h; first order (step 0, or every step with ``order`` 1): c = a_prev phi, e = 0; the last step
    (t_prev = -1, abar_prev = 1) is (1, 0, 0)."""
    ab = np.asarray(alphas_bar, np.float64)
    T = len(ab)
    ts = [int(t) for t in np.arange(T - 1, -1, -(T / n))]
    a, b = np.sqrt(ab), np.sqrt(1 - ab)
    out, h_before = [], None
    for i, t in enumerate(ts):
        if i == len(ts) - 1:
            out.append((t, 1.0, 0.0, 0.0))
            break
        tp = ts[i + 1]
        h = (np.log(a[tp]) - np.log(b[tp])) - (np.log(a[t]) - np.log(b[t]))
        phi = -np.expm1(-h)
        if order == 2 and h_before is not None:
            r = h_before / h
            out.append((t, a[tp] * phi * (1 + 0.5 / r), b[tp] / b[t], -a[tp] * phi * 0.5 / r))
        else:
            out.append((t, a[tp] * phi, b[tp] / b[t], 0.0))
        h_before = h
    return out


# ------------------------------------------------------------------------------------------------ the analytic prior
class GaussianDenoiser(nn.Module):
    """The optimal denoiser of the i.i.d. prior x0 ~ N(mu, s^2): E[x0 | x_t] = mu + k (x_t - a mu), k = a s^2 / (a^2 s^2 + b^2), returned in the V
    parameterisation, v = (a x_t - x0*) / b, from the float64 tables (computed in float64, returned in x_t's dtype).  Assigned to
    ``GaussianDiffusion.denoising``."""

    def __init__(self, schedule, mu, s):
        super().__init__()
        self.a = torch.from_numpy(np.asarray(schedule["sqrt_alphas_bar"], np.float64))
        self.b = torch.from_numpy(np.asarray(schedule["sqrt_one_minus_alphas_bar"], np.float64))
        self.mu, self.s = float(mu), float(s)

    def forward(self, x_t, t, concat_cond=None):
        t = torch.as_tensor(t).reshape(-1).cpu()
        a, b = (tab[t].reshape(-1, 1, 1, 1).to(x_t.device) for tab in (self.a, self.b))
        x = x_t.double()
        x0 = self.mu + a * self.s ** 2 / (a ** 2 * self.s ** 2 + b ** 2) * (x - a * self.mu)
        return ((a * x - x0) / b).to(x_t.dtype)


def gaussian_ode_solution(x_T, schedule, mu, s):
    """the exact solution at t -> 0 of the probability-flow ODE of that prior started from x_T at t = T - 1: mu + s (x_T - a_T mu) / sqrt(a_T^2 s^2 + b_T^2)
    (the marginal at t is N(a_t mu, a_t^2 s^2 + b_t^2), and the flow maps quantiles to quantiles)"""
    a, b = float(schedule["sqrt_alphas_bar"][-1]), float(schedule["sqrt_one_minus_alphas_bar"][-1])
    return mu + s * (_f64(x_T) - a * mu) / (a * a * s * s + b * b) ** 0.5
