"""Float64 restatement of the total-variation regulariser (csrc/tv_loss.hip; the reference's tv_loss, lib/models/losses/tv_loss.py, dims=[-2, -1])
and the per-element bounds the kernel is held to, in the manner of _fp64_bounds.py.  ``emulate_f32`` restates the kernel's own arithmetic in numpy.

Bounds, u = 2^-24 (one fp32 rounding), first order in u; the inputs are fp32, so the float64 differences below are exact.
  slice mean:  the kernel forms dy, dx by one fp32 subtraction each (relative error <= u), s = fma(dx, dx, dy * dy) (<= 2u + 2u = 4u), r = sqrt(s)
               (<= 2u + u = 3u), and r^p by powf (the argument's 3u grows to 3pu; powf's own error <= 2 ulp <= 4u): (3p + 4)u per term.  The terms
               are >= 0 and summed in fp64 (2^-53 per add, 2^-53 h w in all, < u for any slice the contract admits), the mean is rounded to fp32
               once (u):  |mean - ref| <= (3p + 5)u ref; MEAN_C adds 3 for the second-order terms.
  gradient:    a term A = m dy, m = p powf(r, p - 1) / r: r 3u, powf (3(p - 1) + 4)u, the product with p u, the division by r 3u + u, the product
               with dy u + u (dy's own error): (3p + 8)u |A|, the same for B.  The kernel adds ((au - A) + (bl - B)) in fp32: three roundings,
               each <= u times the sum of the magnitudes below it, <= 2u T in all for T = |au| + |A| + |bl| + |B|.  The scale g / (h w) is rounded
               to fp32 once (u) and multiplied in (u):  |grad - ref| <= (3p + 12)u T |g| / (h w); GRAD_C adds 4.
  A term with r == 0 is exactly 0 on both sides, so a flat neighbourhood has a bound of 0: the gradient there must be exactly 0."""
import numpy as np

U = 2.0 ** -24


def mean_c(p):
    return 3.0 * p + 8.0


def grad_c(p):
    return 3.0 * p + 16.0


def diffs(x):
    """zero-padded forward differences along the two trailing dimensions (the reference's diff + cat with zeros)"""
    dy, dx = np.zeros_like(x), np.zeros_like(x)
    dy[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
    dx[..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    return dy, dx


def slice_means_ref(x, p):
    """(...) float64 mean over each (h, w) slice of r^p"""
    dy, dx = diffs(np.asarray(x, np.float64))
    return (np.sqrt(dy * dy + dx * dx) ** p).mean(axis=(-2, -1))


def grad_terms(x, p):
    """(A, B) = p r^(p-1) (dy, dx) / r, 0 where r == 0"""
    dy, dx = diffs(np.asarray(x, np.float64))
    r = np.sqrt(dy * dy + dx * dx)
    safe = np.where(r > 0, r, 1.0)
    m = np.where(r > 0, p * safe ** (p - 1) / safe, 0.0)
    return m * dy, m * dx


def grad_ref(x, p, g):
    """(gradient, its bound's magnitude T |g| / (h w)) of g[k] * slice_mean[k] with respect to x, float64"""
    x = np.asarray(x, np.float64)
    A, B = grad_terms(x, p)
    au, bl = np.zeros_like(A), np.zeros_like(B)
    au[..., 1:, :] = A[..., :-1, :]
    bl[..., :, 1:] = B[..., :, :-1]
    scale = np.asarray(g, np.float64)[..., None, None] / (x.shape[-2] * x.shape[-1])
    return ((au - A) + (bl - B)) * scale, (np.abs(au) + np.abs(A) + np.abs(bl) + np.abs(B)) * np.abs(scale)


def mean_excess(got, x, p):
    """max of |got - ref| / (MEAN_C u ref): <= 1 passes (a zero reference must be met exactly)"""
    ref = slice_means_ref(x, p)
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = mean_c(p) * U * ref
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


def grad_excess(got, x, p, g):
    ref, mag = grad_ref(x, p, g)
    err = np.abs(np.asarray(got, np.float64) - ref)
    bound = grad_c(p) * U * mag
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic in numpy
def _f32(v):
    return np.asarray(v, np.float32)


def emulate_f32(x, p, g, wrap=False, drop_left=False, hw_minus_1=False, f32_sum=False):
    """(slice means, gradient) as the kernel computes them; the keyword arguments switch on deliberately wrong variants"""
    x = _f32(x)
    p32 = np.float32(p)
    if wrap:
        dy, dx = np.roll(x, -1, axis=-2) - x, np.roll(x, -1, axis=-1) - x
    else:
        dy, dx = np.zeros_like(x), np.zeros_like(x)
        dy[..., :-1, :] = x[..., 1:, :] - x[..., :-1, :]
        dx[..., :, :-1] = x[..., :, 1:] - x[..., :, :-1]
    s = _f32(dx.astype(np.float64) * dx + (dy * dy).astype(np.float64))          # fma(dx, dx, dy * dy)
    r = np.sqrt(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(r > 0, np.power(r, p32), np.float32(0))
        m = np.where(r > 0, _f32(p32 * np.power(r, p32 - np.float32(1))) / r, np.float32(0)).astype(np.float32)
    A, B = _f32(m * dy), _f32(m * dx)
    h, w = x.shape[-2:]
    n = h * w - 1 if hw_minus_1 else h * w
    flat = t.reshape(*t.shape[:-2], -1)
    sums = np.cumsum(flat, axis=-1, dtype=np.float32)[..., -1] if f32_sum else flat.astype(np.float64).sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        means = _f32(np.asarray(sums, np.float64) / n)
        scale = _f32(np.asarray(g, np.float64) / n)[..., None, None]
    au, bl = np.zeros_like(A), np.zeros_like(B)
    au[..., 1:, :] = A[..., :-1, :]
    if wrap:
        au[..., 0, :] = A[..., -1, :]
    if not drop_left:
        bl[..., :, 1:] = B[..., :, :-1]
    grad = _f32(_f32(_f32(au - A) + _f32(bl - B)) * scale)
    return means, grad
