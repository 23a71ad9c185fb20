"""float64 references of the UNet kernels (csrc/conv_igemm.hip, csrc/groupnorm.hip) and per-element error bounds derived from them, shared by
tests/test_fp64_bounds_cpu.py (the bounds reject subtly wrong emulations) and tests/test_unet_kernels_fp64_gpu.py (the kernels meet them).

Every reference is computed in float64 from the exact values the kernel read: 16-bit and fp32 tensors upcast, an f32x2 weight as ``w_hi + w_lo``.
A bound is ``c * u * (sum of the magnitudes that an fp32 computation of the same expression rounds)``, u = 2^-24, with the constant ``C_BOUND`` and
the derivation written next to each checker.  Nothing here needs a GPU: the functions work on tensors of any device."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32
C_BOUND = 8               # the c of every bound below (see each checker for why 8 is enough)
C_GN = 4                  # GroupNorm forward: four roundings per element (fp32 rstd * gamma, (pb - mean) * a + beta, * (1 + scale) + shift, x * a + o)


# ------------------------------------------------------------------------------------------------ 16-bit rounding in float64
_FMT = {torch.bfloat16: (8, -125), torch.float16: (11, -13)}              # significand bits, smallest normal exponent (frexp convention)


def ulp16(v: torch.Tensor, dtype) -> torch.Tensor:
    """spacing of the 16-bit format at float64 values ``v`` (subnormal spacing below the normal range)"""
    bits, emin = _FMT[dtype]
    _, e = torch.frexp(v)
    # 2^(e - bits) written as its bit pattern: exact on every device (ldexp / pow may round in the last place)
    return ((torch.clamp(e, min=emin).to(torch.int64) - bits + 1023) << 52).view(torch.float64)


def round16(v: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    """float64 -> nearest value of the 16-bit format, ties to even, still as float64 (one rounding: v / ulp is exact)"""
    q = ulp16(v, dtype)
    return torch.round(v / q) * q                                          # torch.round rounds half to even


# ------------------------------------------------------------------------------------------------ convolution
def conv_ref(x, w, bias=None, res=None, stride=1, upsample=False, x2=None):
    """(ref, A): the float64 convolution (zero padding k // 2, nearest 2x upsampling of the input when ``upsample``, input [x | x2] when ``x2``)
    plus bias and residual, and A = conv(|x|, |w|) + |bias| + |res|, the sum of the magnitudes an fp32 accumulation rounds"""
    xin = x.double() if x2 is None else torch.cat([x.double(), x2.double()], 1)
    if upsample:
        xin = F.interpolate(xin, scale_factor=2, mode="nearest")
    w = w.double()
    pad = w.shape[-1] // 2
    ref = F.conv2d(xin, w, None, stride, pad)
    A = F.conv2d(xin.abs(), w.abs(), None, stride, pad)
    if bias is not None:
        ref = ref + bias.double()[None, :, None, None]
        A = A + bias.double().abs()[None, :, None, None]
    if res is not None:
        ref = ref + res.double()
        A = A + res.double().abs()
    return ref, A


def conv_gamma(K: int, c: float = C_BOUND) -> float:
    """fp32 accumulation of K exact products (bf16 x bf16 is exact in fp32): each partial sum is rounded once, and the rounding errors of a
    long sum behave like a random walk, so the accumulated error stays within c * sqrt(K) * u * A (a worst-case K * u * A bound would hide a
    whole missing product at K = 1152).  One rounding for the bias and one for the residual fit inside the same allowance."""
    return c * math.sqrt(K) * U32


def check_conv_bf16(got, ref, A, K, c: float = C_BOUND):
    """bf16 output.  The result must be bf16_rne(ref), except that it may be the neighbouring bf16 value on the other side of a rounding
    boundary when ref lies within gamma * A of that boundary: precisely, got must be bf16_rne(x) for some x in [ref - gamma A, ref + gamma A]
    (bf16_rne is monotone, so that is the closed range between the roundings of the two ends).  Truncation instead of round-to-nearest-even,
    a second rounding of a partial result to bf16, or any error of about one ulp away from a boundary falls outside.
    Returns (number of elements outside the bound, number of elements that differ from bf16_rne(ref), worst excess in ulps)."""
    g = got.double()
    gam = conv_gamma(K, c)
    lo, hi = round16(ref - gam * A), round16(ref + gam * A)
    bad = (g < lo) | (g > hi)
    mism = int((g != round16(ref)).sum())
    over = torch.maximum(lo - g, g - hi).clamp(min=0) / ulp16(ref, torch.bfloat16)
    return int(bad.sum()), mism, float(over.max()) if over.numel() else 0.0


def f32x2_bound(A, K, c: float = C_BOUND):
    """fp32 output of the bf16 x 2 form.  The activation is split by truncation, x = x_hi + x_lo + d with |d| < 2^-15 |x| (8 + 8 significand
    bits, include/ssdnerf_hip.h, ssdnerf_conv2d_nhwc_f32x2_plan); the weights are exact as passed (the reference uses w_hi + w_lo); lo * lo is
    dropped, |x_lo w_lo| <= 2^-7 |x| 2^-9 |w|.  Per product the error is then well inside 2^-15 |x w| and of either sign, so
    |got - ref| <= 2^-15 A + gamma A, gamma the fp32 accumulation term of ``conv_gamma``."""
    return (2.0 ** -15 + conv_gamma(K, c)) * A


def check_le(got, ref, bound):
    """(number of elements with |got - ref| > bound, worst |got - ref| / bound)"""
    err = (got.double() - ref).abs()
    ratio = err / bound.clamp(min=1e-300)
    return int((err > bound).sum()), float(ratio.max()) if ratio.numel() else 0.0


# ------------------------------------------------------------------------------------------------ GroupNorm
def _silu(v):
    return v * torch.sigmoid(v)


def _dsilu(v):
    s = torch.sigmoid(v)
    return s * (1 + v * (1 - s))


def _group_stats(xc, G):
    """fp64 mean and variance (1 / n) per (sample, group) of an NCHW float64 tensor, as (B, C, 1, 1) per channel"""
    B, C = xc.shape[:2]
    v = xc.reshape(B, G, -1)
    mean = v.mean(-1)
    var = (v - mean[..., None]).square().mean(-1)
    rep = lambda t: t.repeat_interleave(C // G, 1)[:, :, None, None]
    return rep(mean), rep(var)


def gn_ref(x, G, gamma, beta, ss=None, eps=1e-5, act=False, pre_bias=None, x2=None, out_dtype=torch.float32, c: float = C_GN):
    """(ref, bound) of group_norm_nhwc: y = act(x a + o), a = rstd gamma (1 + scale), o = (beta - mean rstd gamma)(1 + scale) + shift.
    The kernel forms a and o per (sample, channel) in fp32 from fp64 statistics and applies one fma per element; each of its four roundings
    (rstd gamma, (pb - mean) a + beta, the scale-shift fma, x a + o) errs by at most u times the magnitude it rounds, so before the activation
    |got - ref| <= c u (|x a| + |mean a| + |beta (1 + scale)| + |shift|), c = 4 (``C_GN``; the statistics themselves are fp64-exact when they are
    right).  This grows LINEARLY with |mean| / std, as any fp32 apply must; a cancellation in E[x^2] - E[x]^2 formed in fp32 grows quadratically
    and exceeds it.  SiLU carries the error through its derivative (|silu'| <= 1.1) and adds its own c u |silu(v)| (fp32 exp2 / rcp).  16-bit
    outputs add half an ulp of ref."""
    xc = x.double() if x2 is None else torch.cat([x.double(), x2.double()], 1)
    C = xc.shape[1]
    if pre_bias is not None:
        xc = xc + pre_bias.double()[None, :, None, None]
    mean, var = _group_stats(xc, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    g64, b64 = gamma.double()[None, :, None, None], beta.double()[None, :, None, None]
    sc = torch.ones_like(g64) if ss is None else 1 + ss.double()[:, :C, None, None]
    sh = torch.zeros_like(g64) if ss is None else ss.double()[:, C:, None, None]
    a = rstd * g64 * sc
    v = (xc - mean) * a + b64 * sc + sh
    mag = (xc * a).abs() + (mean * a).abs() + (b64 * sc).abs() + sh.abs()
    if pre_bias is not None:                                               # the kernel rounds (pb - mean) a, not (x + pb) a
        mag = mag + (pre_bias.double()[None, :, None, None] * a).abs()
    bound = c * U32 * mag
    if act:
        ref = _silu(v)
        bound = 1.1 * bound + c * U32 * ref.abs()
    else:
        ref = v
    if out_dtype != torch.float32:
        bound = bound + 0.5 * ulp16(ref, out_dtype)
    return ref, bound


def gn_bwd_ref(x, dy, G, gamma, beta, ss=None, eps=1e-5, act=False, out_dtype=torch.float32, c: float = C_BOUND):
    """(ref, bound) of group_norm_nhwc_backward(_cat): dx = rstd (p - mean(p) - xhat mean(p xhat)), p = dy silu'(v) gamma (1 + scale), means over
    the group.  The kernel computes each of the three terms in fp32 from fp64 group sums, so |got - ref| <= c u rstd (P + mean(P) +
    (|x| + |mean|) rstd mean(P |xhat|)), P = |dy gamma (1 + scale)| (1 + |v|max) the magnitude of p together with what the rounding of v does to
    it through silu' (|silu''| < 1), |v|max = (|x| + |mean|) rstd |gamma (1 + scale)| + |beta (1 + scale)| + |shift|; xhat is formed from x and the
    mean, whose magnitudes are what its rounding scales with.  c = 8: p takes three products and the SiLU derivative (exp2 / rcp) before the three
    terms are combined.  16-bit outputs add half an ulp of ref."""
    xc = x.double()
    B, C = xc.shape[:2]
    mean, var = _group_stats(xc, G)
    rstd = 1.0 / torch.sqrt(var + eps)
    g64, b64 = gamma.double()[None, :, None, None], beta.double()[None, :, None, None]
    sc = torch.ones_like(g64) if ss is None else 1 + ss.double()[:, :C, None, None]
    sh = torch.zeros_like(g64) if ss is None else ss.double()[:, C:, None, None]
    xh = (xc - mean) * rstd
    v = (xh * g64 + b64) * sc + sh
    p = dy.double() * (_dsilu(v) if act else 1.0) * g64 * sc
    gm = lambda t: t.reshape(B, G, -1).mean(-1).repeat_interleave(C // G, 1)[:, :, None, None]
    mp, mpx = gm(p), gm(p * xh)
    ref = rstd * (p - mp - xh * mpx)
    # magnitudes: P bounds |p| and what the rounding of v (|x| rstd |gamma scale| + ...) does to it through silu' (|silu''| <= 0.5 < 1)
    vmag = (xc.abs() + mean.abs()) * rstd * (g64 * sc).abs() + (b64 * sc).abs() + sh.abs()
    P = (dy.double() * g64 * sc).abs() * (1 + vmag)
    bound = c * U32 * rstd * (P + gm(P) + (xc.abs() + mean.abs()) * rstd * gm(P * xh.abs()))
    if out_dtype != torch.float32:
        bound = bound + 0.5 * ulp16(ref, out_dtype)
    return ref, bound


def check_sums(got, y, G, c: float = C_BOUND):
    """the statistics a producer wrote, fp64 [B][G][2] (sum x, sum x^2), against the tensor it wrote.  What a consumer takes from them is the
    mean and the variance q / n - (s / n)^2, so those are checked: |mean - mean_ref| <= c u 16 (|mean| + std) and |var - var_ref| <=
    c u 16 var -- the accuracy of fp32 partial sums of at most 256 values around a local pivot (rounding errors add like a random walk,
    sqrt(256) = 16), carried on in fp64.  A sum of squares formed in fp32 at a large mean errs by ~ u mean^2 per partial sum, a
    quadratic term in |mean| / std that falls outside.  Returns (failures, worst ratio of error to bound)."""
    B = y.shape[0]
    v = y.double().reshape(B, G, -1)
    n = v.shape[-1]
    mean, var = v.mean(-1), v.var(-1, unbiased=False)
    s, q = got.double().reshape(B, G, 2).unbind(-1)
    mg = s / n
    vg = q / n - mg * mg
    k = c * U32 * 16
    r = torch.stack([(mg - mean).abs() / (k * (mean.abs() + var.sqrt())), (vg - var).abs() / (k * var)])
    return int((r > 1).sum()), float(r.max())
