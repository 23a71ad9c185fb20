"""The per-element bounds of tests/_fp64_bounds.py without a GPU: CPU emulations of correct kernels (fp32 arithmetic, one round-to-nearest-even
to bf16, tie cases included) must meet them, and emulations of subtly wrong kernels must not -- at a bench-like layer and at a ragged one.
Each mutation is an error the old norm-relative or max-abs tolerances of tests/test_unet_fast_gpu.py let through."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _fp64_bounds as FB

# bench-like: a level-1 layer of the cars UNet, K = 1152, whole 128 x 128 tiles; ragged: 35 pixels, 136 = 64 + 64 + 8 input channels, 40 outputs
SHAPES = {"bench": (1, 32, 32, 128, 128), "ragged": (1, 5, 7, 136, 40), "ragged80": (2, 5, 7, 80, 40)}


def _conv_inputs(shape, seed):
    B, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g).bfloat16()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).bfloat16()
    bias = torch.randn(Cout, generator=g)
    res = torch.randn(B, Cout, H, W, generator=g).bfloat16()
    return x, w, bias, res


def _acc32(x, w, cin=None):
    """the fp32 accumulation of a correct kernel (bf16 products are exact in fp32); ``cin``: only the first cin input channels"""
    if cin is not None:
        x, w = x[:, :cin], w[:, :cin]
    return F.conv2d(x.float(), w.float(), None, 1, 1)


def _epilogue(acc, bias, res):
    return (acc + bias[None, :, None, None] + res.float()).bfloat16()


def _trunc_bf16(t32):
    return (t32.contiguous().view(torch.int32) & -65536).view(torch.float32).bfloat16()


def _bad(got, x, w, bias, res):
    ref, A = FB.conv_ref(x, w, bias, res)
    bad, mism, over = FB.check_conv_bf16(got, ref, A, x.shape[1] * 9)
    return bad, mism


@pytest.mark.parametrize("shape", ["bench", "ragged"])
def test_bf16_conv_bound_accepts_a_correct_kernel(shape):
    x, w, bias, res = _conv_inputs(SHAPES[shape], 1)
    got = _epilogue(_acc32(x, w), bias, res)
    bad, mism = _bad(got, x, w, bias, res)
    assert bad == 0
    assert mism < 0.01 * got.numel()                                        # fp32 accumulation flips only values right at a rounding boundary


def test_bf16_conv_bound_accepts_exact_ties_rounded_to_even():
    """integer operands: every sum is exact in fp32, and the odd ones above 256 lie exactly between two bf16 values"""
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-16, 17, (2, 64, 6, 6), generator=g).bfloat16()
    w = torch.randint(-8, 9, (32, 64, 3, 3), generator=g).bfloat16()
    acc = _acc32(x, w)
    got = acc.bfloat16()
    ref, A = FB.conv_ref(x, w)
    assert torch.equal(ref, acc.double())
    ties = (FB.round16(ref) - ref).abs() == FB.ulp16(ref, torch.bfloat16) / 2
    assert int(ties.sum()) > 100
    assert torch.equal(got.double(), FB.round16(ref))                       # torch's bf16 conversion is the even rounding the checker states
    assert FB.check_conv_bf16(got, ref, A, 64 * 9)[0] == 0


@pytest.mark.parametrize("shape", ["bench", "ragged"])
def test_bf16_conv_bound_rejects_truncation_on_one_tile(shape):
    x, w, bias, res = _conv_inputs(SHAPES[shape], 2)
    f = (_acc32(x, w) + bias[None, :, None, None] + res.float()).permute(0, 2, 3, 1).reshape(-1, w.shape[0])      # [M][Cout] as the kernel tiles it
    got = f.bfloat16()
    got[:128, :128] = _trunc_bf16(f[:128, :128])
    got = got.reshape(x.shape[0], x.shape[2], x.shape[3], -1).permute(0, 3, 1, 2)
    assert _bad(got, x, w, bias, res)[0] > 0


@pytest.mark.parametrize("shape", ["bench", "ragged"])
def test_bf16_conv_bound_rejects_a_double_rounding(shape):
    x, w, bias, res = _conv_inputs(SHAPES[shape], 3)
    got = (((_acc32(x, w) + bias[None, :, None, None]).bfloat16().float() + res.float()).bfloat16())
    assert _bad(got, x, w, bias, res)[0] > 0


@pytest.mark.parametrize("shape", ["bench", "ragged"])
def test_bf16_conv_bound_rejects_one_missing_tap_at_one_border_pixel(shape):
    x, w, bias, res = _conv_inputs(SHAPES[shape], 4)
    acc = _acc32(x, w)
    # output pixel (0, 0) of sample 0 without the tap (kh, kw) = (2, 2), which reads input pixel (1, 1)
    acc[0, :, 0, 0] -= (x[0, :, 1, 1].float()[None, :] * w[:, :, 2, 2].float()).sum(1)
    got = _epilogue(acc, bias, res)
    assert _bad(got, x, w, bias, res)[0] > 0


@pytest.mark.parametrize("shape", ["ragged", "ragged80"])
def test_bf16_conv_bound_rejects_a_dropped_partial_k_tile(shape):
    x, w, bias, res = _conv_inputs(SHAPES[shape], 5)
    cin = x.shape[1]
    got = _epilogue(_acc32(x, w, cin=cin // 64 * 64), bias, res)            # 136 -> 128, 80 -> 64: the last, partial K-tile of every tap is lost
    assert _bad(got, x, w, bias, res)[0] > 0


def test_bf16_conv_bound_rejects_a_dropped_partial_k_tile_at_a_bench_like_width():
    x, w, bias, res = _conv_inputs((1, 32, 32, 136, 128), 6)
    got = _epilogue(_acc32(x, w, cin=128), bias, res)
    assert _bad(got, x, w, bias, res)[0] > 0


# ------------------------------------------------------------------------------------------------ f32x2
def _split_trunc(x):
    """the kernels' on-the-fly activation split: hi = truncation to bf16, lo = truncation of the exact remainder"""
    hi = (x.view(torch.int32) & -65536).view(torch.float32)
    lo = ((x - hi).view(torch.int32) & -65536).view(torch.float32)
    return hi, lo


def _f32x2_emulation(x, w_hi, w_lo, bias, res, drop_hi_lo=False):
    xh, xl = _split_trunc(x)
    conv = lambda a, b: F.conv2d(a.double(), b.double(), None, 1, 1)
    acc = conv(xh, w_hi) + conv(xl, w_hi) + (0 if drop_hi_lo else conv(xh, w_lo))
    return (acc.float() + bias[None, :, None, None] + res)


@pytest.mark.parametrize("shape", ["bench", "ragged"])
def test_f32x2_bound_accepts_the_three_product_form_and_rejects_a_dropped_hi_lo(shape):
    B, H, W, Cin, Cout = SHAPES[shape]
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    bias, res = torch.randn(Cout, generator=g), torch.randn(B, Cout, H, W, generator=g)
    from ssdnerf_amd.unet_fast import split_bf16x2
    w_hi, w_lo = split_bf16x2(w)
    ref, A = FB.conv_ref(x, w_hi.double() + w_lo.double(), bias, res)
    bound = FB.f32x2_bound(A, Cin * 9)
    assert FB.check_le(_f32x2_emulation(x, w_hi, w_lo, bias, res), ref, bound)[0] == 0
    assert FB.check_le(F.conv2d(x, w_hi.float() + w_lo.float(), bias, 1, 1) + res, ref, bound)[0] == 0      # plain fp32
    assert FB.check_le(_f32x2_emulation(x, w_hi, w_lo, bias, res, drop_hi_lo=True), ref, bound)[0] > 0
    # one wrong element with an error of 1e-2 (what a norm-relative 3e-5 lets through at the bench shape)
    y = _f32x2_emulation(x, w_hi, w_lo, bias, res)
    y[0, 3, 2, 1] += 1e-2
    assert FB.check_le(y, ref, bound)[0] == 1


# ------------------------------------------------------------------------------------------------ GroupNorm
def _gn_emulation(x, G, gamma, beta, ss, eps, act, out_dtype, var_mode="exact", sums=None):
    """group_norm_nhwc as csrc/groupnorm.hip computes it: fp64 mean / variance from (sum, sum of squares), a and o per channel in fp32, one fma
    per element, fp32 SiLU, one rounding to the output type.  ``var_mode``: "n-1" (unbiased variance) or "eps-std" (eps added to the std) are the
    mutations; ``sums``: fp64 (B, G, 2) statistics to use instead of exact ones."""
    B, C = x.shape[:2]
    xd = x.double()
    n = xd[0].numel() // G
    if sums is None:
        v = xd.reshape(B, G, -1)
        sums = torch.stack([v.sum(-1), v.square().sum(-1)], -1)
    mean = sums[..., 0] / n
    var = (sums[..., 1] / n - mean * mean).clamp(min=0)
    if var_mode == "n-1":
        var = var * n / (n - 1)
    rstd = 1.0 / (var.sqrt() + eps) if var_mode == "eps-std" else 1.0 / torch.sqrt(var + eps)
    rep = lambda t: t.repeat_interleave(C // G, 1)
    r32, m32 = rep(rstd).float(), rep(mean).float()
    f32 = lambda t: t.double().float()                                      # an fma: exact product and sum in fp64, one rounding
    a = r32 * gamma[None]
    o = f32((-m32).double() * a.double() + beta[None].double())
    if ss is not None:
        sc, sh = 1.0 + ss[:, :C], ss[:, C:]
        a = a * sc
        o = f32(o.double() * sc.double() + sh.double())
    y = f32(x.float().double() * a[:, :, None, None].double() + o[:, :, None, None].double())
    if act:
        y = y * torch.sigmoid(y)
    return y.to(out_dtype)


def _kgn_stats_fp32_partials(x, G, rows_per_block=64):
    """k_gn_stats's accumulation order for fp32 input (4 channels per thread, 256 threads): per thread fp32 running sums over rows lane_row,
    lane_row + rif, ... of a block's slab, an fp32 fold over the rows in flight, then fp64 across channels of a group and across blocks"""
    B, C, H, W = x.shape
    HW = H * W
    rif = 256 // (C // 4)
    v = x.permute(0, 2, 3, 1).reshape(B, HW // rows_per_block, rows_per_block // rif, rif, C).numpy().astype(np.float32)
    s = np.zeros((B, HW // rows_per_block, rif, C), np.float32)
    q = np.zeros_like(s)
    for t in range(v.shape[2]):
        s += v[:, :, t]
        q += v[:, :, t] * v[:, :, t]
    s2, q2 = s[:, :, 0].copy(), q[:, :, 0].copy()
    for r in range(1, rif):
        s2 += s[:, :, r]
        q2 += q[:, :, r]
    ds = s2.astype(np.float64).sum(1).reshape(B, G, -1).sum(-1)
    dq = q2.astype(np.float64).sum(1).reshape(B, G, -1).sum(-1)
    return torch.from_numpy(np.stack([ds, dq], -1))


def _gn_inputs(B, C, H, W, r, seed, G=32):
    """groups with |mean| / std = r: per-channel offsets r (+- 5 %) on unit-variance data"""
    g = torch.Generator().manual_seed(seed)
    off = r * (1 + 0.05 * torch.randn(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    off = off.reshape(G, -1).mean(-1, keepdim=True).expand(G, C // G).reshape(C)     # one mean per group, so |mean| / std is r
    x = torch.randn(B, C, H, W, generator=g) + off[None, :, None, None]
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    ss = torch.randn(B, 2 * C, generator=g) * 0.3
    return x, gamma, beta, ss


@pytest.mark.parametrize("out_dtype,r", [(torch.float32, r) for r in (0, 10, 100, 1000)] + [(d, r) for d in (torch.bfloat16, torch.float16) for r in (0, 10, 100)])
def test_gn_bound_accepts_the_kernel_arithmetic(out_dtype, r):
    """(16-bit outputs are run at |mean| / std <= 100: their half ulp dominates)"""
    x, gamma, beta, ss = _gn_inputs(2, 128, 16, 16, r, 11)
    for act, s in ((True, ss), (False, None)):
        ref, bound = FB.gn_ref(x, 32, gamma, beta, s, 1e-5, act, out_dtype=out_dtype)
        got = _gn_emulation(x, 32, gamma, beta, s, 1e-5, act, out_dtype)
        bad, worst = FB.check_le(got, ref, bound)
        assert bad == 0, (act, worst)


@pytest.mark.parametrize("mode", ["n-1", "eps-std"])
@pytest.mark.parametrize("shape", [(8, 128, 16, 16), (1, 96, 5, 7)])
def test_gn_bound_rejects_the_wrong_variance(mode, shape):
    B, C, H, W = shape
    x, gamma, beta, ss = _gn_inputs(B, C, H, W, 0, 12)
    x = x * (0.05 if mode == "eps-std" else 1.0)                            # (eps against a variance of 2.5e-3)
    ref, bound = FB.gn_ref(x, 32, gamma, beta, ss, 1e-5, True)
    assert FB.check_le(_gn_emulation(x, 32, gamma, beta, ss, 1e-5, True, torch.float32), ref, bound)[0] == 0
    assert FB.check_le(_gn_emulation(x, 32, gamma, beta, ss, 1e-5, True, torch.float32, var_mode=mode), ref, bound)[0] > 0


@pytest.mark.parametrize("HW", [64, 128])
def test_gn_bound_rejects_statistics_from_fp32_partial_sums_at_a_large_mean(HW):
    """|mean| / std = 100, B = 1, 4 channels per group: k_gn_stats's fp32 partial sums lose the variance to cancellation in E[x^2] - E[x]^2"""
    x, gamma, beta, _ = _gn_inputs(1, 128, HW, HW, 100, 13)
    ref, bound = FB.gn_ref(x, 32, gamma, beta, None, 1e-5, False)
    assert FB.check_le(_gn_emulation(x, 32, gamma, beta, None, 1e-5, False, torch.float32), ref, bound)[0] == 0
    sums = _kgn_stats_fp32_partials(x, 32)
    assert FB.check_sums(sums, x, 32)[0] > 0
    assert FB.check_le(_gn_emulation(x, 32, gamma, beta, None, 1e-5, False, torch.float32, sums=sums), ref, bound)[0] > 0
    exact = torch.stack([x.double().reshape(1, 32, -1).sum(-1), x.double().reshape(1, 32, -1).square().sum(-1)], -1)
    assert FB.check_sums(exact, x, 32)[0] == 0


def _gn_bwd_emulation(x, dy, G, gamma, beta, ss, eps, rstd_scale=1.0):
    """the backward's arithmetic (csrc/gn_bwd_math.h): fp64 group statistics, p and the three terms of dx in fp32"""
    B, C = x.shape[:2]
    v = x.double().reshape(B, G, -1)
    mean, rstd = v.mean(-1), 1.0 / torch.sqrt(v.var(-1, unbiased=False) + eps) * rstd_scale
    rep = lambda t: t.repeat_interleave(C // G, 1)[:, :, None, None].float()
    m32, r32 = rep(mean), rep(rstd)
    sc, sh = 1 + ss[:, :C, None, None], ss[:, C:, None, None]
    xh = (x - m32) * r32
    u = (xh * gamma[None, :, None, None] + beta[None, :, None, None]) * sc + sh
    s = torch.sigmoid(u)
    p = dy * (s * (1 + u * (1 - s))) * gamma[None, :, None, None] * sc
    gm = lambda t: t.double().reshape(B, G, -1).mean(-1).repeat_interleave(C // G, 1)[:, :, None, None].float()
    return r32 * (p - gm(p) - xh * gm(p * xh))


def test_gn_backward_bound_accepts_the_kernel_arithmetic_and_rejects_the_n_minus_1_variance():
    x, gamma, beta, ss = _gn_inputs(2, 64, 8, 8, 0, 14)
    dy = torch.randn(x.shape, generator=torch.Generator().manual_seed(15))
    ref, bound = FB.gn_bwd_ref(x, dy, 32, gamma, beta, ss, 1e-5, True)
    assert FB.check_le(_gn_bwd_emulation(x, dy, 32, gamma, beta, ss, 1e-5), ref, bound)[0] == 0
    n = x[0].numel() // 32
    assert FB.check_le(_gn_bwd_emulation(x, dy, 32, gamma, beta, ss, 1e-5, math.sqrt((n - 1) / n)), ref, bound)[0] > 0
