"""The UNet's convolution and GroupNorm kernels (csrc/conv_igemm.hip, csrc/groupnorm.hip) held to per-element bounds from float64 references
(tests/_fp64_bounds.py): every convolution case of tests/test_unet_fast_gpu.py with bias and residual, split-K, concatenated inputs and the
pre-split form; the GroupNorm statistics of every producer against fp64 sums of what it wrote; GroupNorm and the fp32 conv -> statistics -> norm
chain at group |mean| / std up to 1000."""
import pytest
import torch

import _fp64_bounds as FB
from ssdnerf_amd import _cabi as C
from ssdnerf_amd import unet_fast as UF
from test_unet_fast_gpu import CONV_CASES, F32X2_CASES

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def _cl(t):
    return t.cuda().contiguous(memory_format=CL)


def _out_hw(H, W, k, stride, upsample):
    Hv, Wv = (2 * H, 2 * W) if upsample else (H, W)
    return (Hv + 2 * (k // 2) - k) // stride + 1, (Wv + 2 * (k // 2) - k) // stride + 1


def _conv_case(case, seed, fp32):
    B, H, W, Cin, Cout, k, stride, upsample, hint = case
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(Cout, generator=g)
    Ho, Wo = _out_hw(H, W, k, stride, upsample)
    res = torch.randn(B, Cout, Ho, Wo, generator=g)
    if fp32:
        return _cl(x), w.cuda(), bias.cuda(), _cl(res)
    return _cl(x.bfloat16()), _cl(w.bfloat16()), bias.cuda(), _cl(res.bfloat16())


def _assert_bf16(got, ref, A, K, what):
    bad, mism, over = FB.check_conv_bf16(got, ref, A, K)
    assert bad == 0, f"{what}: {bad} of {got.numel()} elements outside the bound (worst {over:.2f} ulp past it), {mism} differ from bf16_rne(ref)"
    return mism


def _assert_le(got, ref, bound, what):
    bad, worst = FB.check_le(got, ref, bound)
    assert bad == 0, f"{what}: {bad} of {got.numel()} elements outside the bound, worst error {worst:.2f} x the bound"
    return worst


# ------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,upsample,hint", CONV_CASES)
def test_bf16_conv_is_bf16_rne_of_the_fp64_result(B, H, W, Cin, Cout, k, stride, upsample, hint):
    case = (B, H, W, Cin, Cout, k, stride, upsample, hint)
    x, w, bias, res = _conv_case(case, B * 1000 + H * 10 + Cin + k, fp32=False)
    got = UF.conv2d_nhwc_bf16(x, w, bias, res, stride, upsample, tile_hint=hint)
    ref, A = FB.conv_ref(x, w, bias, res, stride, upsample)
    _assert_bf16(got, ref, A, Cin * k * k, case)
    got = UF.conv2d_nhwc_bf16(x, w, None, None, stride, upsample, tile_hint=hint)
    ref, A = FB.conv_ref(x, w, None, None, stride, upsample)
    _assert_bf16(got, ref, A, Cin * k * k, ("plain",) + case)


@pytest.mark.parametrize("B,H,W,Cin,Cout,k,stride,upsample,hint", F32X2_CASES)
def test_f32x2_conv_meets_the_split_bound(B, H, W, Cin, Cout, k, stride, upsample, hint):
    case = (B, H, W, Cin, Cout, k, stride, upsample, hint)
    x, w, bias, res = _conv_case(case, B * 100 + Cin + k + H, fp32=True)
    hi, lo = UF.split_bf16x2_adjacent(w)
    got = UF.conv2d_nhwc_f32x2(x, hi, lo, bias, res, stride, upsample, tile_hint=hint)
    ref, A = FB.conv_ref(x, hi.double() + lo.double(), bias, res, stride, upsample)
    _assert_le(got, ref, FB.f32x2_bound(A, Cin * k * k), case)


SPLIT_CASES = [(8, 8, 512, 512, 3, 0), (2, 16, 1024, 512, 3, 5), (4, 8, 256, 512, 1, 2), (1, 5, 128, 64, 3, 3), (2, 8, 320, 320, 3, 4), (2, 8, 80, 320, 1, 2)]


@pytest.mark.parametrize("B,H,Cin,Cout,k,splits", SPLIT_CASES)
def test_split_k_convolutions_meet_the_bounds(B, H, Cin, Cout, k, splits):
    case = (B, H, H, Cin, Cout, k, 1, False, 0)
    x, w, bias, res = _conv_case(case, Cin + Cout + k, fp32=False)
    ws = torch.zeros(B * H * H * Cout, dtype=torch.float32, device="cuda")
    got = UF.conv2d_nhwc_bf16(x, w, bias, res, splitk_ws=ws, splits_hint=splits)
    assert float(ws.abs().max()) == 0.0
    ref, A = FB.conv_ref(x, w, bias, res)
    _assert_bf16(got, ref, A, Cin * k * k, ("bf16",) + case)
    x, w, bias, res = _conv_case(case, Cin + Cout + k + 1, fp32=True)
    hi, lo = UF.split_bf16x2_adjacent(w)
    for scratch in (None, torch.zeros(B * H * H * Cout, dtype=torch.float32, device="cuda")):
        got = UF.conv2d_nhwc_f32x2(x, hi, lo, bias, res, splits_hint=splits, splitk_ws=scratch)
        ref, A = FB.conv_ref(x, hi.double() + lo.double(), bias, res)
        _assert_le(got, ref, FB.f32x2_bound(A, Cin * k * k), ("f32x2",) + case)


CAT_CASES = [(80, 80, 80, 3, 0), (320, 160, 320, 3, 0), (160, 80, 160, 1, 0), (72, 24, 40, 3, 0), (128, 64, 128, 3, 5), (128, 64, 128, 3, 6), (256, 128, 256, 1, 5)]


@pytest.mark.parametrize("C1,C2,Cout,k,hint", CAT_CASES)
def test_concatenated_input_convolutions_meet_the_bounds(C1, C2, Cout, k, hint):
    g = torch.Generator().manual_seed(C1 + C2 + Cout + hint)
    B, H, W = 2, 16, 24
    a, b = torch.randn(B, C1, H, W, generator=g), torch.randn(B, C2, H, W, generator=g)
    w = torch.randn(Cout, C1 + C2, k, k, generator=g) / ((C1 + C2) * k * k) ** 0.5
    bias, res = torch.randn(Cout, generator=g).cuda(), torch.randn(B, Cout, H, W, generator=g)
    K = (C1 + C2) * k * k
    ab, bb, wb, rb = _cl(a.bfloat16()), _cl(b.bfloat16()), _cl(w.bfloat16()), _cl(res.bfloat16())
    got = UF.conv2d_nhwc_bf16(ab, wb, bias, rb, x2=bb, tile_hint=hint)
    ref, A = FB.conv_ref(ab, wb, bias, rb, x2=bb)
    _assert_bf16(got, ref, A, K, ("bf16", C1, C2, Cout, k, hint))
    hi, lo = UF.split_bf16x2_adjacent(w.cuda())
    af, bf, rf = _cl(a), _cl(b), _cl(res)
    got = UF.conv2d_nhwc_f32x2(af, hi, lo, bias, rf, x2=bf, tile_hint=hint)
    ref, A = FB.conv_ref(af, hi.double() + lo.double(), bias, rf, x2=bf)
    _assert_le(got, ref, FB.f32x2_bound(A, K), ("f32x2", C1, C2, Cout, k, hint))


@pytest.mark.parametrize("B,cin,cout,hw,k", [(8, 128, 128, 128, 3), (2, 128, 256, 64, 3), (8, 512, 512, 16, 3), (1, 64, 64, 20, 3), (5, 32, 64, 10, 1)])
def test_presplit_convolution_meets_the_split_bound(B, cin, cout, hw, k):
    """the pre-split form (two-group row kernel or the DMA-ring kernel's PS form) on what GroupNorm wrote pre-split; the reference convolves the
    same norm written as plain fp32"""
    g = torch.Generator().manual_seed(cin + cout + hw + k)
    x = _cl(torch.randn(B, cin, hw, hw, generator=g))
    w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).cuda()
    bias, res = torch.randn(cout, generator=g).cuda(), _cl(torch.randn(B, cout, hw, hw, generator=g))
    gamma, beta = (torch.rand(cin, generator=g) + 0.5).cuda(), torch.randn(cin, generator=g).cuda()
    hi, lo = UF.split_bf16x2_adjacent(w)
    assert UF.presplit_supported(x, cout, k) in (1, 2)
    ws = torch.zeros(B * 32 * 2, dtype=torch.float64, device="cuda")
    plain = UF.group_norm_nhwc(x, 32, gamma, beta, None, 1e-5, True, ws, workspace_is_zero=True)
    ws.zero_()
    split = UF.group_norm_nhwc(x, 32, gamma, beta, None, 1e-5, True, ws, workspace_is_zero=True, split_out=True)
    got = UF.conv2d_nhwc_f32x2_presplit(split, hi, lo, bias, res, splitk_ws=UF.shared_splitk_ws(x.device))
    ref, A = FB.conv_ref(plain, hi.double() + lo.double(), bias, res)
    _assert_le(got, ref, FB.f32x2_bound(A, cin * k * k), (B, cin, cout, hw, k))


def test_the_sweep_covers_every_tile_form_and_both_split_plans():
    """what the sweep above asks of the planner: every tile form (1 / 2 / 3 / 4 = 128 x 128, 128 x 64 / 64 x 128, 64 x 64, 256 x 128; 5 / 6 = the
    two-group kernel, generic and row-reuse), split and unsplit plans of both kernels, and the two-group kernel with more tiles than blocks"""
    lib = C.lib()
    bf_forms, bf_splits, f_splits = set(), set(), set()
    for B, H, W, Cin, Cout, k, stride, upsample, hint in CONV_CASES:
        Ho, Wo = _out_hw(H, W, k, stride, upsample)
        plan = lib.ssdnerf_conv2d_nhwc_bf16_plan(C.u32(B * Ho * Wo), C.u32(Cin), C.u32(Cout), C.u32(k), int(hint), 1, 0)
        bf_forms.add(hint if hint else plan & 0xff)
        bf_splits.add((plan >> 8) > 1)
    for B, H, Cin, Cout, k, splits in SPLIT_CASES:
        plan = lib.ssdnerf_conv2d_nhwc_bf16_plan(C.u32(B * H * H), C.u32(Cin), C.u32(Cout), C.u32(k), 0, 1, int(splits))
        bf_splits.add((plan >> 8) > 1)
    for B, H, W, Cin, Cout, k, stride, upsample, hint in F32X2_CASES:
        Ho, Wo = _out_hw(H, W, k, stride, upsample)
        if hint in (0, 1, 3):
            f_splits.add((lib.ssdnerf_conv2d_nhwc_f32x2_plan(C.u32(B * Ho * Wo), C.u32(Cin), C.u32(Cout), C.u32(k), int(hint), 0) >> 8) > 1)
    assert {1, 2, 3, 4, 5, 6} <= bf_forms, bf_forms
    assert bf_splits == {True, False} and f_splits == {True, False}, (bf_splits, f_splits)
    # the two-group kernel (256 x 128 tiles, at most one persistent block per CU) with several tiles per block
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    many = [c for c in CONV_CASES + F32X2_CASES if c[8] in (5, 6) and (c[0] * c[1] * c[2] // 256) * (c[4] // 128) > cus]
    assert many, "no two-group case with more tiles than CUs"


# ------------------------------------------------------------------------------------------------ statistics producers
def _check_producer(y, sums, G, what, fp32, r=0.0):
    """the sums a producer wrote against the output it wrote, then the norm computed from them against the fp64 norm of that output"""
    if fp32 or r == 0:                                                       # (16-bit outputs: the norm's half ulp is the yardstick at an offset)
        bad, worst = FB.check_sums(sums, y, G)
        assert bad == 0, f"{what}: statistics off by {worst:.2f} x the bound"
    g = torch.Generator().manual_seed(G + y.shape[1])
    C = y.shape[1]
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    ss = (torch.randn(y.shape[0], 2 * C, generator=g) * 0.3).cuda()
    out = UF.group_norm_nhwc(y, G, gamma, beta, ss, 1e-5, True, sums.reshape(-1), stats_ready=True)
    ref, bound = FB.gn_ref(y, G, gamma, beta, ss, 1e-5, True, out_dtype=y.dtype)
    return _assert_le(out, ref, bound, what)


def _bias(Cout, r, g, G=32):
    """conv bias of about r (sign per group) with a spread of 0.1 inside a group: the output groups sit at |mean| / std ~ r"""
    sign = torch.where(torch.rand(G, generator=g) < 0.5, -1.0, 1.0).repeat_interleave(Cout // G)
    return (r * sign + 0.1 * torch.randn(Cout, generator=g)).cuda()


@pytest.mark.parametrize("r", [0, 100])
@pytest.mark.parametrize("hint,H,B", [(1, 16, 2), (6, 64, 2), (5, 128, 8)])
def test_conv_epilogue_statistics_bf16(hint, H, B, r):
    g = torch.Generator().manual_seed(hint + H)
    x = _cl(torch.randn(B, 64, H, H, generator=g).bfloat16())
    w = _cl((torch.randn(128, 64, 3, 3, generator=g) / 24).bfloat16())
    sums = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
    y = UF.conv2d_nhwc_bf16(x, w, _bias(128, r, g), None, gn_sums=sums, gn_groups=32, tile_hint=hint)
    _check_producer(y, sums, 32, ("bf16 epilogue", hint, H, B, r), False, r=r)


@pytest.mark.parametrize("r", [0, 10, 100, 1000])
@pytest.mark.parametrize("hint,H,B", [(1, 16, 2), (3, 16, 2), (6, 64, 2), (5, 128, 8)])
def test_conv_epilogue_statistics_fp32(hint, H, B, r):
    g = torch.Generator().manual_seed(hint + H + 1)
    x = _cl(torch.randn(B, 64, H, H, generator=g))
    w = (torch.randn(128, 64, 3, 3, generator=g) / 24).cuda()
    hi, lo = UF.split_bf16x2_adjacent(w)
    sums = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
    y = UF.conv2d_nhwc_f32x2(x, hi, lo, _bias(128, r, g), None, gn_sums=sums, gn_groups=32, tile_hint=hint, splits_hint=1)
    _check_producer(y, sums, 32, ("fp32 epilogue", hint, H, B, r), True, r=r)


@pytest.mark.parametrize("r", [0, 100, 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_split_k_finishing_pass_statistics(dtype, r):
    if dtype == torch.bfloat16 and r > 100:
        r = 100
    g = torch.Generator().manual_seed(int(r) + 3)
    B, H, Cin, Cout = 8, 8, 512, 512
    res = torch.randn(B, Cout, H, H, generator=g)
    sums = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
    ws = torch.zeros(B * H * H * Cout, dtype=torch.float32, device="cuda")
    x = torch.randn(B, Cin, H, H, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / 68
    if dtype == torch.bfloat16:
        y = UF.conv2d_nhwc_bf16(_cl(x.bfloat16()), _cl(w.bfloat16()), _bias(Cout, r, g), _cl(res.bfloat16()), gn_sums=sums, gn_groups=32, splitk_ws=ws, splits_hint=6)
    else:
        hi, lo = UF.split_bf16x2_adjacent(w.cuda())
        y = UF.conv2d_nhwc_f32x2(_cl(x), hi, lo, _bias(Cout, r, g), _cl(res), gn_sums=sums, gn_groups=32, splits_hint=6, splitk_ws=ws)
    assert float(ws.abs().max()) == 0.0
    _check_producer(y, sums, 32, ("split-K finish", dtype, r), dtype == torch.float32, r=r)


@pytest.mark.parametrize("r", [0, 100, 1000])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_bias_residual_statistics(dtype, r):
    if dtype == torch.bfloat16 and r > 100:
        r = 100
    g = torch.Generator().manual_seed(int(r) + 5)
    B, C, H = 2, 256, 32
    x = _cl(torch.randn(B, C, H, H, generator=g).to(dtype))
    res = _cl(torch.randn(B, C, H, H, generator=g).to(dtype))
    bias = _bias(C, r, g)
    want = (x.double() + bias.double()[None, :, None, None] + res.double())
    sums = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
    y = UF.bias_residual_nhwc(x.clone(memory_format=CL), bias, res, gn_sums=sums, gn_groups=32)
    # one fp32 sum of three terms, then (16-bit) one rounding
    bound = 2 * FB.U32 * (x.double().abs() + bias.double().abs()[None, :, None, None] + res.double().abs())
    if dtype != torch.float32:
        bound = bound + 0.5 * FB.ulp16(want, dtype)
    _assert_le(y, want, bound, ("bias_residual", dtype, r))
    _check_producer(y, sums, 32, ("bias_residual", dtype, r), dtype == torch.float32, r=r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_run_level_statistics_from_the_epilogue_feed_the_norm(dtype):
    """runs of 4 channels from the convolution epilogue (gn_groups = Cout / 4), read by the norm's RUNS path with groups that straddle [y | y2]"""
    g = torch.Generator().manual_seed(17)
    B, H, Cin, C1, C2, G = 2, 16, 64, 128, 256, 32
    outs, runs = [], []
    for Cout in (C1, C2):
        x = torch.randn(B, Cin, H, H, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / 24
        rr = torch.zeros(B, Cout // 4, 2, dtype=torch.float64, device="cuda")
        if dtype == torch.float32:
            hi, lo = UF.split_bf16x2_adjacent(w.cuda())
            y = UF.conv2d_nhwc_f32x2(_cl(x), hi, lo, _bias(Cout, 10, g), None, gn_sums=rr, gn_groups=Cout // 4, tile_hint=1, splits_hint=1)
        else:
            y = UF.conv2d_nhwc_bf16(_cl(x.bfloat16()), _cl(w.bfloat16()), _bias(Cout, 10, g), None, gn_sums=rr, gn_groups=Cout // 4, tile_hint=1)
        if dtype == torch.float32:
            assert FB.check_sums(rr, y, Cout // 4)[0] == 0
        outs.append(y)
        runs.append(rr)
    Cc = C1 + C2
    gamma, beta = (torch.rand(Cc, generator=g) + 0.5).cuda(), torch.randn(Cc, generator=g).cuda()
    ss = (torch.randn(B, 2 * Cc, generator=g) * 0.3).cuda()
    got = UF.group_norm_nhwc(outs[0], G, gamma, beta, ss, 1e-5, True, runs[0], x2=outs[1], runs=(runs[0], runs[1]))
    ref, bound = FB.gn_ref(outs[0], G, gamma, beta, ss, 1e-5, True, x2=outs[1], out_dtype=dtype)
    _assert_le(got, ref, bound, ("runs", dtype))


# ------------------------------------------------------------------------------------------------ GroupNorm at large group means
def _offset_input(B, C, HW, r, g, G=32):
    off = (r * torch.where(torch.rand(G, generator=g) < 0.5, -1.0, 1.0)).repeat_interleave(C // G)
    return torch.randn(B, C, HW, HW, generator=g) + off[None, :, None, None]


@pytest.mark.parametrize("r", [0, 10, 100, 1000])
@pytest.mark.parametrize("B,C,HW", [(8, 128, 8), (2, 256, 64), (1, 128, 128)])
def test_group_norm_forward_at_large_group_means(B, C, HW, r):
    """fp32 input: the norm must stay fp32-class at any |mean| / std (its statistics are fp64); 16-bit input at |mean| / std <= 100"""
    g = torch.Generator().manual_seed(B * C + HW + int(r))
    x = _offset_input(B, C, HW, r, g)
    gamma, beta = (torch.rand(C, generator=g) + 0.5).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    ss = (torch.randn(B, 2 * C, generator=g) * 0.3).cuda()
    pb = (torch.randn(C, generator=g) * 0.5).cuda()
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        if dtype != torch.float32 and r > 100:
            continue
        xd = _cl(x.to(dtype))
        for s, act, pre in ((ss, True, None), (None, False, None), (ss, True, pb)):
            ws = torch.zeros(B * 32 * 2, dtype=torch.float64, device="cuda")
            got = UF.group_norm_nhwc(xd, 32, gamma, beta, s, 1e-5, act, ws, pre_bias=pre, workspace_is_zero=True)
            ref, bound = FB.gn_ref(xd, 32, gamma, beta, s, 1e-5, act, pre_bias=pre, out_dtype=dtype)
            _assert_le(got, ref, bound, ("group_norm", B, C, HW, r, dtype, act, pre is not None))


@pytest.mark.parametrize("r", [0, 10, 100, 1000])
@pytest.mark.parametrize("B,HW,hint", [(8, 8, 0), (2, 64, 1), (8, 128, 6)])
def test_fp32_conv_statistics_norm_chain_at_large_group_means(B, HW, hint, r):
    """f32x2 convolution with a bias of about r per group -> its epilogue's (or finishing pass's) statistics -> GroupNorm: what every fp32-class
    res block runs.  The norm of the convolution's output must meet the fp32 bound."""
    g = torch.Generator().manual_seed(B + HW + hint + int(r))
    Cin, Cout = 128, 128
    x = _cl(torch.randn(B, Cin, HW, HW, generator=g))
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).cuda()
    hi, lo = UF.split_bf16x2_adjacent(w)
    sums = torch.zeros(B, 32, 2, dtype=torch.float64, device="cuda")
    y = UF.conv2d_nhwc_f32x2(x, hi, lo, _bias(Cout, r, g), None, gn_sums=sums, gn_groups=32, tile_hint=hint,
                             splitk_ws=UF.shared_splitk_ws(x.device))
    _check_producer(y, sums, 32, ("fp32 chain", B, HW, hint, r), True, r=r)


# ------------------------------------------------------------------------------------------------ GroupNorm backward
@pytest.mark.parametrize("dtype,C,G,HW,r", [(dt, *c) for dt in (torch.float32, torch.bfloat16) for c in ((128, 32, 32, 0), (256, 32, 16, 10), (80, 16, 12, 0))]
                         + [(torch.float32, 128, 32, 64, 100)])
def test_group_norm_backward_meets_the_fp64_bound(dtype, C, G, HW, r):
    g = torch.Generator().manual_seed(C + HW + int(r))
    B = 2
    x = _cl(_offset_input(B, C, HW, r, g, G).to(dtype))
    dy = _cl(torch.randn(B, C, HW, HW, generator=g).to(dtype))
    gamma, beta = torch.randn(C, generator=g).cuda(), (torch.randn(C, generator=g) * 0.3).cuda()
    ss = (torch.randn(B, 2 * C, generator=g) * 0.5).cuda()
    sums = torch.zeros(B * G * 2, dtype=torch.float64, device="cuda")
    UF.group_norm_nhwc(x, G, gamma, beta, ss, 1e-5, True, sums, workspace_is_zero=True)
    got = UF.group_norm_nhwc_backward(x, dy, G, gamma, beta, ss, 1e-5, True, sums)
    ref, bound = FB.gn_bwd_ref(x, dy, G, gamma, beta, ss, 1e-5, True, out_dtype=dtype)
    _assert_le(got, ref, bound, ("gn backward", dtype, C, G, HW, r))
    if C % 2 == 0 and (C // 2) % (C // G) == 0:                               # the two-source form over [x[:, :C/2] | x[:, C/2:]]
        c1 = C // 2
        x1, x2 = _cl(x[:, :c1]), _cl(x[:, c1:])
        got1, got2 = UF.group_norm_nhwc_backward_cat(x1, x2, dy, G, gamma, beta, ss, 1e-5, True, sums)
        _assert_le(torch.cat([got1, got2], 1), ref, bound, ("gn backward cat", dtype, C, G, HW, r))
