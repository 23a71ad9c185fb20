"""LPIPS v0.1 with the VGG16 trunk, restated from its definition in torch ops of any dtype (float64 is the reference of every LPIPS test), the
emulations of other convolution arithmetic that set and validate the end-to-end tolerance, and the float64 reference and error bound of the tap kernel
(csrc/lpips.hip, k_lpips_layer).  Shared by tests/test_lpips_cpu.py and tests/test_lpips_gpu.py; nothing here needs a GPU or the package under test.

The definition, for image pairs p, t in [0, 1], channels RGB:
  1. x = ((2 img - 1) - shift) / scale, shift = (-.030, -.088, -.188), scale = (.458, .448, .450)
  2. VGG16 ``features``: thirteen 3 x 3 convolutions, pad 1, with bias, each followed by ReLU; 3 -> 64, 64, pool, 128, 128, pool, 256, 256, 256, pool,
     512, 512, 512, pool, 512, 512, 512 (2 x 2 / stride 2 max-pool, floor mode); taps: the ReLU outputs of convolutions 2, 4, 7, 10, 13
  3. per tap and pixel fh = f / (sqrt(sum_c f_c^2) + 1e-10), d = sum_c w_c (fh_p - fh_t)^2 with the tap's lin weight w; spatial mean of d; the score is
     the sum over the five taps."""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24
FEATURE_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_AFTER = (1, 3, 6, 9)                    # positions in FEATURE_IDX of the convolutions a pool follows
TAPS = (1, 3, 6, 9, 12)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


# ------------------------------------------------------------------------------------------------ other convolution arithmetic, emulated in float64
def round_bits(x, bits):
    """float64 -> nearest value with ``bits`` significand bits, ties to even"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits) / 2.0 ** bits, e)


def trunc_bits(x, bits):
    """float64 -> the value with ``bits`` significand bits next towards zero"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.trunc(m * 2.0 ** bits) / 2.0 ** bits, e)


def conv_as(x, w, b, mode):
    """3 x 3 / pad 1 convolution + bias of float64 tensors with the products of another arithmetic, accumulated in float64:
    ``tf32``    inputs and weights rounded to 11 significand bits: what PyTorch lets cuDNN do with fp32 convolutions unless told otherwise, and the
                reference does not tell it -- the accuracy of the reference's own LPIPS numbers
    ``bf16x2``  this library's fp32-class form: activations TRUNCATED to 8 + 8 bits, weights as the rounded pair hi + lo, the lo * lo product dropped
    ``bf16``    plain bf16 operands (what the tolerance must reject)"""
    if mode == "exact":
        return F.conv2d(x, w, b, 1, 1)
    if mode == "tf32":
        return F.conv2d(round_bits(x, 11), round_bits(w, 11), b, 1, 1)
    if mode == "bf16":
        return F.conv2d(round_bits(x, 8), round_bits(w, 8), b, 1, 1)
    if mode == "bf16x2":
        xh = trunc_bits(x, 8)
        xl = trunc_bits(x - xh, 8)
        wh = round_bits(w, 8)
        wl = round_bits(w - wh, 8)
        return F.conv2d(xh, wh, b, 1, 1) + F.conv2d(xl, wh, None, 1, 1) + F.conv2d(xh, wl, None, 1, 1)
    raise ValueError(mode)


# ------------------------------------------------------------------------------------------------ the restatement
def params_of(sd, dtype=torch.float64):
    """([(weight, bias)] * 13, [lin (C,)] * 5) from a state dict keyed ``features.<idx>.weight | bias`` and ``lin<k>.model.1.weight``"""
    convs = [(sd[f"features.{i}.weight"].to(dtype), sd[f"features.{i}.bias"].to(dtype)) for i in FEATURE_IDX]
    lins = [sd[f"lin{k}.model.1.weight"].to(dtype).reshape(-1) for k in range(5)]
    return convs, lins


def tap_distance(fp, ft, w):
    """step 3 for NCHW feature tensors of equal shape and a (C,) weight -> (N,) spatial means"""
    hp = fp / (fp.square().sum(1, keepdim=True).sqrt() + 1e-10)
    ht = ft / (ft.square().sum(1, keepdim=True).sqrt() + 1e-10)
    return ((hp - ht).square() * w[None, :, None, None]).sum(1).mean((1, 2))


def lpips_ref(pred, target, sd, dtype=torch.float64, mode="exact"):
    """LPIPS of the pairs of two (n, h, w, 3) image tensors in ``dtype`` arithmetic -> (n,) tensor of ``dtype``"""
    convs, lins = params_of(sd, dtype)
    shift = torch.tensor(SHIFT, dtype=dtype)[None, :, None, None]
    scale = torch.tensor(SCALE, dtype=dtype)[None, :, None, None]
    n = pred.shape[0]
    x = torch.cat([pred, target]).to("cpu", dtype).permute(0, 3, 1, 2)
    x = ((2 * x - 1) - shift) / scale
    out = torch.zeros(n, dtype=dtype)
    for i, (w, b) in enumerate(convs):
        x = F.relu(conv_as(x, w, b, mode))
        if i in TAPS:
            out = out + tap_distance(x[:n], x[n:], lins[TAPS.index(i)])
        if i in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    return out


# ------------------------------------------------------------------------------------------------ test images
def _quant(x):
    return torch.round(x.clamp(0, 1) * 255) / 255


def make_pairs(h, w, seed=5):
    """five (pred, target) pairs of k/255 images, (5, h, w, 3) fp32 each: unrelated noise; smooth +- 3/255; unrelated smooth; shifted by 2 px; blended
    towards white -- from far apart to nearly equal, which is the range of scores a reconstruction's test views cover"""
    g = torch.Generator().manual_seed(seed)

    def smooth():
        return F.interpolate(torch.rand(1, 3, max(h // 8, 2), max(w // 8, 2), generator=g), size=(h, w), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)

    A, B = [], []
    A.append(_quant(torch.rand(h, w, 3, generator=g)))
    B.append(_quant(torch.rand(h, w, 3, generator=g)))
    s = smooth()
    A.append(_quant(s))
    B.append(_quant(s + torch.randint(-3, 4, (h, w, 3), generator=g) / 255))
    A.append(_quant(smooth()))
    B.append(_quant(smooth()))
    s = smooth()
    A.append(_quant(s))
    B.append(_quant(torch.roll(s, 2, 1)))
    s = smooth()
    A.append(_quant(s))
    B.append(_quant(s * 0.8 + 0.2))
    return torch.stack(A).float(), torch.stack(B).float()


def rel_err(got, ref):
    return ((got.double().cpu() - ref.double().cpu()).abs() / ref.double().cpu().abs())


# ------------------------------------------------------------------------------------------------ the tap kernel: reference and bound
LAYER_K, LAYER_K2 = 4, 4


def lpips_layer_ref(x_raw, w, n):
    """(value (n,), E (n,)) in float64 from the raw convolution output x_raw (2n, C, H, W) the kernel read and its (C,) lin weight:
    value = mean_pixels sum_c w_c (fh_p - fh_t)^2 of f = relu(x_raw); E = mean_pixels sum_c |w_c| (|fh_p| + |fh_t|)^2, the magnitude the bound scales"""
    f = F.relu(x_raw.double())
    w = w.double()[None, :, None, None]
    hp = f[:n] / (f[:n].square().sum(1, keepdim=True).sqrt() + 1e-10)
    ht = f[n:] / (f[n:].square().sum(1, keepdim=True).sqrt() + 1e-10)
    value = ((hp - ht).square() * w).sum(1).mean((1, 2))
    E = ((hp.abs() + ht.abs()).square() * w.abs()).sum(1).mean((1, 2))
    return value, E


def lpips_layer_bound(E, C, acc_in=None, value=None):
    """|got - (acc_in + value)| <= LAYER_K u (sqrt(C) + LAYER_K2) E  (+ u |acc_in + value| when something is accumulated into),  u = 2^-24.

    Derivation, first order in u, for an fp32 evaluation whose channel sums are trees of depth at most 2 sqrt(C) - 2 (pairwise sums, or a few serial terms
    per lane followed by a butterfly: depth 8 + log2(C / 8) <= 2 sqrt(C) - 2 from C = 64 on; a fully serial sum over C is NOT covered), every term of such
    a sum non-negative:
      norm      s = sum_c f_c^2: one rounding per product and one per level, relative error <= (depth + 1) u <= (2 sqrt(C) - 1) u; the square root halves
                it and adds u / 2:                                                                      |dn| / n <= sqrt(C) u
      fh        f / (n + eps) or f * (1 / (n + eps)): the addition, the reciprocal or division, the product: 3 u more (2 u when divided)
                                                                                                          |dfh| <= (sqrt(C) + 3) u |fh|
      e         = fh_p - fh_t, one rounding:                 |de| <= (sqrt(C) + 3) u (|fh_p| + |fh_t|) + u |e| <= (sqrt(C) + 4) u (|fh_p| + |fh_t|)
      e^2       |d(e^2)| <= 2 |e| |de| + u e^2 <= (2 sqrt(C) + 9) u (|fh_p| + |fh_t|)^2           (|e| <= |fh_p| + |fh_t|)
      w e^2     one more rounding:                                                                       (2 sqrt(C) + 10) u |w| (|fh_p| + |fh_t|)^2
      sum_c     a tree of the same depth over terms of one sign (or, for signed w, bounded by their magnitudes): + (2 sqrt(C) - 1) u sum_c |w| e^2
    so per pixel |dd| <= (4 sqrt(C) + 9) u sum_c |w_c| (|fh_p| + |fh_t|)^2.  The pixel sum and the division by H W are fp64 (nothing at this scale);
    the conversion of the mean to fp32 adds u |value| <= u E.  Together (4 sqrt(C) + 10) u E <= 4 u (sqrt(C) + 4) E: LAYER_K = 4, LAYER_K2 = 4.
    Accumulating into a non-zero acc rounds the sum once more: u |acc_in + value|, which does not scale with E and is added as its own term."""
    bound = LAYER_K * U32 * (math.sqrt(C) + LAYER_K2) * E
    if acc_in is not None:
        bound = bound + U32 * (acc_in.double() + value).abs()
    return bound


def check_lpips_layer(got, x_raw, w, n, acc_in=None):
    """``got`` (n,) = what a tap evaluation returned for x_raw / w (plus ``acc_in`` when it accumulates) -> (pairs outside the bound, NaN included;
    worst |got - ref| / bound)"""
    value, E = lpips_layer_ref(x_raw.cpu(), w.cpu(), n)
    ref = value if acc_in is None else acc_in.double().cpu() + value
    bound = lpips_layer_bound(E, x_raw.shape[1], None if acc_in is None else acc_in.cpu(), value)
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= bound)
    ratio = err / bound.clamp(min=1e-300)
    return int(bad.sum()), float(ratio.max())


def make_tap_input(n, C, H, W, seed=0, zero_share=0.05):
    """a raw convolution output (2n, C, H, W) fp32 like a VGG layer's (about half the values negative), with pixels whose values are ALL non-positive --
    all-zero features after the ReLU -- in the prediction, in the target, and in both at once"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2 * n, C, H, W, generator=g) * torch.rand(2 * n, 1, H, W, generator=g) * 3
    dead = torch.rand(2 * n, 1, H, W, generator=g) < zero_share
    dead[n:] |= dead[:n] & (torch.rand(n, 1, H, W, generator=g) < 0.5)          # some pixels dead in both images of a pair
    x = torch.where(dead, -x.abs(), x)
    x[0, :, 0, 0] = 0.0                                                           # and one exactly zero before the ReLU
    return x
