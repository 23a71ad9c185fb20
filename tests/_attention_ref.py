"""float64 references of the self-attention kernels (csrc/attention.hip: k_attn_fwd in its bf16 and fp32-class forms, k_attn_bwd_D, k_attn_bwd_dq,
k_attn_bwd_dkv), per-element error bounds derived from them, the seeded input families and the case table, shared by
tests/test_attention_bounds_cpu.py (the bounds accept an emulation of the kernels' arithmetic and reject subtly wrong ones) and
tests/test_attention_fp64_gpu.py (the kernels meet them).  Pure torch; every function works on tensors of any device.

Every reference is computed in float64 from exactly the values a kernel reads: the stored bf16 or fp32 ``qkv``, and for the backward also the fp32
``out`` and ``lse2`` tensors that are passed to it.  All T x T matrices are dense float64, per (sample, head), in chunks of ``CHUNK`` heads.

Notation: u = 2^-24, s = ch^-1/2, C = ``C_BOUND`` = 8, gamma(K) = C sqrt(K) u (the random-walk accumulation term of ``_fp64_bounds.conv_gamma``).

Two things make these bounds differ from ``c u sum|terms|``:
  * the fp32-class products are bf16 PAIR products (``U_PAIR`` below), 2^-16 of the magnitudes and not u;
  * the softmax turns the ABSOLUTE error of a logit into the RELATIVE error of a weight, so every bound on an output carries the logit error
    ``delta`` (which scales with A_S = s |q| |k|^T, not with the logit itself) as a factor of the output's magnitude."""
import math

import torch

from _fp64_bounds import C_BOUND, U32, check_le, conv_gamma, round16, ulp16       # noqa: F401  (check_le, round16: for the test modules)

# A bf16 pair product (at_split8 / at_pack_bf16_rest / at_mfma3 in csrc/attention.hip).  An fp32 x is split as hi = bf16_rne(x), lo = bf16_rne(x - hi); the
# kernels accumulate hi hi + hi lo + lo hi, so against x y they miss  ex y + x ey  (e = x - hi - lo) and  lo lo.  Over a binade, |x - hi| is at most half a
# bf16 ulp, 2^-9 of the binade's TOP: x - hi is exact in fp32 and |lo| <= 2^-9 |x|, |e| <= 2^-18 |x|, lo lo <= 2^-18 |x y| for x in the upper part of its
# binade -- 3 * 2^-18 < 2^-16 per product, the value used here.  Just above a power of two the same half ulp is 2^-8 |x|, so the strict worst case of a
# single product is twice that per factor, 2^-17 + 2^-17 + 2^-16 = 2^-15, reached only when both factors and both of their remainders sit there.  Over random
# operands the error of a product has an rms of 2^-17.8 and exceeds 2^-16 for 0.4 % of them (tests/test_attention_bounds_cpu.py measures both), with either
# sign: U_PAIR times the sum of the magnitudes is more than three rms of even a single product, and further out for every sum of several.
U_PAIR = 2.0 ** -16
U_BF16 = 2.0 ** -9                                    # one round-to-nearest to bf16
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
CHUNK = 64                                            # (sample, head) problems per float64 pass

FAMILIES = ("random", "peaked", "dominant", "offset", "zero_v_tail")


# ------------------------------------------------------------------------------------------------ dispatch rules and the case table
def chp_of(ch: int) -> int:
    """the padded head width the kernels are instantiated for (at_launch, ssdnerf_attention_qkv_f32_backward)"""
    return 32 if ch <= 32 else 64 if ch <= 64 else 96 if ch <= 96 else 128


def fwd_kg(B: int, T: int, heads: int) -> int:
    """key groups of the forward: two when the grid of ceil(T / 128) x B heads blocks is at most 512 and T >= 128"""
    return 2 if ((T + 127) // 128) * B * heads <= 512 and T >= 128 else 1


def bwd_kg(B: int, T: int, heads: int, ch: int) -> int:
    """key / query groups of the backward: the forward's rule, heads of at most 64 channels only"""
    return fwd_kg(B, T, heads) if ch <= 64 else 1


# (B, T, heads, ch), CHP, KG of the forward, KG of the backward -- as the rules above select them (tests/test_attention_bounds_cpu.py asserts both that
# the literals agree with the rules and that every pair the rules can select occurs).  The smallest shapes that reach every instantiation: one key
# block and several, ragged last blocks of 1 and 31 keys, widths below and at the padded width, odd block counts (unequal key groups).
CASES = (
    ((1, 1, 1, 8), 32, 1, 1),
    ((2, 33, 2, 24), 32, 1, 1),
    ((1, 129, 1, 32), 32, 2, 2),
    ((1, 31, 2, 40), 64, 1, 1),
    ((1, 32, 1, 64), 64, 1, 1),
    ((2, 65, 2, 64), 64, 1, 1),
    ((1, 160, 2, 48), 64, 2, 2),
    ((1, 257, 1, 64), 64, 2, 2),
    ((1, 64, 1, 72), 96, 1, 1),
    ((1, 127, 2, 80), 96, 1, 1),
    ((1, 128, 1, 96), 96, 2, 1),
    ((1, 257, 1, 80), 96, 2, 1),
    ((1, 96, 1, 104), 128, 1, 1),
    ((1, 192, 2, 128), 128, 2, 1),
    ((1, 257, 1, 128), 128, 2, 1),                   # nine key blocks: the two groups walk five and four
    ((33, 129, 8, 8), 32, 1, 1),                     # T >= 128 and one group, by the grid alone: 2 x 264 blocks
    ((65, 128, 8, 64), 64, 1, 1),                    # 1 x 520 blocks
)
SHAPES = tuple(c[0] for c in CASES)
FWD_PATHS = {(chp, kg) for chp in (32, 64, 96, 128) for kg in (1, 2)}
BWD_PATHS = {(chp, kg) for chp in (32, 64) for kg in (1, 2)} | {(96, 1), (128, 1)}


# ------------------------------------------------------------------------------------------------ inputs
def make_inputs(family: str, shape, seed: int = 0):
    """(qkv (B, T, 3C) fp32, dout (B, T, C) fp32) of a family, from a seeded CPU generator; channel order [head][q | k | v][ch]"""
    B, T, heads, ch = shape
    g = torch.Generator().manual_seed(1000003 * FAMILIES.index(family) + 7919 * T + 131 * ch + 17 * heads + B + seed)
    x = torch.randn(B, T, heads, 3, ch, generator=g) * 1.3
    dout = torch.randn(B, T, heads, ch, generator=g)
    if family == "peaked":
        x[:, :, :, 0] *= 6.0
    elif family == "dominant":
        # channel 0 carries the logits: q0 = a everywhere, k0 = a at four random keys, 1.2 a at the LAST key and 0 elsewhere, a^2 s = 8 -- so every
        # row's maximum (logit 9.6 against 8 and ~0) arrives in the final, ragged key block, after the running maximum has already moved
        a = math.sqrt(8.0 * math.sqrt(ch))
        x[:, :, :, :2] = torch.randn(B, T, heads, 2, ch, generator=g) * 0.05
        x[:, :, :, 0, 0] = a
        x[:, :, :, 1, 0] = 0.0
        keys = torch.randint(0, T, (B, heads, 4), generator=g)
        for b in range(B):
            for h in range(heads):
                x[b, keys[b, h], h, 1, 0] = a
        x[:, T - 1, :, 1, 0] = 1.2 * a
    elif family == "offset":
        x[:, :, :, 1] += 3.0
        x[:, :, :, 2] += 50.0
    elif family == "zero_v_tail":
        x[:, T - 1, :, 2] = 0.0
        dout[:, T - 1] = 0.0
    elif family != "random":
        raise ValueError(family)
    return x.reshape(B, T, 3 * heads * ch).contiguous(), dout.reshape(B, T, heads * ch).contiguous()


def heads_of(qkv: torch.Tensor, heads: int):
    """(q, k, v), each (B heads, T, ch) float64, of a (B, T, 3C) tensor"""
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    q, k, v = qkv.double().view(B, T, heads, 3, ch).permute(3, 0, 2, 1, 4).reshape(3, B * heads, T, ch)
    return q, k, v


def per_head(x: torch.Tensor, heads: int) -> torch.Tensor:
    """(B, T, C) -> (B heads, T, ch) float64"""
    B, T, C = x.shape
    return x.double().view(B, T, heads, C // heads).permute(0, 2, 1, 3).reshape(B * heads, T, C // heads)


def merge_heads(x: torch.Tensor, B: int) -> torch.Tensor:
    """(B heads, T, ch) -> (B, T, C)"""
    N, T, ch = x.shape
    return x.view(B, N // B, T, ch).permute(0, 2, 1, 3).reshape(B, T, (N // B) * ch)


def merge_qkv(dq, dk, dv, B: int) -> torch.Tensor:
    """three (B heads, T, ch) -> (B, T, 3C) in the layout of qkv"""
    N, T, ch = dq.shape
    return torch.stack([dq, dk, dv], 0).view(3, B, N // B, T, ch).permute(1, 3, 2, 0, 4).reshape(B, T, 3 * (N // B) * ch)


def gamma(K: int) -> float:
    return conv_gamma(K)


# ------------------------------------------------------------------------------------------------ forward
def forward_ref(qkv: torch.Tensor, heads: int):
    """dict(out, out_bound: (B, T, C); lse2, lse2_bound: (B, heads, T)) of the forward on ``qkv`` (fp32: the fp32-class form, bf16: the bf16 form).

    S = s q k^T, P = softmax(S), ref = P v, A = P |v|, A_S = s |q| |k|^T.
    Logit error: delta_ij = prod * A_S,ij + C u (|S_ij| + max_j |S_ij|) with prod = U_PAIR + gamma(3 ch) for the pair products (three fp32
    accumulations per channel) and gamma(ch) for bf16 operands (exact products); the last term is the fp32 constant s log2 e, the fp32
    fma(S, c, -m) -- which rounds a value of magnitude up to |S| + |m| -- and the hardware exp2.  With Delta_i = max_j delta_ij every unnormalised
    weight of the row is off by a factor within e^(+-Delta_i), so is their sum, and every normalised weight by a factor within e^(+-2 Delta_i).
    fp32 form: |got - ref| <= (2 Delta + U_PAIR + gamma(3 T) + C u) A: the pair product P V, its 3 T accumulations (the per-block rescale by alpha
        and the group merge are fewer roundings than that), the division by the row sum.
    bf16 form: P is rounded once to bf16 for the numerator and the row sum takes the unrounded p, 2^-9 each; the output is rounded to bf16:
        |got - ref| <= (2 Delta + 2^-8 + gamma(T) + C u) A + ulp_bf16(ref) / 2.
    lse2 (log2 domain): |got - log2 sum_j e^S_ij| <= Delta / ln 2 + C u (|m| + |lse2|), m the row maximum in the log2 domain: the kernel adds m and
        log2 of the row sum in fp32."""
    f32 = qkv.dtype == torch.float32
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    s = ch ** -0.5
    prod = U_PAIR + gamma(3 * ch) if f32 else gamma(ch)
    tail = U_PAIR + gamma(3 * T) + C_BOUND * U32 if f32 else 2 * U_BF16 + gamma(T) + C_BOUND * U32
    qa, ka, va = heads_of(qkv, heads)
    outs, bounds, lses, lbounds = [], [], [], []
    for i in range(0, qa.shape[0], CHUNK):
        q, k, v = qa[i:i + CHUNK], ka[i:i + CHUNK], va[i:i + CHUNK]
        S = s * (q @ k.transpose(1, 2))
        A_S = s * (q.abs() @ k.abs().transpose(1, 2))
        delta = prod * A_S + C_BOUND * U32 * (S.abs() + S.abs().amax(-1, keepdim=True))
        Delta = delta.amax(-1)
        P = torch.softmax(S, -1)
        ref, A = P @ v, P @ v.abs()
        bound = (2 * Delta + tail)[..., None] * A
        if not f32:
            bound = bound + 0.5 * ulp16(ref, torch.bfloat16)
        lse2 = torch.logsumexp(S, -1) * LOG2E
        m2 = S.amax(-1) * LOG2E
        outs.append(ref); bounds.append(bound); lses.append(lse2)
        lbounds.append(Delta * LOG2E + C_BOUND * U32 * (m2.abs() + lse2.abs()))
    cat = lambda ts: torch.cat(ts, 0)
    return dict(out=merge_heads(cat(outs), B), out_bound=merge_heads(cat(bounds), B), lse2=cat(lses).view(B, heads, T),
                lse2_bound=cat(lbounds).view(B, heads, T))


# ------------------------------------------------------------------------------------------------ backward
def backward_ref(qkv: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, lse2: torch.Tensor, heads: int):
    """(ref, bound), each (B, T, 3C) float64 in the layout of qkv, of attention_qkv_f32_backward on exactly these fp32 tensors.

    P = exp2(S log2 e - lse2), dP = dO v^T, D_i = sum_c dO_ic out_ic, dS = P o (dP - D); dQ = s dS k, dK = s dS^T q, dV = P^T dO.
    E_P   = (U_PAIR + gamma(3 ch)) A_S + C u (|S| + |lse|)     relative error of P: the absolute error of its exponent (pair product S, fp32 fma, exp2)
    d_dP  = (U_PAIR + gamma(3 ch)) |dO| |v|^T                   pair product dP
    d_D   = gamma(ch) sum_c |dO_ic| |out_ic|                    fp32 fma chain over ch channels
    E_dS  = P o (E_P o |dP - D| + d_dP + d_D)                   absolute error of dS (its own two fp32 roundings are inside the pair term below)
    bound(dQ) = s (E_dS |k| + (U_PAIR + gamma(3 T)) |dS| |k|)   and the same with ^T and |q| for dK;   bound(dV) = (P o E_P)^T |dO| + (U_PAIR + gamma(3 T)) P^T |dO|."""
    B, T, C3 = qkv.shape
    ch = C3 // (3 * heads)
    s = ch ** -0.5
    pc, pt = U_PAIR + gamma(3 * ch), U_PAIR + gamma(3 * T)
    qa, ka, va = heads_of(qkv, heads)
    oa, ga, la = per_head(out, heads), per_head(dout, heads), lse2.double().reshape(B * heads, T)
    refs, bounds = [], []
    for i in range(0, qa.shape[0], CHUNK):
        q, k, v, o, g, l2 = qa[i:i + CHUNK], ka[i:i + CHUNK], va[i:i + CHUNK], oa[i:i + CHUNK], ga[i:i + CHUNK], la[i:i + CHUNK, :, None]
        S = s * (q @ k.transpose(1, 2))
        A_S = s * (q.abs() @ k.abs().transpose(1, 2))
        P = torch.exp2(S * LOG2E - l2)
        dP = g @ v.transpose(1, 2)
        D = (g * o).sum(-1, keepdim=True)
        dS = P * (dP - D)
        E_P = pc * A_S + C_BOUND * U32 * (S.abs() + (l2 * LN2).abs())
        d_dP = pc * (g.abs() @ v.abs().transpose(1, 2))
        d_D = gamma(ch) * (g.abs() * o.abs()).sum(-1, keepdim=True)
        E_dS = P * (E_P * (dP - D).abs() + d_dP + d_D)
        dq, dk, dv = s * (dS @ k), s * (dS.transpose(1, 2) @ q), P.transpose(1, 2) @ g
        bq = s * (E_dS @ k.abs() + pt * (dS.abs() @ k.abs()))
        bk = s * (E_dS.transpose(1, 2) @ q.abs() + pt * (dS.abs().transpose(1, 2) @ q.abs()))
        bv = (P * E_P).transpose(1, 2) @ g.abs() + pt * (P.transpose(1, 2) @ g.abs())
        refs.append(torch.stack([dq, dk, dv])); bounds.append(torch.stack([bq, bk, bv]))
    r, b = torch.cat(refs, 1), torch.cat(bounds, 1)
    return merge_qkv(r[0], r[1], r[2], B), merge_qkv(b[0], b[1], b[2], B)


def grad_parts(dqkv: torch.Tensor, heads: int):
    """dict(dq, dk, dv) views (B, T, heads, ch) of a (B, T, 3C) tensor"""
    B, T, C3 = dqkv.shape
    v = dqkv.view(B, T, heads, 3, C3 // (3 * heads))
    return dict(dq=v[:, :, :, 0], dk=v[:, :, :, 1], dv=v[:, :, :, 2])


def backward_failures(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor, heads: int):
    """{dq, dk, dv: (elements outside the bound, worst error / bound)}"""
    g, r, b = grad_parts(got, heads), grad_parts(ref, heads), grad_parts(bound, heads)
    return {k: check_le(g[k], r[k], b[k]) for k in g}
