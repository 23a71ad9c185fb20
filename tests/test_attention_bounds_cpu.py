"""The per-element bounds of tests/_attention_ref.py without a GPU: a torch fp32 emulation of the attention kernels' arithmetic (bf16 pair products
hi hi + hi lo + lo hi accumulated in fp32, the online softmax over blocks of 32 keys, the merge of two key groups, the backward's exp2(S c - lse2))
must meet every bound on every input family, and emulations of subtly wrong kernels must not.  Each mutation is an error that the norm-relative
tolerances of tests/test_unet_fast_gpu.py let through; ``MUTATIONS`` names, for each, the family (one that tests/test_attention_fp64_gpu.py runs
on the same shape) that catches it.  The case table's (CHP, KG) columns are checked against the dispatch rules here as well."""
import math

import pytest
import torch

import _attention_ref as AR

CPU_SHAPES = ((1, 1, 1, 8), (2, 33, 2, 24), (1, 129, 1, 32), (1, 31, 2, 40), (2, 65, 2, 64), (1, 160, 2, 48), (1, 127, 2, 80), (1, 257, 1, 128))
MUT_SHAPE = (1, 129, 1, 32)            # five key blocks, the last one a single key; two key groups in both directions


def _bf(x):
    return x.bfloat16().float()


def _split(x):
    hi = _bf(x)
    return hi, _bf(x - hi)


def _pair(a, b, a_lo=True, b_lo=True):
    """a @ b as the kernels form it from fp32 operands: lo hi + hi lo + hi hi, each an fp32 accumulation.  ``a_lo=False`` / ``b_lo=False`` drop the
    term with that operand's lo half (the operand is then a single bf16)"""
    ah, al = _split(a)
    bh, bl = _split(b)
    acc = ah @ bh
    if b_lo:
        acc = ah @ bl + acc
    if a_lo:
        acc = al @ bh + acc
    return acc


def _fma(a, c, b):
    """fl32(a c + b): the product of two fp32 values is exact in float64"""
    return (a.double() * c + b.double()).float()


def _heads32(t, heads):
    return AR.per_head(t, heads).float()


def emu_forward(qkv, heads, kg, mut=None):
    """k_attn_fwd on (B, T, 3C) fp32 or bf16 ``qkv`` with ``kg`` key groups -> (out (B, T, C) in the input's type, lse2 (B, heads, T) fp32).
    Mutations: ``s_cross``: S without its hi lo term; ``p_lo``: P rounded to a single bf16 in P V (fp32 form); ``drop_key``: the last valid key is
    masked; ``pad_key``: one zero-padded key past T is admitted, with logit 0; ``merge_a1``: the second key group is merged without its rescale."""
    f32 = qkv.dtype == torch.float32
    B, T = qkv.shape[:2]
    q, k, v = (t.float() for t in AR.heads_of(qkv, heads))
    ch = q.shape[-1]
    c = float(torch.tensor(AR.LOG2E, dtype=torch.float32) / torch.sqrt(torch.tensor(float(ch), dtype=torch.float32)))
    if mut == "drop_key":
        k, v = k[:, :T - 1], v[:, :T - 1]
    elif mut == "pad_key":
        k, v = torch.cat([k, torch.zeros_like(k[:, :1])], 1), torch.cat([v, torch.zeros_like(v[:, :1])], 1)
    Tk = k.shape[1]
    nkb = (Tk + 31) // 32
    parts = []
    for g in range(kg):
        m = torch.full(q.shape[:2], -1e30)
        l = torch.zeros(q.shape[:2])
        o = torch.zeros_like(q)
        for kb in range(g, nkb, kg):
            kk, vv = k[:, kb * 32:kb * 32 + 32], v[:, kb * 32:kb * 32 + 32]
            S = _pair(q, kk.transpose(1, 2), b_lo=mut != "s_cross") if f32 else q @ kk.transpose(1, 2)
            m_new = torch.maximum(m, S.amax(-1) * c)
            alpha = torch.exp2(m - m_new)
            p = torch.exp2(_fma(S, c, -m_new[..., None]))
            l = _fma(l, alpha.double(), p.sum(-1))
            o = o * alpha[..., None]
            o = o + (_pair(p, vv, a_lo=mut != "p_lo") if f32 else _bf(p) @ vv)
            m = m_new
        parts.append((m, l, o))
    m, l, o = parts[0]
    for m1, l1, o1 in parts[1:]:
        m_new = torch.maximum(m, m1)
        a0, a1 = torch.exp2(m - m_new), torch.exp2(m1 - m_new)
        if mut == "merge_a1":
            a1 = torch.ones_like(a1)
        l = _fma(l, a0.double(), l1 * a1)
        o = _fma(o, a0[..., None].double(), o1 * a1[..., None])
        m = m_new
    out = AR.merge_heads(o * (1.0 / l)[..., None], B)
    return (out if f32 else out.bfloat16()), (m + torch.log2(l)).view(B, heads, T)


def emu_backward(qkv, out, dout, lse2, heads, mut=None):
    """k_attn_bwd_D + k_attn_bwd_dq + k_attn_bwd_dkv -> dqkv (B, T, 3C) fp32.  Mutations: ``dp_cross``: dP without its hi lo term; ``ds_bf16``: dS
    rounded to a single bf16; ``d_half``: D summed over half the channels; ``drop_key``: the last valid key is masked in the dQ kernel;
    ``drop_query``: the last query row contributes nothing to dK and dV."""
    B, T = qkv.shape[:2]
    q, k, v = (t.float() for t in AR.heads_of(qkv, heads))
    o, g = _heads32(out, heads), _heads32(dout, heads)
    l2 = lse2.float().reshape(-1, T, 1)
    ch = q.shape[-1]
    scale = float(1.0 / torch.sqrt(torch.tensor(float(ch), dtype=torch.float32)))
    c = float(torch.tensor(AR.LOG2E, dtype=torch.float32) * torch.tensor(scale, dtype=torch.float32))
    n = ch // 2 if mut == "d_half" else ch
    D = torch.zeros(q.shape[:2])
    for i in range(n):
        D = _fma(o[..., i], g[..., i].double(), D)
    p = torch.exp2(_fma(_pair(q, k.transpose(1, 2)), c, -l2))
    ds = p * (_pair(g, v.transpose(1, 2), b_lo=mut != "dp_cross") - D[..., None])
    p_q, ds_q = p.clone(), ds.clone()                                       # the dQ kernel's view (a lane = one query) ...
    if mut == "drop_key":
        ds_q[:, :, T - 1] = 0
    p_k, ds_k = p.clone(), ds.clone()                                       # ... and the dK / dV kernel's (a lane = one key)
    if mut == "drop_query":
        p_k[:, T - 1], ds_k[:, T - 1] = 0, 0
    lo = mut != "ds_bf16"
    dq = _pair(k.transpose(1, 2), ds_q.transpose(1, 2), b_lo=lo).transpose(1, 2) * scale          # dQ^T += K^T dS^T: dS is the B operand
    dk = _pair(q.transpose(1, 2), ds_k, b_lo=lo).transpose(1, 2) * scale                          # dK^T += Q^T dS
    dv = _pair(g.transpose(1, 2), p_k).transpose(1, 2)                                            # dV^T += dO^T P
    return AR.merge_qkv(dq, dk, dv, B)


def _failures(family, shape, mut=None, bf16=False):
    """{output: (elements outside, worst ratio)} of the emulated forward (fp32 or bf16 form) and of the backward in isolation and chained"""
    B, T, heads, ch = shape
    qkv, dout = AR.make_inputs(family, shape)
    res = {}
    if bf16:
        qb = qkv.bfloat16()
        ref = AR.forward_ref(qb, heads)
        res["out_bf16"] = AR.check_le(emu_forward(qb, heads, AR.fwd_kg(B, T, heads), mut)[0], ref["out"], ref["out_bound"])
        return res
    ref = AR.forward_ref(qkv, heads)
    fwd_mut = mut if mut in ("s_cross", "p_lo", "drop_key", "pad_key", "merge_a1") else None
    out, lse2 = emu_forward(qkv, heads, AR.fwd_kg(B, T, heads), fwd_mut)
    res["out"] = AR.check_le(out, ref["out"], ref["out_bound"])
    res["lse2"] = AR.check_le(lse2, ref["lse2"], ref["lse2_bound"])
    bwd_mut = mut if mut in ("dp_cross", "ds_bf16", "d_half", "drop_key", "drop_query") else None
    o32, l32 = ref["out"].float(), ref["lse2"].float()                       # in isolation: out and lse2 from the reference, rounded to fp32
    r, b = AR.backward_ref(qkv, o32, dout, l32, heads)
    for k_, v_ in AR.backward_failures(emu_backward(qkv, o32, dout, l32, heads, bwd_mut), r, b, heads).items():
        res[k_] = v_
    if mut is None:                                                          # chained: the forward's own out and lse2, the reference from those
        r, b = AR.backward_ref(qkv, out, dout, lse2, heads)
        for k_, v_ in AR.backward_failures(emu_backward(qkv, out, dout, lse2, heads), r, b, heads).items():
            res["chained_" + k_] = v_
    return res


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_states_the_dispatched_path_and_covers_every_one():
    fwd, bwd = set(), set()
    for (B, T, heads, ch), chp, kgf, kgb in AR.CASES:
        assert ch % 8 == 0 and 8 <= ch <= 128 and B * heads <= 65535
        assert (chp, kgf, kgb) == (AR.chp_of(ch), AR.fwd_kg(B, T, heads), AR.bwd_kg(B, T, heads, ch)), (B, T, heads, ch)
        fwd.add((chp, kgf))
        bwd.add((chp, kgb))
    assert fwd == AR.FWD_PATHS and bwd == AR.BWD_PATHS
    big = [(c[0], c[1]) for c in AR.CASES if c[0][1] >= 128 and c[2] == 1]                  # one key group at T >= 128: by the grid alone
    assert {chp for _, chp in big} >= {32, 64} and all(((T + 127) // 128) * B * h > 512 for (B, T, h, _), _ in big)
    assert any(c[0][1] >= 128 and c[0][3] <= 64 and c[3] == 1 for c in AR.CASES)            # ... and so for the backward
    assert any(((c[0][1] + 31) // 32) % 2 == 1 and c[2] == 2 for c in AR.CASES)             # unequal key groups
    assert set(CPU_SHAPES) <= set(AR.SHAPES) and MUT_SHAPE in AR.SHAPES


def test_pair_constant_against_the_split_as_the_kernels_do_it():
    """the figures quoted next to ``U_PAIR``: remainder of the split, worst case and rms of one pair product, over 2^20 random operand pairs"""
    g = torch.Generator().manual_seed(3)
    x, y = (torch.randn(1 << 20, generator=g).double() * torch.exp2(torch.randint(-20, 20, (1 << 20,), generator=g).double()) for _ in range(2))
    x, y = x.float(), y.float()
    (xh, xl), (yh, yl) = _split(x), _split(y)
    X, Y = x.double(), y.double()
    assert bool((xh.double() + (x - xh).double() == X).all())                               # x - hi is exact in fp32
    assert float(((X - xh.double() - xl.double()).abs() / X.abs()).max()) <= 2.0 ** -17
    rel = ((xh.double() * yh.double() + xh.double() * yl.double() + xl.double() * yh.double() - X * Y).abs() / (X * Y).abs())
    assert float(rel.max()) < 2.0 ** -15
    assert float(rel.square().mean().sqrt()) < 2.0 ** -17.5 and 3 * float(rel.square().mean().sqrt()) < AR.U_PAIR
    assert float((rel > AR.U_PAIR).double().mean()) < 0.01
    top = (torch.frexp(x)[0].abs() >= 0.75) & (torch.frexp(y)[0].abs() >= 0.75)              # both in the upper half of their binade
    assert float(rel[top].max()) < AR.U_PAIR


def test_families_are_what_they_claim():
    shape = (1, 129, 1, 32)
    qkv, _ = AR.make_inputs("dominant", shape)
    q, k, _ = AR.heads_of(qkv, 1)
    S = (q @ k.transpose(1, 2)) / math.sqrt(32)
    assert bool((S.argmax(-1) == 128).all()) and float(S[..., 128].min()) > 9.0             # every row's maximum is the last key, alone in its block
    assert float(S[..., :128].amax(-1).min()) > 7.0                                        # ... after the running maximum has moved already
    P = torch.softmax(S, -1)
    assert float(P.amax(-1).min()) > 0.4
    qkv, dout = AR.make_inputs("zero_v_tail", shape)
    assert float(AR.heads_of(qkv, 1)[2][:, -1].abs().max()) == 0 and float(dout[:, -1].abs().max()) == 0
    flat = torch.softmax(torch.einsum("ntc,nsc->nts", *AR.heads_of(AR.make_inputs("random", shape)[0], 1)[:2]) / math.sqrt(32), -1)
    peak = torch.softmax(torch.einsum("ntc,nsc->nts", *AR.heads_of(AR.make_inputs("peaked", shape)[0], 1)[:2]) / math.sqrt(32), -1)
    assert float(peak.amax(-1).median()) > 0.5 > float(flat.amax(-1).median())


# ------------------------------------------------------------------------------------------------ the kernels' arithmetic is accepted
@pytest.mark.parametrize("shape", CPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("family", AR.FAMILIES)
def test_bounds_accept_the_kernel_arithmetic(family, shape):
    res = _failures(family, shape)
    res.update(_failures(family, shape, bf16=True))
    print(family, shape, {k: round(v[1], 3) for k, v in res.items()})
    assert sum(v[0] for v in res.values()) == 0, res
    assert all(math.isfinite(v[1]) for v in res.values())
    if family == "zero_v_tail":                                             # the bound of a row that must be exactly zero is zero
        qkv, dout = AR.make_inputs(family, shape)
        ref = AR.forward_ref(qkv, shape[2])
        _, b = AR.backward_ref(qkv, ref["out"].float(), dout, ref["lse2"].float(), shape[2])
        assert float(AR.grad_parts(b, shape[2])["dq"][:, -1].abs().max()) == 0


# ------------------------------------------------------------------------------------------------ subtly wrong kernels are rejected
# mutation -> (the family that catches it on MUT_SHAPE, the outputs of which at least one must leave its bound, bf16 form)
MUTATIONS = {
    "s_cross": ("peaked", ("out", "lse2"), False),          # S without hi lo: the logit error 2^-9 A_S reaches the weights only where the softmax is sharp
    "dp_cross": ("offset", ("dq", "dk"), False),            # dP without hi lo: |dO| |v| is large and free of cancellation at v + 50
    "p_lo": ("dominant", ("out",), False),                  # P as one bf16 in P V: five keys hold the weight, their roundings do not average out
    "ds_bf16": ("random", ("dq", "dk"), False),             # dS as one bf16
    "drop_key": ("dominant", ("out", "lse2", "dq"), False),  # the last valid key: it carries most of every row's weight
    "pad_key": ("random", ("out", "lse2"), False),          # a zero key past T at logit 0: weight ~ 1 / T
    "merge_a1": ("dominant", ("out", "lse2"), False),       # the second group's (O, l) not rescaled: its maximum is lower by 1.6 / ln 2
    "d_half": ("random", ("dq", "dk"), False),              # D over half the channels
    "drop_query": ("random", ("dk", "dv"), False),          # the last query row's share of dK and dV
}


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_bounds_reject_the_mutation(mut):
    family, outputs, bf16 = MUTATIONS[mut]
    assert family in AR.FAMILIES and MUT_SHAPE in AR.SHAPES
    clean = _failures(family, MUT_SHAPE, bf16=bf16)
    assert sum(v[0] for v in clean.values()) == 0                           # (the family passes unmutated)
    res = _failures(family, MUT_SHAPE, mut, bf16=bf16)
    print(mut, family, {k: (v[0], round(v[1], 2)) for k, v in res.items()})
    assert all(res[o][0] > 0 and res[o][1] > 1 for o in outputs), res


def test_bf16_form_rejects_a_padded_and_a_dropped_key():
    """the bf16 form's own bound (2^-8 of A for the rounding of P): a padded key at logit 0 and a masked last key leave it as well"""
    for mut, family in (("pad_key", "random"), ("drop_key", "dominant")):
        res = _failures(family, (2, 33, 2, 24), mut, bf16=True)
        assert res["out_bf16"][0] > 0, (mut, res)
