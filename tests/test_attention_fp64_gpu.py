"""The self-attention kernels (csrc/attention.hip: k_attn_fwd in its bf16 and fp32-class forms, k_attn_bwd_D, k_attn_bwd_dq, k_attn_bwd_dkv, through
``ssdnerf_amd.unet_fast``) against the float64 references and per-element bounds of tests/_attention_ref.py, on the seeded families that
tests/test_attention_bounds_cpu.py proves the bounds on: flat, peaked and offset softmaxes, rows whose maximum arrives in the last, ragged key
block, zero rows.  Zero elements may lie outside their bound; there is no norm and no allowance.

Every kernel path that the library dispatches on its own is reached BY SHAPE ALONE (``_attention_ref.CASES`` carries the padded head width and the
key-group count that each shape selects, forward and backward): the library reads its path switches from the environment once per process, so
no test sets one.  The forms that only those switches select -- one or two waves per block (``SSDNERF_ATTN_WPB``) -- are out of scope here.

On an MI355X every kernel meets every bound as derived -- no term had to be added and no kernel changed.  The worst error / bound ratios
(profiles/attention_bounds.json, per kernel, family and output): 0.32 for the fp32 forward, 0.72 for its saved log-sum-exp, 0.84 for the bf16
forward, 0.65 for the backward, each on the ``peaked`` family; the emulation of tests/test_attention_bounds_cpu.py gives 0.07 / 0.42 / 0.73 / 0.39.

``python tests/test_attention_fp64_gpu.py OUT.json`` runs every case and writes those ratios."""
import functools
import json
import sys

import pytest
import torch

import _attention_ref as AR

pytestmark = pytest.mark.gpu

_ids = lambda s: "x".join(map(str, s))
every_case = lambda f: pytest.mark.parametrize("shape", AR.SHAPES, ids=_ids)(pytest.mark.parametrize("family", AR.FAMILIES)(f))


def _uf():
    from ssdnerf_amd import unet_fast
    return unet_fast


@functools.lru_cache(maxsize=None)
def case(family, shape):
    """inputs on the device and the float64 references that depend on them alone; computed once per (family, shape) and never written to"""
    heads = shape[2]
    qkv, dout = (t.cuda() for t in AR.make_inputs(family, shape))
    qb = qkv.bfloat16()
    ref = AR.forward_ref(qkv, heads)
    out32, lse32 = ref["out"].float(), ref["lse2"].float()                  # the backward in isolation: out and lse2 of the reference, rounded to fp32
    bwd = AR.backward_ref(qkv, out32, dout, lse32, heads)
    return dict(qkv=qkv, dout=dout, qb=qb, ref=ref, ref_bf16=AR.forward_ref(qb, heads), out32=out32, lse32=lse32, bwd=bwd)


@pytest.fixture(scope="module", autouse=True)
def _release_the_cases():
    yield
    case.cache_clear()                                                      # (about 2 GB of references at the two large shapes)
    torch.cuda.empty_cache()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _report(name, family, shape, res):
    print(name, family, shape, {k: round(v[1], 3) for k, v in res.items()})
    assert sum(v[0] for v in res.values()) == 0, (name, family, shape, res)


def forward_f32(c, heads):
    out, lse2 = _uf().attention_qkv_f32_with_lse(c["qkv"], heads)
    r = c["ref"]
    return out, lse2, dict(out=AR.check_le(out, r["out"], r["out_bound"]), lse2=AR.check_le(lse2, r["lse2"], r["lse2_bound"]))


def forward_bf16(c, heads):
    out = _uf().attention_qkv_bf16(c["qb"], heads)
    r = c["ref_bf16"]
    return out, dict(out=AR.check_le(out, r["out"], r["out_bound"]))


def backward_isolated(c, heads):
    got = _uf().attention_qkv_f32_backward(c["qkv"], c["out32"], c["dout"], c["lse32"], heads)
    return got, AR.backward_failures(got, *c["bwd"], heads)


def backward_chained(c, heads):
    out, lse2 = _uf().attention_qkv_f32_with_lse(c["qkv"], heads)
    got = _uf().attention_qkv_f32_backward(c["qkv"], out, c["dout"], lse2, heads)
    return got, AR.backward_failures(got, *AR.backward_ref(c["qkv"], out, c["dout"], lse2, heads), heads)


def _zero_rows(family, got, heads):
    """``zero_v_tail``: the last query's dout row is zero, so dS of that row is p (0 - 0) and its dQ row must be exactly zero"""
    if family == "zero_v_tail":
        assert float(AR.grad_parts(got, heads)["dq"][:, -1].abs().max()) == 0.0
        assert bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------ forward
@every_case
def test_forward_fp32_meets_the_fp64_bounds(family, shape):
    c, heads = case(family, shape), shape[2]
    got = _uf().attention_qkv(c["qkv"], heads)
    assert got.dtype == torch.float32 and got.shape == c["ref"]["out"].shape
    _report("forward_f32", family, shape, dict(out=AR.check_le(got, c["ref"]["out"], c["ref"]["out_bound"])))


@every_case
def test_forward_bf16_meets_the_fp64_bounds_through_both_entries(family, shape):
    c, heads = case(family, shape), shape[2]
    got, res = forward_bf16(c, heads)
    assert got.dtype == torch.bfloat16 and _same(got, _uf().attention_qkv(c["qb"], heads))
    _report("forward_bf16", family, shape, res)


@every_case
def test_forward_with_lse_is_the_plain_forward_and_its_lse_meets_the_bound(family, shape):
    c, heads = case(family, shape), shape[2]
    out, lse2, res = forward_f32(c, heads)
    assert _same(out, _uf().attention_qkv(c["qkv"], heads))
    assert lse2.shape == (shape[0], heads, shape[1])
    _report("forward_f32_lse", family, shape, res)


# ------------------------------------------------------------------------------------------------ backward
@every_case
def test_backward_in_isolation_meets_the_fp64_bounds(family, shape):
    c, heads = case(family, shape), shape[2]
    got, res = backward_isolated(c, heads)
    _report("backward", family, shape, res)
    _zero_rows(family, got, heads)


@every_case
def test_backward_chained_to_the_forward_meets_the_fp64_bounds(family, shape):
    c, heads = case(family, shape), shape[2]
    got, res = backward_chained(c, heads)
    _report("backward_chained", family, shape, res)
    _zero_rows(family, got, heads)


# ------------------------------------------------------------------------------------------------ determinism
@every_case
def test_two_calls_return_identical_bits_in_both_directions(family, shape):
    c, heads = case(family, shape), shape[2]
    (o1, l1, _), (o2, l2, _) = forward_f32(c, heads), forward_f32(c, heads)
    assert _same(o1, o2) and _same(l1, l2)
    assert _same(forward_bf16(c, heads)[0], forward_bf16(c, heads)[0])
    assert _same(backward_isolated(c, heads)[0], backward_isolated(c, heads)[0])


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}

    def note(key, res):
        for k, v in res.items():
            worst.setdefault(key, {})[k] = max(worst.get(key, {}).get(k, 0.0), round(v[1], 4))

    for family in AR.FAMILIES:
        for shape in AR.SHAPES:
            c, heads = case(family, shape), shape[2]
            note("attention_fwd_f32/" + family, forward_f32(c, heads)[2])
            note("attention_fwd_bf16/" + family, forward_bf16(c, heads)[1])
            note("attention_bwd/" + family, backward_isolated(c, heads)[1])
            note("attention_bwd_chained/" + family, backward_chained(c, heads)[1])
    return worst


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = dict(what="worst |kernel - fp64 reference| / bound per output, over every shape of tests/test_attention_fp64_gpu.py",
               device=torch.cuda.get_device_name(0), u_pair=AR.U_PAIR, c_bound=AR.C_BOUND, worst_ratio=measure())
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
