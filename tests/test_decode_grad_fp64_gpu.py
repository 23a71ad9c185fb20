"""``ssdnerf_point_decode_backward`` (csrc/decode_bwd.hip) against the float64 reference and the derived bounds of tests/_decode_grad_ref.py, on the seeded families that
tests/test_decode_grad_bounds_cpu.py proves the bounds on.  The pipeline is split at the workspace (``ssdnerf_point_decode_backward_layout``): the tests call the
C ABI with a workspace tensor of their own and read the intermediates back.
  * per sample: ``counters`` are exact, every slot is identified through its keys and every sample with a gradient is present exactly once, ``pos`` is within the
    coordinate bound with the key its floor, ``gfeat`` inside ``B_gf`` -- k_decode_bwd_feat (fp32 and fp16 planes, colour and density-only) under the VALU bound,
    the opt-in k_decode_bwd_feat_mfma (flag 0x100) under the MFMA-class bound;
  * per texel: ``grad_code`` against the float64 scatter of the kernel's own workspace under the reduction bound (k_decode_bwd_bin_owned + k_decode_bwd_sum), on every
    texel of every reduction family; a texel no sample touches is exactly 0;
  * end to end: ``TriPlaneDecoder.point_decode`` + ``torch.autograd.grad`` (``_PointDecodeFn``: cached workspace, offsets from the point counts) under the end-to-end
    per-texel bound, also for a smaller problem behind a larger one on the same decoder (stale workspace contents).
The control runs the MFMA variant against the VALU bound on the coherent family.
The per-sample bounds are worst-case (coordinate uncertainty C_X u size on every gather, u times the partial sums of every chain, carried through 64 hidden units):
on random planes, where the coordinate term leads, the default kernel sits at 0.01 - 0.03 of them (profiles/decode_grad_bounds.json), like ``point_decode``'s
colours under the forward's, and at 0.10 on the coherent family; the reduction bound is met at up to ~0.5.

``python tests/test_decode_grad_fp64_gpu.py OUT.json`` writes the worst |kernel - reference| / bound per stage, family and variant, and the control's counts
(profiles/decode_grad_bounds.json is such a run)."""
import ctypes
import json
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _decode_grad_ref as G

pytestmark = pytest.mark.gpu

MFMA_FLAG = 0x100
MULTI_SCENE = [n for n, v in G.SAMPLE_FAMILIES.items() if len(v[3]) > 1]


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def layout(S, total, H, W):
    from ssdnerf_amd import _cabi as C
    out = (ctypes.c_uint64 * 6)()
    C.lib().ssdnerf_point_decode_backward_layout(C.u32(S), C.u32(total), C.u32(H), C.u32(W), out)
    return SimpleNamespace(counters=int(out[0]), keys=int(out[1]), pos=int(out[2]), gfeat=int(out[3]), partial=int(out[4]), K=int(out[5]),
                           bytes=int(C.lib().ssdnerf_point_decode_backward_workspace(C.u32(S), C.u32(total), C.u32(H), C.u32(W))))


def run_backward(c, density_only=False, mfma=False):
    """one ``ssdnerf_point_decode_backward`` on a workspace of the test's own (filled with 0xff first: whatever the kernels do not write reads as NaN / key -1):
    namespace of counters [S], keys [3, total], pos [3, total, 2], gfeat [3, total, 6], grad_code [S, 3, 6, H, W] (numpy) and K"""
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd.decoders import pack_triplanes
    S, total, H, W = c.S, len(c.xyz), c.H, c.W
    lay = layout(S, total, H, W)
    assert lay.counters < lay.keys < lay.pos < lay.gfeat < lay.partial < lay.bytes
    planes = pack_triplanes(cu(c.code), torch.float16 if c.fp16 else torch.float32)
    ws = torch.full((lay.bytes,), 0xFF, dtype=torch.uint8, device="cuda")
    grad = torch.full((S, 3, 6, H, W), float("nan"), dtype=torch.float32, device="cuda")
    P, xyz, offsets, gs = cu(c.P.astype(np.float32)), cu(c.xyz), cu(c.offsets.astype(np.int32)), cu(c.g_sigma)
    dirs, grgb = (None, None) if density_only else (cu(c.dirs), cu(c.g_rgb))
    C.check(C.lib().ssdnerf_point_decode_backward(C.ptr(planes), C.dtype_code(planes) | (MFMA_FLAG if mfma else 0), C.u32(S), C.u32(H), C.u32(W), C.ptr(P), C.ptr(xyz),
                                                  C.ptr(dirs), C.ptr(offsets), C.u32(total), C.f32(c.sat), C.ptr(gs), C.ptr(grgb), C.ptr(grad), C.ptr(ws),
                                                  ctypes.c_size_t(lay.bytes), C.stream()), "point_decode_backward")
    torch.cuda.synchronize()
    w = ws[:lay.partial].cpu().numpy()
    take = lambda off, n, dt: w[off:off + 4 * n].view(dt)
    return SimpleNamespace(counters=take(lay.counters, S * 32, np.uint32).reshape(S, 32)[:, 0].astype(np.int64), keys=take(lay.keys, 3 * total, np.uint32).reshape(3, total),
                           pos=take(lay.pos, 6 * total, np.float32).reshape(3, total, 2), gfeat=take(lay.gfeat, 18 * total, np.float32).reshape(3, total, 6),
                           grad_code=grad.cpu().numpy(), K=lay.K)


# ------------------------------------------------------------------------------------------------ per sample
def identify(c, out, active):
    """the sample of every compacted slot, through the keys of planes 0 and 1 (unique within a scene by construction): (slots, samples) index arrays.  Asserts the
    counters and that the slots hold every sample with a gradient exactly once."""
    ref = G.sample_keys(c.xyz, c.H, c.W).astype(np.uint64)
    slots, samples = [], []
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        live = a + np.flatnonzero(active[a:b])
        assert int(out.counters[s]) == len(live), (s, int(out.counters[s]), len(live))
        sl = np.arange(a, a + len(live))
        want, got = (ref[0, live] << np.uint64(32)) | ref[1, live], (out.keys[0, sl].astype(np.uint64) << np.uint64(32)) | out.keys[1, sl].astype(np.uint64)
        ow, og = np.argsort(want), np.argsort(got)
        assert np.array_equal(want[ow], got[og]), ("slots do not hold the scene's samples exactly once", s)
        slots.append(sl[og]); samples.append(live[ow])
    return np.concatenate(slots), np.concatenate(samples)


def sample_failures(name, density_only, mfma, bound_mfma=None):
    """{check: (elements outside, worst ratio)} of the first stage of one family; ``bound_mfma``: the arithmetic class of the bound when it is not the kernel's"""
    c, gf, B, active = G.sample_reference(name, mfma if bound_mfma is None else bound_mfma, density_only)
    out = run_backward(c, density_only, mfma)
    slots, samples = identify(c, out, active)
    assert np.array_equal(out.keys[:, slots], G.sample_keys(c.xyz, c.H, c.W)[:, samples])
    ix, iy = G._texel_coords(c.xyz, c.H, c.W)
    dx, dy = np.full_like(ix[:, samples], G.C_X * G.U32 * c.W), np.full_like(ix[:, samples], G.C_X * G.U32 * c.H)
    got = out.gfeat[:, slots].transpose(1, 2, 0).reshape(-1, 18)             # gf[c * 3 + p] = gfeat[p][slot][c]
    res = dict(gfeat=G.check_le(got, gf[samples], B[samples]), pos_x=G.check_le(out.pos[:, slots, 0], ix[:, samples], dx),
               pos_y=G.check_le(out.pos[:, slots, 1], iy[:, samples], dy))
    # the reduction of exactly these intermediates, including the texels of an empty scene and of a scene without gradients: all exactly 0
    ref, bnd = G.workspace_scatter_ref(out.counters, c.offsets, out.pos, out.gfeat, c.S, c.H, c.W, out.K)
    res["grad_code"] = G.check_le(out.grad_code, ref, bnd)
    return res


def n_failures(res):
    return sum(v[0] for v in res.values())


@pytest.mark.parametrize("density_only", [False, True], ids=["colour", "density-only"])
@pytest.mark.parametrize("name", list(G.SAMPLE_FAMILIES))
def test_first_stage_meets_the_per_sample_bounds(name, density_only):
    res = sample_failures(name, density_only, False)
    print(name, density_only, {k: round(v[1], 3) for k, v in res.items()})
    assert n_failures(res) == 0, res


@pytest.mark.parametrize("name", list(G.SAMPLE_FAMILIES))
def test_mfma_first_stage_meets_the_mfma_class_bounds(name):
    res = sample_failures(name, False, True)
    print(name, "mfma", {k: round(v[1], 3) for k, v in res.items()})
    assert n_failures(res) == 0, res


def run_control():
    """the coherent family under the VALU bound: {"mfma": (elements outside, worst ratio) of k_decode_bwd_feat_mfma, "valu": of the default kernel}"""
    return {"mfma": sample_failures("coherent", False, True, bound_mfma=False)["gfeat"], "valu": sample_failures("coherent", False, False)["gfeat"]}


def test_mfma_first_stage_leaves_the_valu_bound_that_the_default_kernel_meets():
    """the control: on the coherent family the bf16-pair products of the MFMA variant must put at least one sample outside the VALU bound, and the default kernel none.
    The family's flat planes let ONE feature, the last of the chain, carry every pre-activation: the pair residual of that feature (123 u of the 128 u the split allows)
    is a relative error common to all 64 hidden units, which the all-positive heads add up, while the VALU chain rounds small partial sums until its last fma.  Under
    the worst-case-sum form of the layer bounds, (K + 1) u sum |terms|, and planes of eighteen comparable features the variant sat at 0.26 of the VALU bound (default
    kernel 0.034): that form could not tell the two apart, so the VALU class is held to the partial sums of the kernel's own order (``G.chain_rounding``).  Measured
    on an MI355X: the variant has 29794 of 3001 x 18 elements outside (worst 2.53), the default kernel none (worst 0.098)."""
    res = run_control()
    print("control: mfma", res["mfma"], "valu", res["valu"])
    assert res["valu"][0] == 0, res
    assert res["mfma"][0] >= 1 and res["mfma"][1] > 1.0, res


# ------------------------------------------------------------------------------------------------ per texel: the reduction
def reduction_failures(kind, planes):
    c = G.reduction_case(kind, planes)
    out = run_backward(c)
    assert np.array_equal(out.counters, np.asarray(c.sizes))
    if kind in ("two-scenes", "empty-split"):
        assert out.K >= 2, out.K
    ref, bnd = G.workspace_scatter_ref(out.counters, c.offsets, out.pos, out.gfeat, c.S, c.H, c.W, out.K)
    return dict(grad_code=G.check_le(out.grad_code, ref, bnd), untouched=(int((out.grad_code[bnd == 0] != 0).sum()), 0.0))


@pytest.mark.parametrize("kind,planes", G.REDUCTION_CASES)
def test_reduction_meets_the_per_texel_bound_of_its_own_workspace(kind, planes):
    res = reduction_failures(kind, planes)
    print(kind, planes, {k: round(v[1], 3) for k, v in res.items()})
    assert n_failures(res) == 0, res


# ------------------------------------------------------------------------------------------------ end to end
def make_decoder(c):
    from ssdnerf_amd.decoders import TriPlaneDecoder
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256)
    dec.load_state_dict(c.sd, strict=False)
    dec = dec.cuda().train(True).requires_grad_(False)
    assert dec.sigmoid_saturation == c.sat and np.array_equal(dec.packed_params().cpu().numpy().view(np.uint32), c.P.view(np.uint32))
    return dec


def e2e_failures(dec, name):
    """``point_decode`` + ``autograd.grad`` of one multi-scene family on ``dec`` against the end-to-end per-texel bound"""
    c, gf, B, _ = G.sample_reference(name, False, False)
    dec.plane_dtype = torch.float16 if c.fp16 else torch.float32
    assert dec.fused_code_grad and not dec.decode_bwd_feat_mfma
    code = cu(c.code).requires_grad_(True)
    cut = [(int(c.offsets[s]), int(c.offsets[s + 1])) for s in range(c.S)]
    sig, rgb, num = dec.point_decode([cu(c.xyz[a:b]) for a, b in cut], [cu(c.dirs[a:b]) for a, b in cut], code)
    assert num == list(c.sizes)
    (got,) = torch.autograd.grad((sig, rgb), code, (cu(c.g_sigma), cu(c.g_rgb)))
    got = got.cpu().numpy()
    K = layout(c.S, len(c.xyz), c.H, c.W).K
    bad, worst = 0, 0.0
    for s, (a, b) in enumerate(cut):
        ref, bnd = G.scatter_e2e_ref(c.xyz[a:b], gf[a:b], B[a:b], c.H, c.W, K)
        r = G.check_le(got[s], ref, bnd)
        bad, worst = bad + r[0], max(worst, r[1])
    return dict(grad_code=(bad, worst))


@pytest.mark.parametrize("name", MULTI_SCENE)
def test_point_decode_gradient_meets_the_end_to_end_bound(name):
    res = e2e_failures(make_decoder(G.sample_case(name)), name)
    print(name, {k: round(v[1], 3) for k, v in res.items()})
    assert n_failures(res) == 0, res


def run_stale():
    dec = make_decoder(G.sample_case("square-fp16-straddle"))                # 1377 samples, four scenes of 128 x 128 planes, then 512 samples, two scenes of 40 x 72
    return [e2e_failures(dec, n) for n in ("square-fp16-straddle", "ragged-fp32-aligned", "square-fp16-straddle")]


def test_a_smaller_problem_behind_a_larger_one_on_the_same_decoder_meets_the_bound():
    """the decoder's cached workspace holds the larger problem's counters, keys and partial images when the smaller one runs"""
    res = run_stale()
    print([{k: round(v[1], 3) for k, v in r.items()} for r in res])
    assert sum(n_failures(r) for r in res) == 0, res


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}

    def note(key, res, must_pass=True):
        worst[key] = {k: round(v[1], 4) for k, v in res.items() if k != "untouched"}
        assert not must_pass or n_failures(res) == 0, (key, res)

    for name in G.SAMPLE_FAMILIES:
        note(f"per-sample/{name}/valu/colour", sample_failures(name, False, False))
        note(f"per-sample/{name}/valu/density-only", sample_failures(name, True, False))
        note(f"per-sample/{name}/mfma/colour", sample_failures(name, False, True))
    for kind, planes in G.REDUCTION_CASES:
        note(f"reduction/{kind}/{planes}", reduction_failures(kind, planes))
    for name in MULTI_SCENE:
        note(f"end-to-end/{name}", e2e_failures(make_decoder(G.sample_case(name)), name))
    for i, r in enumerate(run_stale()):
        note(f"end-to-end/stale-workspace/{i}", r)
    ctl = run_control()
    return worst, {k: dict(elements_outside=v[0], worst_ratio=round(v[1], 4)) for k, v in ctl.items()}


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst, control = measure()
    out = dict(what="worst |kernel - fp64 reference| / bound per stage, family and variant, over every seeded case of tests/test_decode_grad_fp64_gpu.py",
               device=torch.cuda.get_device_name(0), c_exp=G.C_EXP, c_x=G.C_X, pair=G.PAIR, worst_ratio=worst, control_coherent_gfeat_under_valu_bound=control)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
