"""The decoder-parameter gradient of the fused decode, on the CPU (no GPU): the gcc build of the kernel's arithmetic header (csrc/decode_bwd_params_math.h through
tests/host/decode_bwd_params_host.c; correctly rounded exp2 and division where the device has its hardware units: it stands for the arithmetic class, not for the
kernel's bits) against the float64 reference and the derived bounds of tests/_decode_param_grad_ref.py, element by element, on every family of
``_decode_grad_ref.SAMPLE_FAMILIES`` (at most 3001 samples per scene; an empty scene, blocks that straddle scenes, 30 % dead samples, fp16 planes, the clamp's knees);
against float64 autograd through ``TriPlaneDecoder.point_decode_eager``; and the controls: two mutated references are rejected, and the bounds are small against the sums
they guard.  Plus the host-side surface: the constructor switch, the exported symbols, the argument checks that need no device."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import _decode_grad_ref as G
import _decode_param_grad_ref as PG
import _render_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FAMILIES = list(G.SAMPLE_FAMILIES)


@functools.lru_cache(maxsize=None)
def host():
    so = os.path.join(tempfile.mkdtemp(prefix="decode_param_grad_host"), "decode_bwd_params_host.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tests", "host", "decode_bwd_params_host.c"), "-o", so, "-lm"],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.decode_bwd_params_points.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def host_gradient(name):
    """the packed gradient [N_PARAMS] fp32 of the host build over every scene of a family (scene by scene, added in scene order); shared, read-only"""
    c = G.sample_case(name)
    sh = np.ascontiguousarray(RR.sh4(c.dirs)[0].astype(F))                   # (the float64 SH rounded once: within the SH bound of every component)
    grad = np.zeros(PG.N_PARAMS, F)
    for s in range(c.S):
        a, b = int(c.offsets[s]), int(c.offsets[s + 1])
        if a == b:
            continue
        planes = np.zeros((3, c.H, c.W, 8), F)
        planes[..., :6] = c.code[s].transpose(0, 2, 3, 1)
        host().decode_bwd_params_points(_p(planes), ctypes.c_uint32(c.H), ctypes.c_uint32(c.W), _p(np.ascontiguousarray(c.P, F)), _p(np.ascontiguousarray(c.xyz[a:b])),
                                        _p(np.ascontiguousarray(sh[a:b])), ctypes.c_uint32(b - a), ctypes.c_float(c.sat), _p(np.ascontiguousarray(c.g_sigma[a:b])),
                                        _p(np.ascontiguousarray(c.g_rgb[a:b])), _p(grad))
    return grad


# ------------------------------------------------------------------------------------------------ the bounds hold
@pytest.mark.parametrize("name", FAMILIES)
def test_host_build_meets_the_bound_of_every_parameter_element(name):
    r = PG.reference(name)
    got = host_gradient(name)
    bad, worst = PG.check_le(got, r.ref, r.bound)
    print(name, "live", r.n_live, "worst ratio", round(worst, 3))
    assert bad == 0, (bad, worst)
    assert not got[r.bound == 0].any() and (r.bound > 0).sum() == PG.N_PARAMS - 64              # nothing but the padding column is unreached, and that is exactly 0
    assert not got[:1536].reshape(64, 24)[:, 23].any()


# ------------------------------------------------------------------------------------------------ ... against autograd
class _SH64(torch.nn.Module):
    """the float64 SH basis of tests/_render_ref.py in place of the HIP encoder (a CPU decoder in double precision)"""

    def forward(self, dirs):
        return torch.from_numpy(RR.sh4(dirs.detach().numpy())[0])


class _TruncExp64Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.exp(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        return g * y.clamp(min=G.CLAMP_LO, max=G.CLAMP_HI)


class _TruncExp64(torch.nn.Module):
    """``ssdnerf_amd.activation.TruncExp`` without its cast: that one evaluates exp in fp32 whatever its input (as the reference's does), which would leave an fp32
    rounding on the density branch of an otherwise float64 evaluation.  Same function, same clamp (the kernel's fp32 constants), in the input's precision."""

    def forward(self, x):
        return _TruncExp64Fn.apply(x)


@functools.lru_cache(maxsize=None)
def autograd_gradient(name):
    """{state-dict key: float64 gradient} of ``point_decode_eager`` on a ``.double()`` CPU decoder: grid_sample + four nn.Linear + autograd"""
    from ssdnerf_amd.decoders import TriPlaneDecoder
    c = G.sample_case(name)
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256)
    dec.load_state_dict(c.sd, strict=False)
    dec = dec.double().train(True)
    dec.dir_encoder = _SH64()
    assert type(dec.density_net[1]).__name__ == "TruncExp"
    dec.density_net[1] = _TruncExp64()
    assert dec.sigmoid_saturation == c.sat
    cut = [(int(c.offsets[s]), int(c.offsets[s + 1])) for s in range(c.S)]
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    sig, rgb, _ = dec.point_decode_eager([t64(c.xyz[a:b]) for a, b in cut], [t64(c.dirs[a:b]) for a, b in cut], t64(c.code))
    params = dict(dec.named_parameters())
    grads = torch.autograd.grad((sig, rgb), [params[k] for k in PG.NAMES], (t64(c.g_sigma), t64(c.g_rgb)))
    return {k: g.numpy() for k, g in zip(PG.NAMES, grads)}


@pytest.mark.parametrize("name", FAMILIES)
def test_reference_is_float64_autograd_and_the_host_build_agrees_with_it(name):
    """the reference and autograd are two float64 evaluations of one function: they agree to 1e-9 of sum |term| (thousands of float64 roundings are below 1e-12 of it);
    the host build then lies inside the bound around autograd's value, widened by that 1e-9"""
    r, want, got = PG.reference(name), autograd_gradient(name), PG.unpack(host_gradient(name))
    ref, bnd, mag = PG.unpack(r.ref), PG.unpack(r.bound), PG.unpack(r.mag)
    for k in PG.NAMES:
        assert want[k].shape == ref[k].shape, k
        assert float((np.abs(want[k] - ref[k]) - 1e-9 * mag[k]).max()) <= 0.0, (name, k)
        bad, worst = PG.check_le(np.ascontiguousarray(got[k]), want[k], bnd[k] + 1e-9 * mag[k])
        assert bad == 0, (name, k, bad, worst)


# ------------------------------------------------------------------------------------------------ controls
@pytest.mark.parametrize("mutate", PG.MUTATIONS)
@pytest.mark.parametrize("name", FAMILIES)
def test_a_mutated_reference_is_rejected(name, mutate):
    """``db1-without-e``: the colour branch's share e_i missing from db1; ``dWc-untransposed``: dWc [3, 64] laid into the records' [64, 3] slot without the transposition.
    Every family has colour gradients, so both mutations touch every family: the host build must leave the (honest) bound around the mutated value."""
    honest, wrong = PG.reference(name), PG.reference(name, mutate)
    bad, worst = PG.check_le(host_gradient(name), wrong.ref, honest.bound)
    print(name, mutate, "elements outside", bad, "worst ratio", round(worst, 1))
    assert bad >= 1 and worst > 1.0
    changed = wrong.ref != honest.ref
    rec = np.zeros(PG.N_PARAMS, bool)
    rec[:1536].reshape(64, 24)[:, 18 if mutate == "db1-without-e" else slice(20, 23)] = True
    assert changed.any() and not changed[~rec].any()


@pytest.mark.parametrize("name", FAMILIES)
def test_the_bounds_are_small_against_the_sums_they_guard(name):
    """a bound that is a large share of sum |term| would accept a lost term: on at least 99 % of the elements some sample reaches, the bound is below 1e-3 of sum |term|"""
    r = PG.reference(name)
    reached = r.mag > 0
    share = float((r.bound[reached] < 1e-3 * r.mag[reached]).mean())
    print(name, "elements with bound < 1e-3 sum |term|:", round(share, 4), "worst bound / sum |term|", float((r.bound[reached] / r.mag[reached]).max()))
    assert share >= 0.99, (name, share)


def test_third_derivative_constant_of_the_local_silu_bound():
    u = np.linspace(-60.0, 60.0, 1200001)
    worst = float(np.abs(PG.silu3(u)).max())
    print("max |silu'''| on the grid", worst)
    assert worst < 0.40 < PG.L3                                               # (grid step 1e-4 and |silu''''| < 1: the maximum between grid points is within 1e-4 of it)


# ------------------------------------------------------------------------------------------------ the host-side surface
def test_param_grad_switch_of_the_decoder():
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.registry import build_module
    kw = dict(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64])
    assert TriPlaneDecoder(**kw).param_grad == TriPlaneDecoder.param_grad
    assert TriPlaneDecoder(param_grad="eager", **kw).param_grad == "eager" and TriPlaneDecoder(param_grad="fused", **kw).param_grad == "fused"
    assert build_module(dict(type="TriPlaneDecoder", param_grad="fused", **kw)).param_grad == "fused"          # a config's decoder dict may carry the key
    with pytest.raises(ValueError):
        TriPlaneDecoder(param_grad="hip", **kw)
    # a CPU tensor never takes the fused path, whatever the switch says
    dec = TriPlaneDecoder(param_grad="fused", **kw).train(True)
    code = torch.randn(1, 3, 6, 8, 8, requires_grad=True)
    assert not dec.fused_supported(code)
    sig, _, _ = dec.point_decode([torch.rand(5, 3) * 2 - 1], None, code, density_only=True)      # (the eager statement; the colour branch's SH encoder is GPU-only)
    sig.sum().backward()
    assert dec.base_net[0].weight.grad is not None and code.grad is not None


def test_unpack_mlp_grads_inverts_pack_mlp_params():
    """the eight tensors of a random state dict come back bit for bit and in their shapes: Wc transposed back, the biases (1,) and (3,)"""
    from ssdnerf_amd.decoders import MLP_PARAM_FLOATS, MLP_PARAM_KEYS, pack_mlp_params, unpack_mlp_grads
    shapes = [(64, 18), (64,), (1, 64), (1,), (64, 16), (64,), (3, 64), (3,)]
    gen = torch.Generator().manual_seed(7)
    sd = {k: torch.randn(shp, generator=gen) for k, shp in zip(MLP_PARAM_KEYS, shapes)}
    assert list(MLP_PARAM_KEYS) == list(PG.NAMES)
    packed = pack_mlp_params(sd, "cpu")
    assert packed.shape == (MLP_PARAM_FLOATS,) and not packed[:1536].view(64, 24)[:, 23].any()
    back = unpack_mlp_grads(packed)
    assert len(back) == 8
    for k, shp, got in zip(MLP_PARAM_KEYS, shapes, back):
        assert tuple(got.shape) == shp and torch.equal(got.contiguous().view(torch.int32), sd[k].view(torch.int32)), k
    for k, got in PG.unpack(packed.numpy()).items():                         # ... and the reference's own unpacking reads the same block the same way
        assert np.array_equal(got, sd[k].numpy()), k


def test_python_layout_offsets_are_the_headers():
    from ssdnerf_amd import decoders as D
    tmp = tempfile.mkdtemp(prefix="mlp_layout")
    src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "ssdnerf_hip.h"\n'
                'int main(void) { printf("%d %d %d %d\\n", SSDNERF_MLP_OFF_WD, SSDNERF_MLP_OFF_BD, SSDNERF_MLP_OFF_TAIL, SSDNERF_MLP_PARAM_FLOATS); return 0; }\n')
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    assert [int(v) for v in out.split()] == [D.MLP_OFF_WD, D.MLP_OFF_BD, D.MLP_OFF_TAIL, D.MLP_PARAM_FLOATS] == [1536, 2560, 2624, 2628]


def test_environment_sets_the_default_of_new_decoders():
    import sys
    prog = ("from ssdnerf_amd.decoders import TriPlaneDecoder as T; "
            "print(T.param_grad, T(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64]).param_grad)")
    # the switch is read when the module is imported: one fresh interpreter with it set; this process shows the other side
    out = subprocess.run([sys.executable, "-c", prog], cwd=ROOT, env=dict(os.environ, SSDNERF_DECODE_PARAM_GRAD="1"), capture_output=True, text=True, check=True).stdout
    assert out.split() == ["fused", "fused"], out
    from ssdnerf_amd.decoders import TriPlaneDecoder
    assert TriPlaneDecoder.param_grad == ("fused" if os.environ.get("SSDNERF_DECODE_PARAM_GRAD", "0") == "1" else "eager")


def test_entry_points_are_declared_exported_and_check_their_arguments_without_a_device():
    from ssdnerf_amd import _cabi as C, build
    header = open(os.path.join(ROOT, "include", "ssdnerf_hip.h")).read()
    assert "decode_bwd_params.hip" in build.SOURCES and "decode_bwd_params_math.h" in build.HEADERS
    for sym in ("ssdnerf_point_decode_backward_params_workspace", "ssdnerf_point_decode_backward_params"):
        assert sym in C.EXPORTS and f" {sym}(" in header
    lib = ctypes.CDLL(build.build())
    u32, f32, size_t = ctypes.c_uint32, ctypes.c_float, ctypes.c_size_t
    lib.ssdnerf_point_decode_backward_params_workspace.restype = size_t
    lib.ssdnerf_last_error.restype = ctypes.c_char_p
    rec = PG.N_PARAMS * 4
    assert lib.ssdnerf_point_decode_backward_params_workspace(u32(2), u32(3000), u32(2)) == 2 * rec                  # twelve groups on two blocks
    assert lib.ssdnerf_point_decode_backward_params_workspace(u32(2), u32(3000), u32(0)) == 12 * rec                 # one block per group below the default cap
    assert lib.ssdnerf_point_decode_backward_params_workspace(u32(2), u32(0), u32(0)) == rec
    buf = (ctypes.c_float * 64)()
    call = lambda planes, dtype, grad, ws, ws_bytes: lib.ssdnerf_point_decode_backward_params(
        planes, dtype, u32(1), u32(2), u32(2), buf, buf, buf, buf, u32(5), f32(0.001), buf, buf, grad, u32(0), ws, size_t(ws_bytes), None)
    assert call(buf, 0, None, buf, 1 << 20) == -1 and b"grad_params" in lib.ssdnerf_last_error()
    assert call(None, 0, buf, buf, 1 << 20) == -1 and b"null pointer" in lib.ssdnerf_last_error()
    assert call(buf, 0, buf, None, 1 << 20) == -1 and b"null pointer" in lib.ssdnerf_last_error()
    assert call(buf, 2, buf, buf, 1 << 20) == -1 and b"dtype" in lib.ssdnerf_last_error()
    assert call(buf, 0, buf, buf, rec - 1) == -3 and b"workspace" in lib.ssdnerf_last_error()
