"""The total-variation regulariser without a GPU: the float64 restatement against the reference's own values (tests/golden/tv_loss.npz), the
bounds of tests/_tv_ref.py met by an fp32 emulation of the kernel and broken by deliberately wrong variants, the C ABI's declarations and its
host-side argument checks, and TVLoss built from the stage-1 configs' dict."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _tv_ref as T

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tv_loss.npz")


def _golden_cases():
    z = np.load(GOLDEN)
    return [(z[f"x_{k}"], float(z[f"power_{k}"]), float(z[f"weight_{k}"]), z[f"means_{k}"], float(z[f"value_{k}"]), z[f"grad_{k}"])
            for k in range(int(z["n_cases"]))]


def test_restatement_reproduces_the_reference_values_and_gradients():
    for k, (x, p, weight, means, value, grad) in enumerate(_golden_cases()):
        got = T.slice_means_ref(x, p)
        assert np.allclose(got, means, rtol=1e-12, atol=0), k
        assert abs(got.mean() * weight - value) <= 1e-12 * max(abs(value), 1e-300), k
        g = np.full(means.shape, weight / means.size)                  # d value / d slice_mean under the 'mean' reduction
        ref, _ = T.grad_ref(x, p, g)
        assert np.allclose(ref, grad, rtol=1e-10, atol=1e-300), (k, float(np.abs(ref - grad).max()))
    flat = [c for c in _golden_cases() if c[0].shape[-2:] == (5, 5)][0]
    assert (flat[5][0, 0] == 0).all() and (flat[5][0, 2] == 0).all()    # constant slices: zero gradient, not NaN


def _inputs():
    g = np.random.default_rng(7)
    out = [g.standard_normal((3, 2, 16, 16)).astype(np.float32), g.standard_normal((4, 7, 13)).astype(np.float32),
           g.standard_normal((2, 1, 17)).astype(np.float32), g.standard_normal((2, 17, 1)).astype(np.float32),
           (g.standard_normal((2, 9, 12)) * 1e3).astype(np.float32), (g.standard_normal((2, 9, 12)) * 1e-3).astype(np.float32),
           (g.integers(-2, 3, (2, 4, 3)).astype(np.float32) * 0.5).repeat(4, axis=-2).repeat(4, axis=-1)]
    return out


@pytest.mark.parametrize("p", [1.0, 1.5, 2.0, 3.0])
def test_fp32_emulation_meets_the_bounds(p):
    g = np.random.default_rng(int(p * 10))
    for x in _inputs():
        up = g.uniform(0.5, 2.0, x.shape[:-2]).astype(np.float32)
        means, grad = T.emulate_f32(x, p, up)
        assert T.mean_excess(means, x, p) <= 1, (x.shape, T.mean_excess(means, x, p))
        assert T.grad_excess(grad, x, p, up) <= 1, (x.shape, T.grad_excess(grad, x, p, up))


def test_flat_planes_give_exact_zeros():
    x = np.full((2, 8, 8), 0.3, np.float32)
    x[1, 4:, :] = -0.7
    means, grad = T.emulate_f32(x, 1.5, np.ones(2, np.float32))
    ref, mag = T.grad_ref(x, 1.5, np.ones(2))
    assert means[0] == 0 and grad[0].max() == 0 and grad[0].min() == 0
    assert np.all(grad[1][mag[1] == 0] == 0) and np.isfinite(grad).all()


@pytest.mark.parametrize("variant", ["wrap", "drop_left", "hw_minus_1"])
def test_wrong_variants_break_the_bounds(variant):
    x = np.random.default_rng(3).standard_normal((2, 3, 128, 128)).astype(np.float32)
    up = np.ones(x.shape[:-2], np.float32)
    means, grad = T.emulate_f32(x, 1.5, up, **{variant: True})
    excess = max(T.mean_excess(means, x, 1.5), T.grad_excess(grad, x, 1.5, up))
    assert excess > 10, (variant, excess)


def test_fp32_accumulation_over_a_512_slice_breaks_the_mean_bound():
    x = np.random.default_rng(4).standard_normal((1, 512, 512)).astype(np.float32)
    good, _ = T.emulate_f32(x, 1.5, np.ones(1, np.float32))
    bad, _ = T.emulate_f32(x, 1.5, np.ones(1, np.float32), f32_sum=True)
    assert T.mean_excess(good, x, 1.5) <= 1
    assert T.mean_excess(bad, x, 1.5) > 2, T.mean_excess(bad, x, 1.5)


def test_registry_and_abi_declarations():
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd.registry import MODULES
    from ssdnerf_amd.codes import TVLoss
    assert MODULES.get("TVLoss") is TVLoss
    for name in ("ssdnerf_tv_loss_forward", "ssdnerf_tv_loss_backward"):
        assert name in C.EXPORTS and hasattr(C.lib(), name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssdnerf_hip.h")).read()
    assert "int ssdnerf_tv_loss_forward(const float* x, uint32_t n, uint32_t h, uint32_t w, float power, float* slice_mean, void* stream);" in header
    assert ("int ssdnerf_tv_loss_backward(const float* x, const float* g, uint32_t n, uint32_t h, uint32_t w, float power, float* dx_out, "
            "void* stream);") in header
    assert C.lib().ssdnerf_abi_version() == C.ABI_VERSION == 3


def test_tv_loss_rejects_bad_arguments_host_side():
    """Rejected before any HIP call (no device needed): the pointers below are never dereferenced."""
    from ssdnerf_amd import _cabi as C
    lib = C.lib()
    fake = ctypes.c_void_p(256)

    def fwd(x, n, h, w, p):
        return lib.ssdnerf_tv_loss_forward(x, n, h, w, p, fake, None)

    def bwd(x, n, h, w, p):
        return lib.ssdnerf_tv_loss_backward(x, fake, n, h, w, p, fake, None)

    for args, cause in [((None, 2, 8, 8, 1.5), "null pointer"), ((fake, 0, 8, 8, 1.5), "n == 0"), ((fake, 2, 0, 8, 1.5), "empty slice"),
                        ((fake, 2, 8, 0, 1.5), "empty slice"), ((fake, 2, 8, 8, 0.5), "power"), ((fake, 2, 8, 8, float("nan")), "power"),
                        ((fake, 2, 8, 8, float("inf")), "power"), ((fake, 2, 1 << 16, 1 << 15, 1.0), "larger than 2^30")]:
        for call in (fwd, bwd):
            assert call(*args) == -1, (call.__name__, args)
            msg = lib.ssdnerf_last_error().decode()
            assert msg.startswith("tv_loss") and cause in msg, msg
    assert lib.ssdnerf_tv_loss_backward(fake, None, 2, 8, 8, 1.5, fake, None) == -1


def test_wrapper_rejects_inputs_before_the_library():
    from ssdnerf_amd.tv_loss import tv_slice_means
    with pytest.raises(TypeError):
        tv_slice_means(torch.zeros(2, 4, 4, dtype=torch.float64))
    for bad in (torch.zeros(2, 4, 4), torch.zeros(4), torch.zeros(0, 4, 4)):
        with pytest.raises(ValueError):
            tv_slice_means(bad)


def test_tvloss_builds_from_the_stage1_config():
    from ssdnerf_amd.registry import MODULES, build_module
    from ssdnerf_amd.codes import TVLoss
    loss = build_module(dict(type="TVLoss", power=1.5, loss_weight=1.0))
    assert isinstance(loss, TVLoss) and loss.power == 1.5 and loss.loss_weight == 1.0 and loss.dims == [-2, -1]
    for dims in ([-1, -2], (3, 4), [4, -2]):
        MODULES.build(dict(type="TVLoss", dims=dims))._check_dims(5)
    for dims in ([-3, -1], [-1], [-2, -1, 0], [2, 3]):
        with pytest.raises(ValueError):
            MODULES.build(dict(type="TVLoss", dims=dims))._check_dims(5)
    with pytest.raises(ValueError):
        TVLoss(power=0.5)
    with pytest.raises(NotImplementedError):
        loss(torch.zeros(1, 3, 2, 4, 4), weight=torch.ones(1))
    with pytest.raises(NotImplementedError):
        loss(torch.zeros(1, 3, 2, 4, 4), avg_factor=2.0)


def test_stage1_model_dict_builds():
    """paper_cfgs/stage1_cars_recons16v.py's model dict: TVLoss as reg_loss, the running mean code as a buffer, BaseNeRF's val_step"""
    from ssdnerf_amd.codes import TVLoss
    from ssdnerf_amd.models import BaseNeRF, DiffusionNeRF
    from ssdnerf_amd.registry import MODELS
    dec = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[6 * 3, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
               dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64, decoder=dec,
                          decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0), cache_size=2458, init_from_mean=True))
    assert isinstance(m.reg_loss, TVLoss) and m.reg_loss.power == 1.5
    assert "init_code" in dict(m.named_buffers()) and m.init_code.shape == (3, 6, 128, 128) and float(m.init_code.abs().max()) == 0
    assert type(m).val_step is BaseNeRF.val_step and DiffusionNeRF.val_step is not BaseNeRF.val_step
