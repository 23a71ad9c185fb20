"""LPIPS without a GPU: the float64 restatement against its own fp32 form, the weight loader, the model's state dict, the tap kernel's checker
against right and wrong evaluations, and that the end-to-end tolerance of tests/test_lpips_gpu.py can be met by the library's arithmetic."""
import pytest
import torch
import torch.nn.functional as F

from _lpips_ref import (check_lpips_layer, lpips_ref, make_pairs, make_tap_input, rel_err)


@pytest.fixture(scope="module")
def sd():
    from ssdnerf_amd import synthetic as S
    return S.make_lpips_params(1)


def test_restatement_fp32_agrees_with_fp64(sd):
    a, b = make_pairs(64, 96, seed=3)
    r64 = lpips_ref(a, b, sd, torch.float64)
    r32 = lpips_ref(a, b, sd, torch.float32)
    assert r64.shape == (5,) and bool((r64 > 0).all())
    err = rel_err(r32, r64)
    print("fp32 vs fp64 restatement, relative:", err.tolist(), "values:", r64.tolist())
    assert float(err.max()) <= 1e-6


def test_synthetic_params_follow_the_recipe(sd):
    from ssdnerf_amd import lpips as L, synthetic as S
    assert len(sd) == 2 * 13 + 5
    again = S.make_lpips_params(1)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    for idx, (cin, cout) in zip(L.FEATURE_IDX, L.CHANNELS):
        w, b = sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"]
        assert w.shape == (cout, cin, 3, 3) and b.shape == (cout,)
        assert float(w.var()) == pytest.approx(2 / (9 * cin), rel=0.2) and -0.1 <= float(b.min()) and float(b.max()) <= 0.1
    for k, c in enumerate(L.TAP_CHANNELS):
        w = sd[f"lin{k}.model.1.weight"]
        assert w.shape == (1, c, 1, 1) and 0 <= float(w.min()) and float(w.max()) <= 2 / c
    assert L.flops_per_image(128, 128) == pytest.approx(10.0e9, rel=0.01)


def _as_lpips_package(sd):
    """the same tensors under the names of ``lpips.LPIPS(net='vgg').state_dict()``: the trunk in five slices that keep the ``features`` index, every lin
    layer registered twice, and the scaling layer's buffers"""
    from ssdnerf_amd.lpips import FEATURE_IDX
    slice_of = {0: 1, 2: 1, 5: 2, 7: 2, 10: 3, 12: 3, 14: 3, 17: 4, 19: 4, 21: 4, 24: 5, 26: 5, 28: 5}
    out = {"scaling_layer.shift": torch.tensor([-.030, -.088, -.188])[None, :, None, None], "scaling_layer.scale": torch.tensor([.458, .448, .450])[None, :, None, None]}
    for idx in FEATURE_IDX:
        for kind in ("weight", "bias"):
            out[f"net.slice{slice_of[idx]}.{idx}.{kind}"] = sd[f"features.{idx}.{kind}"]
    for k in range(5):
        out[f"lin{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
        out[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"]
    return out


def _same_net(a, b):
    return (all(torch.equal(x, y) for x, y in zip(a._weights, b._weights)) and all(torch.equal(x, y) for x, y in zip(a._biases, b._biases))
            and all(torch.equal(x, y) for x, y in zip(a._lins, b._lins)))


def test_loader_takes_both_key_styles(sd, tmp_path):
    from ssdnerf_amd.lpips import CHANNELS, LPIPSVGG
    tv = LPIPSVGG.from_state_dict(sd)
    assert tv._weights[0].shape == (64, 8, 3, 3) and torch.equal(tv._weights[0][:, :3], sd["features.0.weight"]) and not bool(tv._weights[0][:, 3:].any())
    assert [tuple(w.shape) for w in tv._weights[1:]] == [(co, ci, 3, 3) for ci, co in CHANNELS[1:]]
    assert [l.shape for l in tv._lins] == [(64,), (128,), (256,), (512,), (512,)]
    assert _same_net(tv, LPIPSVGG.from_state_dict(_as_lpips_package(sd)))
    prefixed = {("module.vgg." + k if k.startswith("features") else k.replace("lin", "lins.", 1).replace(".model.1", "")): v for k, v in sd.items()}
    flat = {k: (v.reshape(-1) if k.startswith("lins.") else v) for k, v in prefixed.items()}
    assert _same_net(tv, LPIPSVGG.from_state_dict(flat))
    torch.save(dict(state_dict=_as_lpips_package(sd)), tmp_path / "lpips_vgg.pth")
    assert _same_net(tv, LPIPSVGG.load(str(tmp_path / "lpips_vgg.pth")))


def test_loader_passes_over_the_classifier_of_a_full_torchvision_dict(sd):
    """``torchvision.models.vgg16().state_dict()`` also holds ``classifier.0|3|6.weight|bias``, and 0 is a trunk index: only ``features`` / ``slice<k>`` (or
    a bare index, the dict of ``vgg16().features`` itself) name trunk tensors"""
    from ssdnerf_amd.lpips import LPIPSVGG
    tv = LPIPSVGG.from_state_dict(sd)
    full = dict(sd)
    for idx, (cout, cin) in zip((0, 3, 6), ((4096, 25088), (4096, 4096), (1000, 4096))):          # the real shapes, without their memory
        full[f"classifier.{idx}.weight"] = torch.ones(1, 1).expand(cout, cin)
        full[f"classifier.{idx}.bias"] = torch.ones(1).expand(cout)
    assert _same_net(tv, LPIPSVGG.from_state_dict(full))
    assert _same_net(tv, LPIPSVGG.from_state_dict({"module." + k: v for k, v in full.items()}))
    # a classifier-like module under another name whose shapes would even fit is not taken for the trunk either
    decoy = dict(full)
    decoy["head.0.weight"], decoy["head.0.bias"] = torch.zeros(64, 3, 3, 3), torch.zeros(64)
    assert _same_net(tv, LPIPSVGG.from_state_dict(decoy))
    bare = {(k[len("features."):] if k.startswith("features.") else k): v for k, v in sd.items()}
    assert "0.weight" in bare and _same_net(tv, LPIPSVGG.from_state_dict(bare))
    with pytest.raises(KeyError, match=r"features\.0\.weight"):                                     # and the classifier cannot stand in for a missing trunk tensor
        LPIPSVGG.from_state_dict({k: v for k, v in full.items() if k != "features.0.weight"})


def test_loader_rejects_missing_and_misshaped_tensors_by_name(sd):
    from ssdnerf_amd.lpips import LPIPSVGG
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        LPIPSVGG.from_state_dict({k: v for k, v in sd.items() if k != "features.17.bias"})
    with pytest.raises(KeyError, match="lin3"):
        LPIPSVGG.from_state_dict({k: v for k, v in sd.items() if not k.startswith("lin3")})
    bad = dict(sd)
    bad["features.5.weight"] = sd["features.5.weight"][:, :32]
    with pytest.raises(ValueError, match=r"features\.5\.weight"):
        LPIPSVGG.from_state_dict(bad)
    bad = _as_lpips_package(sd)
    bad["net.slice4.19.bias"] = torch.zeros(256)
    with pytest.raises(ValueError, match=r"net\.slice4\.19\.bias"):
        LPIPSVGG.from_state_dict(bad)
    bad = dict(sd)
    bad["lin1.model.1.weight"] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError, match=r"lin1\.model\.1\.weight"):
        LPIPSVGG.from_state_dict(bad)
    bad = _as_lpips_package(sd)
    bad["lins.2.model.1.weight"] = bad["lins.2.model.1.weight"] + 1
    with pytest.raises(ValueError, match=r"lins\.2\.model\.1\.weight"):
        LPIPSVGG.from_state_dict(bad)


def test_model_state_dict_holds_no_lpips_tensor(sd):
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd.lpips import LPIPSVGG
    from ssdnerf_amd.registry import MODELS
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
                          decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3],
                                       use_dir_enc=True, dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001,
                                       max_steps=256),
                          decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss")))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.use_lpips_metric and m._lpips_net() is None
    net = LPIPSVGG.from_state_dict(sd)
    m.set_lpips(net)
    assert m._lpips_net() is net
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not any("lpips" in k or "lin" in k.split(".")[0] for k in after)
    assert all(not isinstance(c, LPIPSVGG) for c in m.modules()) and sum(p.numel() for p in m.parameters()) == sum(
        v.numel() for k, v in before.items() if k in dict(m.named_parameters()))
    m.load_state_dict(before)                                              # strict: a state dict saved without a net loads into a model with one
    m.use_lpips_metric = False
    assert m._lpips_net() is None
    m.use_lpips_metric = True
    m.set_lpips(None)
    assert m._lpips_net() is None


# ---------------------------------------------------------------------------------------------- the tap kernel's checker
def _tap_fp32(x_raw, w, n, variant="right"):
    """step 3 of one tap in fp32 torch ops from the raw convolution output (2n, C, H, W), and the wrong forms the checker must reject"""
    x = x_raw.float()
    f = x if variant == "no_relu" else F.relu(x)
    if variant == "short_last_row" and f.shape[2] % 2 == 1:
        f = f[:, :, :-1]
    eps = 0.0 if variant == "no_eps" else 1e-10
    w = torch.ones_like(w) if variant == "unit_w" else w.float()
    w = w[None, :, None, None]
    fp, ft = f[:n], f[n:]
    if variant == "normalise_after":
        e = fp - ft
        d = (e / (e.square().sum(1, keepdim=True).sqrt() + eps)).square() * w
    else:
        d = (fp / (fp.square().sum(1, keepdim=True).sqrt() + eps) - ft / (ft.square().sum(1, keepdim=True).sqrt() + eps)).square() * w
    d = d.sum(1)
    return d.sum((1, 2)) if variant == "sum" else d.mean((1, 2))


@pytest.mark.parametrize("tap,H,W", [(0, 17, 12), (1, 9, 9), (2, 6, 7), (3, 5, 4), (4, 7, 3)])
def test_tap_checker_accepts_fp32_and_rejects_wrong_forms(sd, tap, H, W):
    """on the library's tap widths and the lin weights the loader hands the kernel"""
    from ssdnerf_amd.lpips import LPIPSVGG, TAP_CHANNELS
    n, C = 3, TAP_CHANNELS[tap]
    x = make_tap_input(n, C, H, W, seed=C + H)
    assert bool((F.relu(x).sum(1) == 0).any()), "the input must hold all-zero pixels"
    w = LPIPSVGG.from_state_dict(sd)._lins[tap]
    assert w.shape == (C,) and torch.equal(w, sd[f"lin{tap}.model.1.weight"].reshape(C))
    bad, worst = check_lpips_layer(_tap_fp32(x, w, n), x, w, n)
    print(f"fp32 evaluation, C = {C}: worst error / bound = {worst:.3f}")
    assert bad == 0 and worst < 1
    acc = torch.rand(n) * 0.05
    bad, worst = check_lpips_layer(acc + _tap_fp32(x, w, n), x, w, n, acc_in=acc)
    assert bad == 0, worst
    assert check_lpips_layer(_tap_fp32(x, w, n), x, w, n, acc_in=acc)[0] == n          # a kernel that overwrites acc instead of adding to it
    for variant in ("normalise_after", "unit_w", "sum", "no_relu", "short_last_row", "no_eps"):
        if variant == "short_last_row" and H % 2 == 0:
            continue
        bad, worst = check_lpips_layer(_tap_fp32(x, w, n, variant), x, w, n)
        assert bad > 0, (variant, worst)
    # an error of one part in 10^4 of the value -- half-precision features, say -- is outside as well
    value = _tap_fp32(x, w, n).double()
    assert check_lpips_layer(value * (1 + 1e-4), x, w, n)[0] == n


# ---------------------------------------------------------------------------------------------- the end-to-end tolerance can be met
def test_end_to_end_tolerance_is_satisfiable(sd):
    """tests/test_lpips_gpu.py holds LPIPSVGG to the accuracy of the reference's own default arithmetic (TF32 convolutions).  On the same inputs (64 x 64) the
    library's bf16 x 2 products, emulated, stay below that, and plain bf16 does not."""
    a, b = make_pairs(64, 64)
    exact = lpips_ref(a, b, sd)
    tol = float(rel_err(lpips_ref(a, b, sd, mode="tf32"), exact).max())
    x2 = float(rel_err(lpips_ref(a, b, sd, mode="bf16x2"), exact).max())
    bf = float(rel_err(lpips_ref(a, b, sd, mode="bf16"), exact).max())
    print(f"worst relative error over the pairs: tf32 {tol:.2e}  bf16x2 {x2:.2e}  bf16 {bf:.2e}; values {exact.tolist()}")
    assert 0 < x2 < tol < bf
    assert float(exact.min()) > 1e-6 and float(exact.max()) < 0.1        # small scores: only a relative tolerance says anything
