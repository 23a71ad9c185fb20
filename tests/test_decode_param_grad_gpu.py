"""``ssdnerf_point_decode_backward_params`` (csrc/decode_bwd_params.hip) and ``TriPlaneDecoder(param_grad='fused')`` against the float64 reference and the derived bounds
of tests/_decode_param_grad_ref.py, on the seeded families tests/test_decode_param_grad_cpu.py proves the bounds on.
  * the C ABI, every family, ``max_blocks`` 0 (one block per 256-sample group) and 2 (two blocks loop over up to twelve groups): every parameter element inside its
    bound, unreached elements (the padding column) exactly 0; two calls give the same bits; no samples, or no upstream gradient, give zeros; argument errors return
    their codes and write nothing;
  * through Python: ``point_decode`` leaves in the eight ``.grad`` tensors what the reference says (unpacking, the transposed Wc), ``code.grad`` meets the end-to-end
    bounds of tests/_decode_grad_ref.py, a frozen parameter gets no gradient, without gradients or with ``param_grad='eager'`` the new entry point is not called, and
    a frozen decoder whose weights change in place before the backward still gets the gradient of the network its forward evaluated;
  * one ``MultiSceneNeRF.train_step`` with ``param_grad='fused'`` never enters the eager decode and leaves the gradients of the eager-mode run of the same seeded step
    (cosine >= 0.999: a check of the WIRING against gross errors, not a precision claim -- precision is the bound tests' job)."""
import ctypes

import numpy as np
import pytest
import torch

import _decode_grad_ref as G
import _decode_param_grad_ref as PG

pytestmark = pytest.mark.gpu

FAMILIES = list(G.SAMPLE_FAMILIES)
MULTI_SCENE = [n for n, v in G.SAMPLE_FAMILIES.items() if len(v[3]) > 1]
SYMBOL = "ssdnerf_point_decode_backward_params"


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_params(c, max_blocks, g_sigma=None, g_rgb=None, total=None):
    """one ``ssdnerf_point_decode_backward_params`` on a workspace of the test's own (0xff first: a record the kernels do not write reads as NaN): [N_PARAMS] numpy"""
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd.decoders import pack_triplanes
    total = len(c.xyz) if total is None else total
    planes = pack_triplanes(cu(c.code), torch.float16 if c.fp16 else torch.float32)
    need = int(C.lib().ssdnerf_point_decode_backward_params_workspace(C.u32(c.S), C.u32(total), C.u32(max_blocks)))
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device="cuda")
    grad = torch.full((PG.N_PARAMS,), float("nan"), dtype=torch.float32, device="cuda")
    offsets = c.offsets.astype(np.int32) if total else np.zeros(c.S + 1, np.int32)
    gs, grgb = cu(c.g_sigma if g_sigma is None else g_sigma), cu(c.g_rgb if g_rgb is None else g_rgb)
    P, xyz, dirs, offsets = cu(c.P.astype(np.float32)), cu(c.xyz), cu(c.dirs), cu(offsets)
    C.check(C.lib().ssdnerf_point_decode_backward_params(
        C.ptr(planes), C.dtype_code(planes), C.u32(c.S), C.u32(c.H), C.u32(c.W), C.ptr(P), C.ptr(xyz), C.ptr(dirs), C.ptr(offsets), C.u32(total), C.f32(c.sat),
        C.ptr(gs), C.ptr(grgb), C.ptr(grad), C.u32(max_blocks), C.ptr(ws), ctypes.c_size_t(need), C.stream()), SYMBOL)
    torch.cuda.synchronize()
    return grad.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.mark.parametrize("max_blocks", [0, 2])
@pytest.mark.parametrize("name", FAMILIES)
def test_kernel_meets_the_bound_of_every_parameter_element(name, max_blocks):
    r = PG.reference(name)
    got = run_params(G.sample_case(name), max_blocks)
    bad, worst = PG.check_le(got, r.ref, r.bound)
    print(name, "max_blocks", max_blocks, "live", r.n_live, "worst ratio", round(worst, 4))
    assert bad == 0, (bad, worst)
    assert (r.bound == 0).sum() == 64 and not got[r.bound == 0].any()        # the padding column rec[:, 23], exactly 0


@pytest.mark.parametrize("max_blocks", [0, 2])
def test_two_consecutive_calls_give_the_same_bits(max_blocks):
    c = G.sample_case("square-fp16-straddle")
    a, b = run_params(c, max_blocks), run_params(c, max_blocks)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_no_samples_and_no_upstream_gradient_give_zeros():
    c = G.sample_case("ragged-fp32-aligned")
    assert not run_params(c, 0, total=0).view(np.uint32).any()
    for max_blocks in (0, 2):
        got = run_params(c, max_blocks, g_sigma=np.zeros_like(c.g_sigma), g_rgb=np.zeros_like(c.g_rgb))
        assert not got.any() and np.isfinite(got).all()


def test_argument_errors_return_their_codes_and_write_nothing():
    from ssdnerf_amd import _cabi as C
    lib = C.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    grad = torch.full((PG.N_PARAMS,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.zeros(PG.N_PARAMS * 4, dtype=torch.uint8, device="cuda")

    def call(planes=buf, dtype=0, params=buf, xyz=buf, dirs=buf, offsets=buf, grgb=buf, out=grad, work=ws, work_bytes=None):
        return lib.ssdnerf_point_decode_backward_params(C.ptr(planes), dtype, C.u32(1), C.u32(2), C.u32(2), C.ptr(params), C.ptr(xyz), C.ptr(dirs), C.ptr(offsets),
                                                        C.u32(5), C.f32(0.001), C.ptr(buf), C.ptr(grgb), C.ptr(out), C.u32(0), C.ptr(work),
                                                        ctypes.c_size_t(ws.numel() if work_bytes is None else work_bytes), C.stream())
    for kw in (dict(planes=None), dict(params=None), dict(xyz=None), dict(dirs=None), dict(offsets=None), dict(grgb=None), dict(out=None), dict(work=None)):
        assert call(**kw) == -1, kw                                          # SSDNERF_E_INVALID
        assert b"null" in lib.ssdnerf_last_error()
    assert call(dtype=2) == -1 and b"dtype" in lib.ssdnerf_last_error()
    assert call(work_bytes=ws.numel() - 1) == -3 and b"workspace" in lib.ssdnerf_last_error()       # SSDNERF_E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(grad).all()) and not bool(ws.any())             # nothing was launched


# ------------------------------------------------------------------------------------------------ through Python
def make_decoder(c, param_grad):
    from ssdnerf_amd.decoders import TriPlaneDecoder
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256, param_grad=param_grad)
    dec.load_state_dict(c.sd, strict=False)
    dec = dec.cuda().train(True)
    dec.plane_dtype = torch.float16 if c.fp16 else torch.float32
    assert dec.sigmoid_saturation == c.sat and np.array_equal(dec.packed_params().cpu().numpy().view(np.uint32), c.P.view(np.uint32))
    return dec


def decode_and_backward(dec, c, code, between=None):
    cut = [(int(c.offsets[s]), int(c.offsets[s + 1])) for s in range(c.S)]
    sig, rgb, num = dec.point_decode([cu(c.xyz[a:b]) for a, b in cut], [cu(c.dirs[a:b]) for a, b in cut], code)
    assert num == list(c.sizes)
    if between is not None:
        between()
    if sig.requires_grad:
        torch.autograd.backward((sig, rgb), (cu(c.g_sigma), cu(c.g_rgb)))
    return cut


@pytest.fixture
def calls(monkeypatch):
    """counts the calls of the new entry point (the library object's attribute is wrapped)"""
    from ssdnerf_amd import _cabi as C
    real, n = getattr(C.lib(), SYMBOL), []

    def spy(*args):
        n.append(1)
        return real(*args)
    monkeypatch.setattr(C.lib(), SYMBOL, spy)
    return n


def check_code_gradient(name, c, cut, got):
    """``got`` (S,3,6,H,W) numpy under the end-to-end bounds of the code gradient around the float64 reference of the family's own weights"""
    from ssdnerf_amd import _cabi as C
    _, gf, B, _ = G.sample_reference(name, False, False)
    lay = (ctypes.c_uint64 * 6)()
    C.lib().ssdnerf_point_decode_backward_layout(C.u32(c.S), C.u32(len(c.xyz)), C.u32(c.H), C.u32(c.W), lay)
    K = int(lay[5])                                                          # the split count of the code gradient's reduction
    for s, (a, b) in enumerate(cut):
        e_ref, e_bnd = G.scatter_e2e_ref(c.xyz[a:b], gf[a:b], B[a:b], c.H, c.W, K)
        bad, worst = G.check_le(got[s], e_ref, e_bnd)
        assert bad == 0, (name, s, bad, worst)


@pytest.mark.parametrize("name", MULTI_SCENE)
def test_point_decode_leaves_the_reference_gradients_in_parameters_and_code(name, calls):
    c, r = G.sample_case(name), PG.reference(name)
    dec = make_decoder(c, "fused")
    code = cu(c.code).requires_grad_(True)
    cut = decode_and_backward(dec, c, code)
    assert len(calls) == 1
    ref, bnd = PG.unpack(r.ref), PG.unpack(r.bound)
    params = dict(dec.named_parameters())
    for k in PG.NAMES:
        got = params[k].grad
        assert got is not None and got.dtype == torch.float32 and tuple(got.shape) == ref[k].shape, k
        bad, worst = PG.check_le(got.cpu().numpy(), np.ascontiguousarray(ref[k]), np.ascontiguousarray(bnd[k]))
        assert bad == 0, (name, k, bad, worst)
    # the code's gradient: the launches of ssdnerf_point_decode_backward, under that gradient's own end-to-end bounds
    check_code_gradient(name, c, cut, code.grad.cpu().numpy())


def test_a_frozen_parameter_gets_no_gradient_and_a_frozen_code_none(calls):
    c, r = G.sample_case("ragged-fp32-aligned"), PG.reference("ragged-fp32-aligned")
    dec = make_decoder(c, "fused")
    frozen = ("dir_net.0.weight", "color_net.0.bias")
    params = dict(dec.named_parameters())
    for k in frozen:
        params[k].requires_grad_(False)
    code = cu(c.code)
    decode_and_backward(dec, c, code)
    assert len(calls) == 1 and code.grad is None
    ref, bnd = PG.unpack(r.ref), PG.unpack(r.bound)
    for k in PG.NAMES:
        if k in frozen:
            assert params[k].grad is None, k
        else:
            assert PG.check_le(params[k].grad.cpu().numpy(), np.ascontiguousarray(ref[k]), np.ascontiguousarray(bnd[k]))[0] == 0, k


def test_a_frozen_decoder_gets_the_gradient_of_the_weights_its_forward_read(calls):
    """the backward reads the packed block the forward read: a weight doubled in place between the two does not reach the code's gradient, which stays under the
    end-to-end bounds around the reference of the ORIGINAL weights (re-packing at backward time would differentiate the doubled network)"""
    name = "ragged-fp32-aligned"
    c = G.sample_case(name)
    dec = make_decoder(c, "eager").requires_grad_(False)
    code = cu(c.code).requires_grad_(True)

    def double():
        with torch.no_grad():
            dec.base_net[0].weight.mul_(2)
    cut = decode_and_backward(dec, c, code, between=double)
    assert calls == [] and not np.array_equal(dec.packed_params().cpu().numpy(), c.P)        # (the change is real: the next forward packs the doubled weights)
    check_code_gradient(name, c, cut, code.grad.cpu().numpy())


def test_without_gradients_and_in_eager_mode_the_call_sequence_is_the_present_one(calls, monkeypatch):
    c = G.sample_case("ragged-fp32-aligned")
    dec = make_decoder(c, "fused")
    entered = []
    eager = dec.point_decode_eager
    monkeypatch.setattr(dec, "point_decode_eager", lambda *a, **k: (entered.append(1), eager(*a, **k))[1])
    with torch.no_grad():                                                    # no gradient: the fused forward alone
        decode_and_backward(dec, c, cu(c.code).requires_grad_(True))
    assert calls == [] and entered == []
    dec.requires_grad_(False)                                                # a frozen decoder: the code-gradient launches alone, as before
    code = cu(c.code).requires_grad_(True)
    decode_and_backward(dec, c, code)
    assert calls == [] and entered == [] and code.grad is not None
    dec = make_decoder(c, "eager")                                           # the default: a trainable decoder decodes eagerly
    entered2 = []
    eager2 = dec.point_decode_eager
    monkeypatch.setattr(dec, "point_decode_eager", lambda *a, **k: (entered2.append(1), eager2(*a, **k))[1])
    decode_and_backward(dec, c, cu(c.code).requires_grad_(True))
    assert calls == [] and entered2 == [1] and dec.base_net[0].weight.grad is not None
    dec = make_decoder(c, "fused")                                           # density-only and missing directions stay eager under 'fused'
    entered3 = []
    eager3 = dec.point_decode_eager
    monkeypatch.setattr(dec, "point_decode_eager", lambda *a, **k: (entered3.append(1), eager3(*a, **k))[1])
    sig, _ = dec.point_density_decode([cu(c.xyz[:256]), cu(c.xyz[256:])], cu(c.code))
    sig.sum().backward()
    assert calls == [] and entered3 == [1]


# ------------------------------------------------------------------------------------------------ one training step
DEC = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[6 * 3, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
           dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)


@pytest.fixture(scope="module")
def views():
    """(images, poses, intrinsics) of two synthetic scenes, two 64 x 64 views each, rendered by the synthetic decoder"""
    from ssdnerf_amd import nerf, synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.density import get_density
    dec = TriPlaneDecoder(**{k: v for k, v in DEC.items() if k != "type"})
    dec.load_state_dict(S.make_decoder_params(), strict=False)
    dec = dec.cuda().eval()
    codes = torch.stack([S.make_triplane(s) for s in (51, 52)]).cuda()
    with torch.no_grad():
        _, bits = get_density(dec, codes, 64, density_thresh=0.1, density_step=4)
        poses = S.spiral_poses()[[30, 150]].cuda()[None].expand(2, -1, -1, -1).contiguous()
        intr = S.cars_intrinsics(64, 64).cuda()[None, None].expand(2, 2, -1).contiguous()
        image, _ = nerf.render(dec, codes, bits, 64, 64, intr, poses)
    return image.clamp(0, 1), poses, intr


def seeded_step(param_grad, views, monkeypatch):
    """the gradients one ``train_step`` leaves: ({parameter name: grad}, [code grad per scene]); shape: 2 scenes, planes 3 x 6 x 32 x 32, 256 rays, no extra steps"""
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    train_cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=0, n_inverse_rays=256, n_decoder_rays=256, loss_coef=0.1 / (64 * 64),
                     optimizer=dict(type="Adam", lr=1e-2, weight_decay=0.))
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 32, 32), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
                          decoder=dict(DEC, param_grad=param_grad), decoder_use_ema=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          cache_size=4, init_from_mean=True, train_cfg=train_cfg))
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    with torch.no_grad():           # the running mean code a trained model would hold (all zeros would render an empty grid: no gradient)
        m.init_code.copy_(torch.nn.functional.avg_pool2d(S.make_triplane(80), 4))
    m = m.cuda().train()
    assert m.decoder.param_grad == param_grad
    if param_grad == "fused":
        def never(*a, **k):
            raise AssertionError("point_decode_eager entered with param_grad='fused'")
        monkeypatch.setattr(m.decoder, "point_decode_eager", never)
    code_grads = []
    save = m.save_cache
    monkeypatch.setattr(m, "save_cache", lambda leaves, *a, **k: (code_grads.extend(l.grad.detach().clone() for l in leaves), save(leaves, *a, **k))[1])
    imgs, poses, intr = views
    data = dict(scene_id=[0, 2], scene_name=["s0", "s2"], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr)
    opt = dict(decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    torch.manual_seed(1)
    out = m.train_step(data, opt)
    assert out["num_samples"] == 2 and bool(torch.isfinite(torch.as_tensor(out["log_vars"]["loss"]).float()))
    return {k: p.grad.detach().clone() for k, p in m.decoder.named_parameters()}, code_grads


def test_train_step_with_fused_parameter_gradients_matches_the_eager_step(views, monkeypatch, calls):
    """GROSS-ERROR check of the wiring (which tensor gets which gradient, transposition, scale, sign), not a precision claim: the two modes differ by fp32 rounding
    per sample, and the bound tests above hold the kernel to its precision"""
    fused, fused_code = seeded_step("fused", views, monkeypatch)
    assert len(calls) == 1
    eager, eager_code = seeded_step("eager", views, monkeypatch)
    assert len(calls) == 1
    assert set(fused) == set(eager) == set(PG.NAMES) and len(fused_code) == len(eager_code) == 2
    for k, a, b in [(k, fused[k], eager[k]) for k in PG.NAMES] + [(f"code {s}", fused_code[s], eager_code[s]) for s in range(2)]:
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, k
        cos = float(torch.nn.functional.cosine_similarity(a.double().reshape(1, -1), b.double().reshape(1, -1)))
        print(k, "cosine", cos)
        assert cos >= 0.999, (k, cos)
