"""ExponentialMovingAverageHook on the MI355X: the kernel (csrc/ema.hip) against the numpy three-rounding restatement of tests/_ema_ref.py,
BIT FOR BIT -- single tensors at odd sizes and alignments, tables of up to 300 mixed rows in one launch, sentinels around every array -- the
host-side plan validation, the hook on decoder and UNet pairs (packed weights must notice the update), plan rebuilds, and three
``DiffusionNeRF.train_step``s each followed by the hook."""
import ctypes
import types
from copy import deepcopy

import numpy as np
import pytest
import torch

import _ema_ref as E

pytestmark = pytest.mark.gpu

CHUNK = 4096                                            # elements per block (csrc/ema.hip, EMA_CHUNK)
SENT = 12345.0
M_ITER0, M_FINAL = 9.5367431640625e-07, 0.9972312513520695         # the configs' rampup momentum at iteration 0 and from iteration 4999 on


def _carve(values, offset):
    """a contiguous fp32 GPU view holding ``values`` at ``offset`` elements past a 16-byte boundary (offset 1: 4-byte aligned only), between
    sentinel elements; returns (view, whole buffer, index of the view's first element)"""
    n, front = len(values), 4 + offset
    buf = torch.full((front + n + 7,), SENT, device="cuda")
    view = buf[front:front + n]
    view.copy_(torch.from_numpy(values))
    assert view.data_ptr() % 16 == (4 * offset) % 16 and view.is_contiguous()
    return view, buf, front


class _Holder(torch.nn.Module):
    """tensors carved out of larger buffers as the entries of a module: kind 'train' / 'frozen' (parameters) or 'buffer'"""

    def __init__(self, views, kinds):
        super().__init__()
        for k, (v, kind) in enumerate(zip(views, kinds)):
            if kind == "buffer":
                self.register_buffer(f"t{k}", v)
            else:
                self.register_parameter(f"t{k}", torch.nn.Parameter(v, requires_grad=kind == "train"))
            assert getattr(self, f"t{k}").data_ptr() == v.data_ptr()


def _pair_model(rows):
    """rows: (numel, src offset, dst offset, kind, seed) -> (model with .net / .net_ema over carved tensors, per-row bookkeeping)"""
    held, src_views, dst_views = [], [], []
    for numel, so, do, kind, seed in rows:
        ema, src = E.make_values(numel, seed)
        sv, sbuf, sfront = _carve(src, so)
        dv, dbuf, dfront = _carve(ema, do)
        src_views.append(sv)
        dst_views.append(dv)
        held.append(dict(ema=ema, src=src, sbuf=sbuf, sfront=sfront, dbuf=dbuf, dfront=dfront, kind=kind, numel=numel))
    m = torch.nn.Module()
    m.net = _Holder(src_views, [r[3] for r in rows])
    m.net_ema = _Holder(dst_views, [r[3] for r in rows])
    return m, held


def _assert_rows(held, momentum, nontrainable, what):
    torch.cuda.synchronize()
    for k, h in enumerate(held):
        m = momentum if h["kind"] == "train" else nontrainable
        want = E.update32(h["ema"], h["src"], m)
        dbuf, sbuf = h["dbuf"].cpu().numpy(), h["sbuf"].cpu().numpy()
        got = dbuf[h["dfront"]:h["dfront"] + h["numel"]]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (what, k, "NaN positions")
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), (what, k, int((got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan]).sum()))
        # sentinels on both sides of both arrays, and the source bit for bit
        assert np.all(dbuf[:h["dfront"]] == SENT) and np.all(dbuf[h["dfront"] + h["numel"]:] == SENT), (what, k, "dst sentinels")
        assert np.all(sbuf[:h["sfront"]] == SENT) and np.all(sbuf[h["sfront"] + h["numel"]:] == SENT), (what, k, "src sentinels")
        assert np.array_equal(sbuf[h["sfront"]:h["sfront"] + h["numel"]].view(np.uint32), h["src"].view(np.uint32)), (what, k, "src changed")


SINGLE = [(n, 0, 0) for n in (1, 3, 4, 5, 1023, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)] + [(5, 1, 1), (4099, 1, 1), (4099, 0, 1), (4099, 1, 0), (5, 2, 3),
                                                                                                (3 * CHUNK + 7, 3, 1)]


@pytest.mark.parametrize("numel,src_offset,dst_offset", SINGLE)
def test_single_tensor_is_bit_identical_to_the_restatement(numel, src_offset, dst_offset):
    from ssdnerf_amd import ema
    for j, m in enumerate((0.0, M_ITER0, M_FINAL, 1.0)):
        for kind in ("train", "buffer"):
            model, held = _pair_model([(numel, src_offset, dst_offset, kind, 1000 * j + numel)])
            hook = ema.ExponentialMovingAverageHook("net_ema", interval=1, interp_cfg=dict(momentum=m if kind == "train" else 0.5,
                                                                                            momentum_nontrainable=0.5 if kind == "train" else m))
            count, eager = ema.launches, ema.eager_tensors
            hook.update(model, 0)
            assert ema.launches == count + 1 and ema.eager_tensors == eager
            _assert_rows(held, m if kind == "train" else 0.5, 0.5 if kind == "train" else m, f"numel {numel} offsets {src_offset}/{dst_offset} m {m} {kind}")


@pytest.mark.parametrize("T", [1, 2, 33, 300])
def test_table_of_mixed_rows_in_one_launch(T):
    from ssdnerf_amd import ema
    sizes = [1, 3 * CHUNK + 7, 1, 5, CHUNK, 1, CHUNK + 1, 4099, 64, 2 * CHUNK - 1, 7, 1023]
    kinds = ["train", "buffer", "train", "frozen"]
    rows = [(sizes[k % len(sizes)] + k // len(sizes), k % 2, (k // 2) % 2, kinds[k % 4] if T > 1 else "train", 50 + k) for k in range(T)]
    model, held = _pair_model(rows)
    hook = ema.ExponentialMovingAverageHook("net_ema", interval=1, interp_cfg=dict(momentum=M_FINAL, momentum_nontrainable=0.25))
    count, builds, eager = ema.launches, ema.plan_builds, ema.eager_tensors
    hook.update(model, 0)
    assert (ema.launches, ema.plan_builds, ema.eager_tensors) == (count + 1, builds + 1, eager)           # exactly one library call
    _assert_rows(held, M_FINAL, 0.25, f"T {T}")
    # a second update: from the first one's result, the plan reused
    for h in held:
        h["ema"] = h["dbuf"].cpu().numpy()[h["dfront"]:h["dfront"] + h["numel"]].copy()
    hook.update(model, 1)
    assert (ema.launches, ema.plan_builds) == (count + 2, builds + 1)
    _assert_rows(held, M_FINAL, 0.25, f"T {T}, second update")


def test_host_validation_refuses_bad_rows_and_launches_nothing():
    from ssdnerf_amd import _cabi as C, ema
    lib = C.lib()
    src, dst = torch.ones(64, device="cuda"), torch.full((64,), 2.0, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()

    def build(rows):
        tab = (C.EmaRow * len(rows))()
        for e, (a, b, n) in zip(tab, rows):
            e.src, e.dst, e.numel, e.trainable = a, b, n, 1
        return lib.ssdnerf_ema_plan_build(tab, len(rows), ctypes.byref(ctypes.c_uint32(0)))

    assert build([(s, d, 64)]) == 0
    for rows, cause in [([(0, d, 64)], "null pointer"), ([(s, 0, 64)], "null pointer"), ([(s + 2, d, 8)], "4-byte aligned"), ([(s, d + 1, 8)], "4-byte aligned"),
                        ([(s, d, 0)], "numel == 0"), ([(s, d, 16), (s + 64, d, 16)], "appears twice"), ([(s, d, 16), (s + 64, d + 32, 16)], "overlaps dst"),
                        ([(s, s + 32, 16)], "overlaps src"), ([(s, d, 16), (d + 32, s + 128, 16)], "overlaps src")]:
        with pytest.raises(RuntimeError, match=cause):
            C.check(build(rows), "ema_plan_build")
    # through the hook: an EMA entry that IS its source entry is refused before anything is launched
    model = torch.nn.Module()
    model.net = torch.nn.Linear(8, 8).cuda()
    model.net_ema = deepcopy(model.net)
    model.net_ema.weight = model.net.weight
    count = ema.launches
    with pytest.raises(RuntimeError, match="ema_plan_build"):
        ema.ExponentialMovingAverageHook("net_ema", interval=1).update(model, 0)
    torch.cuda.synchronize()
    assert ema.launches == count and torch.all(src == 1.0) and torch.all(dst == 2.0)


# ---------------------------------------------------------------------------------------------- the hook on modules
def _perturb(module, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.add_((torch.randn(p.shape, generator=g) * scale).to(p.device, p.dtype))
        for b in module.buffers():
            if b.is_floating_point():
                b.add_((torch.randn(b.shape, generator=g) * scale).to(b.device, b.dtype))


def _step_and_check(hook, model, key, iteration, what, **ref_kw):
    """one hook update of ``model``; the EMA module's state dict against the plain-torch restatement applied to snapshots, bit for bit"""
    src, trainable = E.snapshot(getattr(model, key[:-4]))
    before, _ = E.snapshot(getattr(model, key))
    hook.after_train_iter(types.SimpleNamespace(iter=iteration, model=model))
    E.assert_state_bits_equal(getattr(model, key), E.hook_step(src, trainable, before, iteration, **ref_kw), what)
    E.assert_state_bits_equal(getattr(model, key[:-4]), src, what + " (source)")
    return src


RAMPUP = dict(momentum_policy="rampup", momentum_cfg=E.CFG_MOMENTUM)


def _decoder_model():
    import test_tv_loss_gpu as TV
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    model = torch.nn.Module()
    model.decoder = TriPlaneDecoder(**{k: v for k, v in TV.DEC.items() if k != "type"})
    model.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    model.decoder_ema = deepcopy(model.decoder)
    return model.cuda()


def test_decoder_pair_three_rampup_updates_then_frozen_is_a_copy():
    from ssdnerf_amd import ema
    model = _decoder_model()
    hook = ema.ExponentialMovingAverageHook(("decoder_ema",), interval=1, **RAMPUP)
    count, eager = ema.launches, ema.eager_tensors
    for it in range(3):
        _perturb(model.decoder, 10 + it)
        _step_and_check(hook, model, "decoder_ema", it, f"iteration {it}", **RAMPUP)
    assert ema.launches == count + 3 and ema.eager_tensors == eager                 # every entry of the decoder rode in the launch
    assert not torch.equal(model.decoder_ema.base_net[0].weight, model.decoder.base_net[0].weight)     # (momentum 0.25 at iteration 2: not a copy)
    model.decoder.requires_grad_(False)
    _perturb(model.decoder, 20)
    src = _step_and_check(hook, model, "decoder_ema", 3, "frozen source", **RAMPUP)
    E.assert_state_bits_equal(model.decoder_ema, src, "frozen source: a copy")


def _decode_inputs():
    from ssdnerf_amd import synthetic as S
    g = torch.Generator().manual_seed(5)
    xyz = (torch.rand(1, 4099, 3, generator=g) * 1.6 - 0.8).cuda()
    dirs = torch.nn.functional.normalize(torch.randn(1, 4099, 3, generator=g), dim=-1).cuda()
    return xyz, dirs, S.make_triplane(41).cuda()[None]


def test_decoder_emas_fused_decode_sees_the_update():
    """the packed parameter block is keyed on the weights' version counters; the kernel writes through raw pointers"""
    import test_tv_loss_gpu as TV
    from ssdnerf_amd import ema
    from ssdnerf_amd.decoders import TriPlaneDecoder
    model = _decoder_model().eval()
    xyz, dirs, code = _decode_inputs()
    with torch.no_grad():
        sig0, rgb0, _ = model.decoder_ema.point_decode(xyz, dirs, code)
        packed0 = model.decoder_ema.packed_params().clone()
        _perturb(model.decoder, 30, scale=0.2)
        versions = [p._version for p in model.decoder_ema.parameters()]
        ema.ExponentialMovingAverageHook(("decoder_ema",), interval=1, **RAMPUP).update(model, 0)
        assert all(p._version > v for p, v in zip(model.decoder_ema.parameters(), versions))
        sig1, rgb1, _ = model.decoder_ema.point_decode(xyz, dirs, code)
        fresh = TriPlaneDecoder(**{k: v for k, v in TV.DEC.items() if k != "type"}).cuda().eval()
        fresh.load_state_dict(model.decoder_ema.state_dict())
        sig2, rgb2, _ = fresh.point_decode(xyz, dirs, code)
    assert not torch.equal(model.decoder_ema.packed_params(), packed0)
    assert torch.equal(sig1, sig2) and torch.equal(rgb1, rgb2)
    assert not torch.equal(rgb1, rgb0) and bool(torch.isfinite(rgb1).all())


def test_unet_pair_and_the_executors_packed_weights():
    """the smallest UNet tests/test_unet_fast_gpu.py runs through the inference executor.  Two evaluations of the same weights by the same
    kernels: the bound is 1e-4 of the output's scale, 20 x tighter than that file's executor-against-eager bound (2e-3) and room only for the
    order of fp32 partial sums; stale packed weights are off by the whole update (asserted to be more than 100 x the bound)."""
    import test_unet_fast_gpu as TU
    from ssdnerf_amd import ema
    model = torch.nn.Module()
    model.diffusion = TU._unet(seed=0)
    model.diffusion_ema = deepcopy(model.diffusion)
    hook = ema.ExponentialMovingAverageHook(("diffusion_ema",), interval=1, **RAMPUP)
    g = torch.Generator().manual_seed(3)
    x, t = torch.randn(2, 18, 32, 32, generator=g).cuda(), torch.tensor([999, 19]).cuda()
    model.diffusion_ema.fast_inference = True
    with torch.no_grad():
        out0 = model.diffusion_ema(x, t).clone()
    count, eager = ema.launches, ema.eager_tensors
    for it in range(2):
        _perturb(model.diffusion, 40 + it, scale=0.02)
        _step_and_check(hook, model, "diffusion_ema", it, f"iteration {it}", **RAMPUP)
    assert ema.launches == count + 2 and ema.eager_tensors == eager
    fresh = TU._unet(seed=7)
    fresh.load_state_dict(model.diffusion_ema.state_dict())
    fresh.fast_inference = True
    with torch.no_grad():
        out1 = model.diffusion_ema(x, t).clone()
        out2 = fresh(x, t)
    bound = 1e-4 * max(1.0, float(out2.abs().max()))
    err, moved = float((out1 - out2).abs().max()), float((out1 - out0).abs().max())
    print("executor after the update against a fresh network:", err, "bound:", bound, "moved by the update:", moved)
    assert err <= bound and moved > 100 * bound


def test_plan_is_rebuilt_when_the_tensors_change():
    from ssdnerf_amd import ema
    model = _decoder_model()
    hook = ema.ExponentialMovingAverageHook(("decoder_ema",), interval=1, interp_cfg=dict(momentum=M_FINAL))
    _perturb(model.decoder, 50)
    _step_and_check(hook, model, "decoder_ema", 0, "first", momentum=M_FINAL)
    # load_state_dict (copies in place here; reallocating would be noticed the same way)
    other = _decoder_model()
    _perturb(other.decoder, 51)
    model.decoder.load_state_dict(other.decoder.state_dict())
    model.decoder_ema.load_state_dict(other.decoder_ema.state_dict())
    _step_and_check(hook, model, "decoder_ema", 1, "after load_state_dict", momentum=M_FINAL)
    # one Parameter object replaced: exactly one more plan
    builds, count = ema.plan_builds, ema.launches
    old = model.decoder.base_net[0].weight
    model.decoder.base_net[0].weight = torch.nn.Parameter(old.detach().clone() + 0.125)
    _step_and_check(hook, model, "decoder_ema", 2, "after a swapped Parameter", momentum=M_FINAL)
    assert ema.plan_builds == builds + 1 and ema.launches == count + 1
    _step_and_check(hook, model, "decoder_ema", 3, "the new plan reused", momentum=M_FINAL)
    assert ema.plan_builds == builds + 1 and ema.launches == count + 2
    # .double() on one submodule: its entries go eager, the rest still take one launch
    model.decoder.dir_net.double()
    model.decoder_ema.dir_net.double()
    n_double = len(model.decoder.dir_net.state_dict())
    _perturb(model.decoder, 52)
    builds, count, eager = ema.plan_builds, ema.launches, ema.eager_tensors
    _step_and_check(hook, model, "decoder_ema", 4, "after .double()", momentum=M_FINAL)
    assert n_double > 0 and (ema.plan_builds, ema.launches, ema.eager_tensors) == (builds + 1, count + 1, eager + n_double)
    assert model.decoder_ema.dir_net[0].weight.dtype == torch.float64
    # only the source in double: the formula promotes, the copy back casts
    model.decoder_ema.dir_net.float()
    _step_and_check(hook, model, "decoder_ema", 5, "source in double, EMA in float", momentum=M_FINAL)
    # the whole pair moved to the CPU: no launch at all
    model.cpu()
    count = ema.launches
    _step_and_check(hook, model, "decoder_ema", 6, "on the CPU", momentum=M_FINAL)
    assert ema.launches == count


# ---------------------------------------------------------------------------------------------- in training
def test_three_train_steps_each_followed_by_the_hook():
    """needs no run-to-run determinism of the train step: the expected EMA state is the restatement applied to snapshots taken between
    ``train_step`` and the hook"""
    import test_rows_gpu as TR
    from ssdnerf_amd import ema, nerf, synthetic as S
    from ssdnerf_amd.density import get_density
    from ssdnerf_amd.registry import MODELS, build_hook
    train_cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=1, n_inverse_rays=2 ** 12, n_decoder_rays=2 ** 12,
                     loss_coef=0.1 / (64 * 64), optimizer=dict(type="Adam", lr=0.02))
    test_cfg = dict(img_size=(128, 128), num_timesteps=2, clip_range=[-2, 2], density_thresh=0.1)
    m = MODELS.build(dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2),
                          grid_size=64, diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                                                       denoising=TR._unet(base=32, cfg=(1, 1), att=(), groups=8),
                                                       timestep_sampler=dict(type="SNRWeightedTimeStepSampler", power=0.5),
                                                       ddpm_loss=dict(type="DDPMMSELossMod", rescale_mode="timestep_weight",
                                                                      data_info=dict(pred="v_t_pred", target="v_t"), weight_scale=4.0, scale_norm=True)),
                          decoder=TR.DEC, decoder_use_ema=True, freeze_decoder=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=4, init_scale=0.5, train_cfg=train_cfg, test_cfg=test_cfg))
    TR._randomize(m.diffusion.denoising, 3)
    m.diffusion_ema.load_state_dict(m.diffusion.state_dict())
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().train()
    dec = TR._decoder()
    codes = torch.stack([S.make_triplane(51), S.make_triplane(52)]).cuda()
    _, bits = get_density(dec, codes, 64, density_thresh=0.1, density_step=4)
    poses = S.spiral_poses()[[30, 150]].cuda()[None].expand(2, -1, -1, -1).contiguous()
    intr = S.cars_intrinsics(64, 64).cuda()[None, None].expand(2, 2, -1).contiguous()
    target, _ = nerf.render(dec, codes, bits, 64, 64, intr, poses)
    data = dict(scene_id=[0, 2], scene_name=["s0", "s2"], cond_imgs=target.clamp(0, 1), cond_poses=poses, cond_intrinsics=intr)
    opt = dict(diffusion=torch.optim.Adam(m.diffusion.parameters(), lr=1e-4), decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    hook = build_hook(dict(type="ExponentialMovingAverageHook", module_keys=("diffusion_ema", "decoder_ema"), interp_mode="lerp", interval=1, start_iter=0,
                           priority="VERY_HIGH", **RAMPUP))
    runner = types.SimpleNamespace(iter=0, model=m)
    hook.before_run(runner)
    init, _ = E.snapshot(m.diffusion_ema)
    np.random.seed(1); torch.manual_seed(1)
    count, builds, eager = ema.launches, ema.plan_builds, ema.eager_tensors
    for it in range(3):
        out = m.train_step(data, opt)
        assert bool(torch.isfinite(torch.as_tensor(out["log_vars"]["loss_ddpm_mse"]).float()).all())
        runner.iter = it
        snaps = {k: (E.snapshot(getattr(m, k[:-4])), E.snapshot(getattr(m, k))[0]) for k in hook.module_keys}
        hook.after_train_iter(runner)
        for k, ((src, trainable), before) in snaps.items():
            E.assert_state_bits_equal(getattr(m, k), E.hook_step(src, trainable, before, it, **RAMPUP), f"{k} after iteration {it}")
    assert (ema.launches, ema.plan_builds, ema.eager_tensors) == (count + 3, builds + 1, eager)        # both pairs in one plan, one launch per iteration
    assert any(not torch.equal(v, init[k]) for k, v in m.diffusion_ema.state_dict().items())
    assert not torch.equal(m.diffusion_ema.denoising.out.conv.weight, init["denoising.out.conv.weight"])
    m.eval()
    noise = torch.randn(1, 3, 6, 128, 128, generator=torch.Generator().manual_seed(2)).cuda()
    with torch.no_grad():
        code, _, bits = m.val_uncond(dict(scene_id=[0], noise=noise))
    assert code.shape == (1, 3, 6, 128, 128) and bool(torch.isfinite(code).all()) and bits.dtype == torch.uint8
