"""``k_point_decode`` (csrc/decode.hip) and the fused render pipelines (render_fused.hip, render_queue.hip, shade_mfma.hip, through
``TriPlaneDecoder.render_packed``) against the float64 reference and the per-sample / per-ray bounds of tests/_render_ref.py, on the seeded
families that tests/test_render_bounds_cpu.py proves the bounds on.  The VALU pipelines ("single", "queue") and ``point_decode`` are held to the
bound without the split term, the default MFMA pipeline to the bound with it; a decided ray's sample count must be exact and the overflow flag 0.
The built-in control runs the opt-in three-product form of the direction term once and expects it OUTSIDE the MFMA bound.  Oracle parity stays in
tests/test_render_gpu.py.

``python tests/test_render_fp64_gpu.py OUT.json`` runs every case and writes the worst error / bound ratio per output, family and pipeline, and
the control's ratios (profiles/render_bounds.json is such a run)."""
import functools
import json
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _render_ref as RR

pytestmark = pytest.mark.gpu

PIPELINES = ("single", "queue", "queue_mfma")


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_decoder(c):
    """a decoder that holds the case's state dict; the packed block the kernels read must be the one the reference upcasts"""
    from ssdnerf_amd.decoders import TriPlaneDecoder
    dec = TriPlaneDecoder(base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], dir_layers=[16, 64], max_steps=256)
    dec.load_state_dict(c.sd, strict=False)
    dec = dec.cuda().eval()
    assert dec.sigmoid_saturation == c.sat and np.array_equal(dec.packed_params().cpu().numpy().view(np.uint32), c.P.view(np.uint32))
    return dec


@functools.lru_cache(maxsize=None)
def case_decoder(family, n_rays):
    return make_decoder(RR.case(family, n_rays))


def pack(code, fp16):
    from ssdnerf_amd.decoders import pack_triplanes
    planes = pack_triplanes(cu(code)[None] if code.ndim == 4 else cu(code), torch.float16 if fp16 else torch.float32)
    return planes


def collect(dec, out, s=0):
    assert int(dec.last_render_stats["overflow"].item()) == 0
    return dict(image=out["image"][s].cpu().numpy(), depth=out["depth"][s].cpu().numpy(), weights_sum=out["weights_sum"][s].cpu().numpy(),
                sample_counts=dec.last_render_stats["sample_counts"][s].cpu().numpy())


def run_render(dec, c, pipeline):
    dec.fused_pipeline = pipeline
    try:
        with torch.no_grad():
            out = dec.render_packed(pack(c.code, c.fp16), cu(c.rays_o)[None], cu(c.rays_d)[None], cu(c.bits)[None], [c.grid], [c.dt_gamma], c.T_thresh,
                                    bg_color=c.bg, want_counts=True, check_overflow=False)
        return collect(dec, out)
    finally:
        dec.fused_pipeline = "queue_mfma"


# ------------------------------------------------------------------------------------------------ point_decode
def run_point_decode(dec, c, density_only):
    code = cu(c.code)[None]
    with torch.no_grad():
        sig, rgb, n = dec._point_decode_hip([cu(c.xyz)], None if density_only else [cu(c.dirs)], code, density_only, planes=pack(c.code, c.fp16))
    assert n == [len(c.xyz)]
    return sig.cpu().numpy(), None if rgb is None else rgb.cpu().numpy()


def point_failures(c, ref, sig, rgb):
    res = dict(sigma=RR.check_le(sig, ref[0], ref[1]))
    if rgb is not None:
        res["rgb"] = RR.check_le(rgb, ref[2], ref[3])
    return res


@pytest.mark.parametrize("density_only", [False, True], ids=["colour", "density-only"])
@pytest.mark.parametrize("name", [p[0] for p in RR.POINT_CASES])
def test_point_decode_meets_the_per_sample_bounds(name, density_only):
    c, ref = RR.point_reference(name)
    sig, rgb = run_point_decode(make_decoder(c), c, density_only)
    res = point_failures(c, ref, sig, rgb)
    print(name, density_only, {k: round(v[1], 3) for k, v in res.items()})
    assert RR.n_failures(res) == 0, res


def test_point_decode_api_is_the_same_kernel():
    """``point_decode`` / ``point_density_decode`` (fp32 planes packed from the code) give the values checked above, bit for bit"""
    c, _ = RR.point_reference("square-fp32")
    dec = make_decoder(c)
    sig0, rgb0 = run_point_decode(dec, c, False)
    with torch.no_grad():
        sig, rgb, _ = dec.point_decode([cu(c.xyz)], [cu(c.dirs)], cu(c.code)[None])
        sd, _ = dec.point_density_decode([cu(c.xyz)], cu(c.code)[None])
    assert np.array_equal(sig.cpu().numpy(), sig0) and np.array_equal(rgb.cpu().numpy(), rgb0) and np.array_equal(sd.cpu().numpy(), sig0)


# ------------------------------------------------------------------------------------------------ fused render
@pytest.mark.parametrize("pipeline", PIPELINES)
@pytest.mark.parametrize("family,n_rays", RR.CASES)
def test_fused_render_meets_the_per_ray_bounds(family, n_rays, pipeline):
    c, ref = RR.reference(family, n_rays, pipeline == "queue_mfma")
    assert int(ref.undecided.sum()) <= RR.MAX_UNDECIDED * n_rays
    res = RR.ray_failures(run_render(case_decoder(family, n_rays), c, pipeline), ref)
    print(family, n_rays, pipeline, {k: round(v[1], 3) for k, v in res.items()})
    assert RR.n_failures(res) == 0, res


def cams_case():
    """the smooth family's scene seen by two cameras of 16 x 24 pixels; the rays are ``nerf.get_cam_rays``' on the GPU, which the render kernels
    generate bit for bit (tests/test_render_gpu.py::test_camera_fed_render_is_bit_identical_to_ray_arrays)"""
    from ssdnerf_amd import nerf, synthetic as S
    c = RR.case("smooth", 257)
    poses = S.spiral_poses()[[64, 200]].cuda()[None].contiguous()
    intr = (S.cars_intrinsics(128, 128) * torch.tensor([0.55, 0.55, 24 / 128, 16 / 128])).cuda()[None, None].expand(1, 2, -1).contiguous()
    ro, rd = nerf.get_cam_rays(poses, intr, 16, 24)
    c = SimpleNamespace(**{**c.__dict__, "rays_o": ro.reshape(-1, 3).cpu().numpy(), "rays_d": rd.reshape(-1, 3).cpu().numpy()})
    return c, (poses, intr, 16, 24)


def run_cams():
    c, cams = cams_case()
    ref = RR.render_ref(c, True)
    dec = case_decoder("smooth", 257)
    with torch.no_grad():
        out = dec.render_packed(pack(c.code, False), None, None, cu(c.bits)[None], [c.grid], [c.dt_gamma], c.T_thresh, bg_color=c.bg, want_counts=True,
                                check_overflow=False, cams=cams)
    return ref, RR.ray_failures(collect(dec, out), ref)


def test_camera_fed_render_meets_the_per_ray_bounds():
    ref, res = run_cams()
    assert int(ref.undecided.sum()) <= RR.MAX_UNDECIDED * len(ref.count) and int((ref.count > 0).sum()) >= 20
    print("cams", {k: round(v[1], 3) for k, v in res.items()})
    assert RR.n_failures(res) == 0, res


def batch_cases():
    """two unequal scenes under one decoder: the smooth family's, and another object (``make_triplane(12)``) behind the same bitfield with other rays and
    the cone angle of ``DT_GAMMAS[1]``"""
    from ssdnerf_amd import synthetic as S
    a, b = RR.case("smooth", 257), RR.case("smooth-cone", 257)
    b = SimpleNamespace(**{**b.__dict__, "code": S.make_triplane(12).numpy(), "sd": a.sd, "P": a.P})
    return a, b


def run_batch(pipeline):
    a, b = batch_cases()
    dec = case_decoder("smooth", 257)
    dec.fused_pipeline = pipeline
    try:
        with torch.no_grad():
            out = dec.render_packed(pack(np.stack([a.code, b.code]), False), cu(np.stack([a.rays_o, b.rays_o])), cu(np.stack([a.rays_d, b.rays_d])),
                                    cu(np.stack([a.bits, b.bits])), a.grid, torch.tensor([a.dt_gamma, b.dt_gamma], dtype=torch.float32).cuda(), a.T_thresh,
                                    bg_color=a.bg, want_counts=True, check_overflow=False)
        refs = [RR.render_ref(c, pipeline == "queue_mfma") for c in (a, b)]
        return refs, [RR.ray_failures(collect(dec, out, s), refs[s]) for s in range(2)]
    finally:
        dec.fused_pipeline = "queue_mfma"


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_two_scene_batch_with_per_scene_cone_angles_meets_the_bounds(pipeline):
    refs, res = run_batch(pipeline)
    for s in range(2):
        assert int(refs[s].undecided.sum()) <= RR.MAX_UNDECIDED * len(refs[s].count) and int(refs[s].count.sum()) > 500
        print("batch", pipeline, s, {k: round(v[1], 3) for k, v in res[s].items()})
        assert RR.n_failures(res[s]) == 0, (s, res[s])


# ------------------------------------------------------------------------------------------------ the built-in control
def run_control():
    """flat x8 under the MFMA bound: {3: failures of the opt-in three-product direction term, 6: of the default}"""
    c, ref = RR.reference("flat-x8", 4097, True)
    dec = case_decoder("flat-x8", 4097)
    res = {}
    for n in (3, 6):
        dec.shade_dir_products = n
        try:
            res[n] = RR.ray_failures(run_render(dec, c, "queue_mfma"), ref)
        finally:
            dec.shade_dir_products = type(dec).shade_dir_products
    return res


def test_three_direction_products_leave_the_bound_that_six_meet():
    """the control: an existing, supported kernel variant whose direction term carries 16 significand bits per factor must put at least one ray outside
    the MFMA bound on the family that is sharp for the split products, while the default six-product kernel is inside it"""
    assert type(case_decoder("flat-x8", 4097)).shade_dir_products == 6
    res = run_control()
    print("control: three products", res[3]["image"], "six products", res[6]["image"])
    assert RR.n_failures(res[6]) == 0, res[6]
    assert res[3]["image"][0] >= 1 and res[3]["image"][1] > 1.0, res[3]
    assert res[3]["counts"][0] == 0 and res[3]["depth"][0] == 0 and res[3]["weights_sum"][0] == 0      # (the direction term reaches the colour only)


# ------------------------------------------------------------------------------------------------ the measured ratios
def measure():
    worst = {}

    def note(key, res):
        for k, v in res.items():
            if k not in ("counts", "sane"):
                worst.setdefault(key, {})[k] = max(worst.get(key, {}).get(k, 0.0), round(v[1], 4))
        assert RR.n_failures(res) == 0, (key, res)

    for name, _, _ in RR.POINT_CASES:
        c, ref = RR.point_reference(name)
        note("point_decode/" + name, point_failures(c, ref, *run_point_decode(make_decoder(c), c, False)))
    for family, n_rays in RR.CASES:
        for pipeline in PIPELINES:
            c, ref = RR.reference(family, n_rays, pipeline == "queue_mfma")
            note(f"render/{family}/{pipeline}", RR.ray_failures(run_render(case_decoder(family, n_rays), c, pipeline), ref))
    note("render/cams/queue_mfma", run_cams()[1])
    for pipeline in PIPELINES:
        for s, res in enumerate(run_batch(pipeline)[1]):
            note(f"render/batch-scene{s}/{pipeline}", res)
    ctl = run_control()
    control = {f"{n}_products": dict(rays_outside=ctl[n]["image"][0], worst_ratio=round(ctl[n]["image"][1], 4)) for n in (3, 6)}
    return worst, control


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    worst, control = measure()
    out = dict(what="worst |kernel - fp64 reference| / bound per output, over every seeded case of tests/test_render_fp64_gpu.py",
               device=torch.cuda.get_device_name(0), c_exp=RR.C_EXP, c_x=RR.C_X, worst_ratio=worst, control_flat_x8_image=control)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))
