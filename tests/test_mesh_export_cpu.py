"""CPU half of the mesh export: the float64 reference of the attribute kernel is right, the error bound of its density
gradient holds for a plain fp32 evaluation and rejects wrong gradients, and the STL / PLY writers round-trip bit for bit."""
import os

import numpy as np
import pytest
import torch

import _mesh_attr_ref as R


@pytest.fixture(scope="module")
def scene():
    from ssdnerf_amd import synthetic as S
    sd, code = S.make_decoder_params(), S.make_triplane(2021)
    P = R.params64(sd)
    return dict(P=P, P32={k: v.float() for k, v in P.items()}, code=code, c64=R.planes64(code))


def _surface_points(sc, res):
    vol = R.density_volume(sc["P"], sc["c64"], res)
    v = R.crossing_vertices(vol.numpy(), 10.0)
    lo = np.full(3, -1.1, np.float32)
    scale = ((lo.astype(np.float64) * -2) / (res - 1.0)).astype(np.float32)
    return torch.from_numpy(R.fma_world(v, lo, scale))


def test_reference_gradient_equals_central_differences(scene):
    """autograd's grad sigma in float64 against float64 central differences (step 1e-6) at 2 000 random points inside the box that are at least 1e-3
    texel units from every texel centre line, to 1e-6 of |grad sigma|"""
    P, c64 = scene["P"], scene["c64"]
    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(4000, 3, generator=g, dtype=torch.float64) * 2 - 1) * 0.99
    pts = pts[~R.excluded(pts, 128)][:2000]
    assert len(pts) == 2000
    _, grad, _, _ = R.sigma_and_grad(P, c64, pts)
    step, fd = 1e-6, torch.zeros_like(grad)
    for a in range(3):
        e = torch.zeros(3, dtype=torch.float64)
        e[a] = step
        sp, sm = R.sigma_and_grad(P, c64, pts + e)[0], R.sigma_and_grad(P, c64, pts - e)[0]
        fd[:, a] = (sp - sm) / (2 * step)
    rel = (grad - fd).norm(dim=1) / grad.norm(dim=1).clamp(min=1e-300)
    print(f"autograd vs central differences: worst relative error {float(rel.max()):.3e}")
    assert float(rel.max()) <= 1e-6
    # ... and the kernel's formulas, written out in float64, are the same function
    _, g2 = R.explicit_grad(P, c64, pts)
    assert float(((g2 - grad).norm(dim=1) / grad.norm(dim=1).clamp(min=1e-300)).max()) <= 1e-12


def test_sh16_matches_the_closed_forms():
    """the recurrence of csrc/sh_basis.h restated in float64 against the polynomials of the reference's kernel (shencoder.cu:60-82)"""
    d = torch.nn.functional.normalize(torch.randn(257, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64), dim=1)
    x, y, z = d.unbind(1)
    want = torch.stack([
        torch.full_like(x, 0.28209479177387814), -0.48860251190291987 * y, 0.48860251190291987 * z, -0.48860251190291987 * x,
        1.0925484305920792 * x * y, -1.0925484305920792 * y * z, 0.94617469575755997 * z * z - 0.31539156525251999, -1.0925484305920792 * x * z,
        0.54627421529603959 * (x * x - y * y), 0.59004358992664352 * y * (-3 * x * x + y * y), 2.8906114426405538 * x * y * z,
        0.45704579946446572 * y * (1 - 5 * z * z), 0.3731763325901154 * z * (5 * z * z - 3), 0.45704579946446572 * x * (1 - 5 * z * z),
        1.4453057213202769 * z * (x * x - y * y), 0.59004358992664352 * x * (-x * x + 3 * y * y)], dim=1)
    assert float((R.sh16(d) - want).abs().max()) <= 1e-14


@pytest.mark.parametrize("plane_dtype", [torch.float32, torch.float16])
def test_bound_holds_for_fp32_and_rejects_wrong_gradients(scene, plane_dtype):
    """c = 8 on surface vertices (96^3) and on 20 000 random points: an explicit fp32 evaluation of the kernel's formulas meets it on both, fp32
    autograd (ATen's bilinear fraction) on the surface -- on random points its worst ratio is recorded and held to 4 c (tests/_mesh_attr_ref.py says
    why); five wrong gradients, evaluated in float64, do not meet it."""
    P, P32 = scene["P"], scene["P32"]
    c64 = R.planes64(scene["code"], plane_dtype)
    c32 = c64.float()
    for name, pts, gamma in (("surface 96^3", _surface_points(dict(scene, c64=c64), 96), R.GAMMA), ("random", R.random_points(20000, 7), R.GAMMA)):
        keep = ~R.excluded(pts, 128)
        assert float((~keep).double().mean()) <= 0.01
        p64 = pts.double()
        _, ref, _, _ = R.sigma_and_grad(P, c64, p64)
        A = R.bound_magnitude(P, c64, p64)
        w_exp, n = R.worst_ratio(R.explicit_grad(P32, c32, pts)[1], ref, A, keep)
        w_aut, _ = R.worst_ratio(R.sigma_and_grad(P32, c32, pts)[1], ref, A, keep)
        print(f"{name} ({plane_dtype}): {n} components, worst err / (u A): explicit fp32 {w_exp:.1f}, fp32 autograd {w_aut:.1f}, allowed {gamma / R.U32:.0f}")
        w_ord, _ = R.worst_ratio(R.explicit_grad(P32, c32, pts, "aten_order")[1], ref, A, keep)
        print(f"  explicit fp32 with ATen's fraction ix - floor(ix): {w_ord:.1f}")
        assert w_exp <= gamma / R.U32
        assert w_aut <= (R.GAMMA if name != "random" else R.GAMMA_ATEN_RANDOM) / R.U32
        clipped = R.clipped_axes(p64, 128)[keep]
        for variant in ("missing_plane", "sigmoid_for_dsilu", "no_half_size", "align_corners", "clipped_moves"):
            _, gv = R.explicit_grad(P, c64, p64, variant)
            bad = ((gv - ref).abs() > gamma * A)[keep]
            if variant == "clipped_moves":                                # differs on clipped axes only: none on a surface inside the box
                if not clipped.any():
                    continue
                bad = bad[clipped]                                        # (on the high border i1 == i0 and the mistake is invisible: about half are left)
            share = float(bad.double().mean())
            print(f"  {variant}: {100 * share:.1f} % of components outside the bound")
            assert share >= 0.30, (name, variant, share)


def test_fp32_colour_evaluation_is_within_the_projects_rgb_tolerance(scene):
    """the GPU test compares colours at atol 2e-6 (tests/test_golden.py's rgb tolerance): an fp32 eager evaluation on the CPU is within it"""
    P, P32, c64 = scene["P"], scene["P32"], scene["c64"]
    pts = torch.cat([_surface_points(scene, 64), R.random_points(5000, 3)])
    _, g, _, _ = R.sigma_and_grad(P, c64, pts.double())
    n = (-g / g.norm(dim=1, keepdim=True).clamp(min=1e-300)).float()
    d = R.view_dirs(n.clone())
    err = (R.colors(P32, c64.float(), pts, d, 0.001).double() - R.colors(P, c64, pts.double(), d.double(), 0.001)).abs().max()
    print(f"fp32 eager colour against float64: worst {float(err):.2e}")
    assert float(err) <= 2e-6


# ------------------------------------------------------------------------------------------------ writers
def _tetrahedron():
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32) * np.float32(0.7) + np.float32(0.1)
    return v, np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], np.int32)


def _sphere():
    from ssdnerf_amd.mesh import marching_cubes_reference
    g = np.arange(24, dtype=np.float32)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    return marching_cubes_reference(8.3 - np.sqrt((X - 11.4) ** 2 + (Y - 11.7) ** 2 + (Z - 12.1) ** 2), 0.0)


@pytest.mark.parametrize("make", [_tetrahedron, _sphere])
def test_stl_round_trip(tmp_path, make):
    from ssdnerf_amd import mesh as M
    v, t = make()
    path = str(tmp_path / "m.stl")
    M.write_stl(path, v, t)
    assert os.path.getsize(path) == 84 + 50 * len(t)
    raw = open(path, "rb").read()
    assert int(np.frombuffer(raw, "<u4", 1, 80)[0]) == len(t)
    assert not np.frombuffer(raw[84:], np.uint8).reshape(len(t), 50)[:, 48:].any()       # the attribute word
    normals, corners = M.read_stl(path)
    assert np.array_equal(corners.view(np.uint32), v[t].view(np.uint32))
    p = corners.astype(np.float64)
    c = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    want = (c / np.linalg.norm(c, axis=1, keepdims=True)).astype(np.float32)
    assert np.array_equal(normals.view(np.uint32), want.view(np.uint32))
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() <= 2e-7


def test_stl_degenerate_triangle_gets_normal_zero(tmp_path):
    from ssdnerf_amd import mesh as M
    v = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    M.write_stl(str(tmp_path / "d.stl"), v, np.array([[0, 1, 2]], np.int32))
    normals, _ = M.read_stl(str(tmp_path / "d.stl"))
    assert np.array_equal(normals, np.zeros((1, 3), np.float32))


@pytest.mark.parametrize("make", [_tetrahedron, _sphere])
def test_ply_round_trip(tmp_path, make):
    from ssdnerf_amd import mesh as M
    v, t = make()
    rng = np.random.default_rng(0)
    n = rng.standard_normal((len(v), 3)).astype(np.float32)
    c = rng.integers(0, 256, (len(v), 3)).astype(np.uint8)
    for normals, colors in ((None, None), (n, None), (None, c), (n, c)):
        path = str(tmp_path / "m.ply")
        M.write_ply(path, v, t, normals=normals, colors=colors)
        got = M.read_ply(path)
        assert np.array_equal(got["vertices"].view(np.uint32), v.view(np.uint32)) and np.array_equal(got["triangles"], t)
        assert got["triangles"].dtype == np.int32 and got["vertices"].dtype == np.float32
        assert (got["normals"] is None) if normals is None else np.array_equal(got["normals"].view(np.uint32), n.view(np.uint32))
        assert (got["colors"] is None) if colors is None else (got["colors"].dtype == np.uint8 and np.array_equal(got["colors"], c))
    head = ("ply\nformat binary_little_endian 1.0\ncomment ssdnerf_amd\n" + f"element vertex {len(v)}\n"
            "property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            "property uchar red\nproperty uchar green\nproperty uchar blue\n" + f"element face {len(t)}\n"
            "property list uchar int vertex_indices\nend_header\n").encode("ascii")
    raw = open(path, "rb").read()
    assert raw.startswith(head) and len(raw) == len(head) + len(v) * 27 + len(t) * 13
    assert raw[len(head) + len(v) * 27] == 3                                             # the first face's vertex count


def test_empty_meshes_are_valid_files(tmp_path):
    from ssdnerf_amd import mesh as M
    e3 = np.zeros((0, 3), np.float32)
    M.write_stl(str(tmp_path / "e.stl"), e3, np.zeros((0, 3), np.int32))
    assert os.path.getsize(str(tmp_path / "e.stl")) == 84
    normals, corners = M.read_stl(str(tmp_path / "e.stl"))
    assert normals.shape == (0, 3) and corners.shape == (0, 3, 3)
    M.write_ply(str(tmp_path / "e.ply"), e3, np.zeros((0, 3), np.int32), normals=e3, colors=np.zeros((0, 3), np.uint8))
    got = M.read_ply(str(tmp_path / "e.ply"))
    assert got["vertices"].shape == (0, 3) and got["triangles"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["colors"].shape == (0, 3)
    assert b"element vertex 0\n" in open(str(tmp_path / "e.ply"), "rb").read() and b"element face 0\n" in open(str(tmp_path / "e.ply"), "rb").read()


def test_readers_reject_other_files(tmp_path):
    from ssdnerf_amd import mesh as M
    (tmp_path / "x.stl").write_bytes(b"solid ascii\nendsolid\n")
    (tmp_path / "x.ply").write_bytes(b"ply\nformat ascii 1.0\nelement vertex 0\nend_header\n")
    with pytest.raises(ValueError):
        M.read_stl(str(tmp_path / "x.stl"))
    with pytest.raises(ValueError):
        M.read_ply(str(tmp_path / "x.ply"))


def test_abi_entry_is_declared_and_exported():
    from ssdnerf_amd import _cabi as C, build
    assert "ssdnerf_mesh_vertex_attributes" in C.EXPORTS and "mesh_attr.hip" in build.SOURCES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ssdnerf_hip.h")).read()
    assert "int ssdnerf_mesh_vertex_attributes(" in header
