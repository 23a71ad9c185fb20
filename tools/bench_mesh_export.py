"""Mesh export at the reference's resolution (256^3, threshold 10) on ``synthetic.make_triplane(2021)`` and on a batch of 8
(``make_scene_batch``): HIP-event means (warm-up, then --reps) of the three device stages -- density volume (``nerf.extract_density_volume``), marching
cubes (``mesh.marching_cubes``, its one host read included), the attribute kernel (``ssdnerf_mesh_vertex_attributes``, csrc/mesh_attr.hip) -- with V
and T; the same attributes through the eager restatement on the same device (``grid_sample`` + ``nn.Linear``, ``torch.autograd.grad`` for the density
gradient, a second eager decode for the colour); and wall seconds of ``BaseNeRF.save_mesh`` per scene for both formats, file writing included.
Prints one JSON line and writes it to --out.   usage: python tools/bench_mesh_export.py [--reps 20] [--out profiles/mesh_export.json]"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _events_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _eager_attributes(dec, code, xyz):
    """what the kernel computes, through the reference-shaped eager decode: sigma and its gradient by autograd, the normal, a second decode for rgb"""
    x = xyz.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        sigma, _, _ = dec.point_decode_eager([x], None, code[None], density_only=True)
        (g,) = torch.autograd.grad(sigma.sum(), x)
    n = -torch.nn.functional.normalize(g, dim=-1)
    with torch.no_grad():
        _, rgb, _ = dec.point_decode_eager([xyz], [-n], code[None])
    return sigma.detach(), g, n, rgb, torch.round(rgb.clamp(0, 1) * 255).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_export.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh_export: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import mesh as M, nerf, synthetic as S
    from ssdnerf_amd.decoders import TriPlaneDecoder
    from ssdnerf_amd.models import BaseNeRF
    dec = TriPlaneDecoder(interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True, dir_layers=[16, 64],
                          activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)
    dec.load_state_dict(S.make_decoder_params(), strict=False)
    dec = dec.cuda().eval()
    res, thr = args.resolution, args.threshold
    b_min, b_max = (dec.aabb[:3] - 0.1).cpu().numpy(), (dec.aabb[3:] + 0.1).cpu().numpy()

    def stages(code):
        vol = nerf.extract_density_volume(dec, code, res)
        v_idx, tris = M.marching_cubes(vol, thr)
        out = dict(V=int(v_idx.size(0)), T=int(tris.size(0)))
        out["density_volume_ms"] = _events_ms(lambda: nerf.extract_density_volume(dec, code, res), args.reps, args.warmup)
        out["marching_cubes_ms"] = _events_ms(lambda: M.marching_cubes(vol, thr), args.reps, args.warmup)
        out["vertex_attributes_ms"] = _events_ms(lambda: M.vertex_attributes(dec, code, v_idx, b_min, b_max, res), 5 * args.reps, args.warmup)
        att = M.vertex_attributes(dec, code, v_idx, b_min, b_max, res, want_grad=True)
        out["eager_attributes_ms"] = _events_ms(lambda: _eager_attributes(dec, code, att["xyz"]), args.reps, args.warmup)
        _, g, n, rgb, _ = _eager_attributes(dec, code, att["xyz"])
        out["eager_vs_kernel"] = dict(grad_rel=float((g - att["grad_sigma"]).norm() / g.norm()), normal_max=float((n - att["normals"]).abs().max()),
                                      rgb_max=float((rgb - att["colors"]).abs().max()))
        total = out["density_volume_ms"] + out["marching_cubes_ms"] + out["vertex_attributes_ms"]
        out["attribute_share_of_device_stages"] = out["vertex_attributes_ms"] / total
        return out

    single = stages(S.make_triplane(2021).cuda())
    codes = S.make_scene_batch(args.scenes).cuda()
    per_scene = [stages(c) for c in codes]
    keys = ("density_volume_ms", "marching_cubes_ms", "vertex_attributes_ms", "eager_attributes_ms", "attribute_share_of_device_stages")
    batch = dict(scenes=args.scenes, V=[s["V"] for s in per_scene], T=[s["T"] for s in per_scene],
                 **{k + "_per_scene": sum(s[k] for s in per_scene) / len(per_scene) for k in keys})
    names = [f"scene_{i}" for i in range(args.scenes)]
    save = {}
    with tempfile.TemporaryDirectory() as tmp:
        BaseNeRF.save_mesh(tmp, dec, codes[:1], names[:1], res, thr)                      # warm-up (tables, allocator)
        for fmt in ("stl", "ply"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            BaseNeRF.save_mesh(tmp, dec, codes, names, res, thr, mesh_format=fmt)
            save[f"save_mesh_{fmt}_s_per_scene"] = (time.perf_counter() - t0) / args.scenes
            save[f"{fmt}_mbytes_per_scene"] = sum(os.path.getsize(os.path.join(tmp, n + "." + fmt)) for n in names) / args.scenes / 1e6
    rnd = lambda o: {k: rnd(v) for k, v in o.items()} if isinstance(o, dict) else [rnd(v) for v in o] if isinstance(o, list) else float(f"{o:.4g}") if isinstance(o, float) else o
    line = json.dumps(rnd(dict(tool="bench_mesh_export", resolution=res, threshold=thr, reps=args.reps, device=torch.cuda.get_device_name(0),
                               single=single, batch=batch, **save)))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
