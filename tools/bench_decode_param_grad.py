"""The decode of the joint iteration of a training step with a TRAINABLE decoder: ``param_grad='eager'`` (grid_sample + nn.Linear under autograd, the default) against
``param_grad='fused'`` (the fused decode forward, ``ssdnerf_point_decode_backward_params`` and the code-gradient launches: one ``_PointDecodeFn``; csrc/decode_bwd_params.hip).

At the joint step's shape -- 8 scenes x 2^12 rays, the synthetic object scenes of the stage-1 model of tests/test_tv_loss_gpu.py, the samples the train march yields
(captured from a real ``train_step``) -- it reports, by HIP events, median (min - max) over windows taken in turn:
  * ``param_launches_ms``   the two new launches alone, through the C ABI;
  * ``code_launches_ms``    the three launches of ``ssdnerf_point_decode_backward`` next to them;
  * ``fused_fwd_bwd_ms``    ``point_decode`` + backward with ``param_grad='fused'``: everything the mode runs, Python included;
  * ``eager_fwd_bwd_ms``    the same with ``param_grad='eager'``: what it replaces;
  * ``frozen_fwd_bwd_ms``   the same call on a frozen copy of the decoder, gradient w.r.t. the code only: the path of guidance and fine-tuning;
  * ``train_step``          ms per ``MultiSceneNeRF.train_step`` (``extra_scene_step=15``, ``HIPAdam``) in both modes, host clock over synchronised windows, with
                            ``gap_exceeds_spread``: whether the two modes' [min, max] intervals are disjoint.
The upstream gradients of the isolated timings are random and non-zero on every sample (no sample is skipped: the launches' worst case).  The speed is reported, not
promised; the default path is the parent commit's.

Prints one JSON line.   usage: python tools/bench_decode_param_grad.py [--iters 20] [--windows 5] [--calls 3] > profiles/decode_param_grad.json"""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCENES, RAYS = 8, 2 ** 12


def _spread(vals):
    return dict(median=round(statistics.median(vals), 4), min=round(min(vals), 4), max=round(max(vals), 4))


def _window(fn, steps):
    """(HIP-event ms per call, host wall ms per call) of ``steps`` calls between two synchronisations"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def _alternate(fns, steps, windows, warmup):
    """{name: (event ms per window, wall ms per window)}: ``windows`` windows per path, taken in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    got = {name: ([], []) for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            ev, wall = _window(fn, steps)
            got[name][0].append(ev)
            got[name][1].append(wall)
    return got


def _model(param_grad):
    import test_tv_loss_gpu as TV
    cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=15, n_inverse_rays=RAYS, n_decoder_rays=RAYS, loss_coef=0.1 / (64 * 64),
               optimizer=dict(type="HIPAdam", lr=1e-2, weight_decay=0.))
    m = TV._stage1_model(train_cfg=cfg).train()
    m.decoder.param_grad = param_grad
    from ssdnerf_amd.optim import HIPAdam
    return m, dict(decoder=HIPAdam(m.decoder.parameters(), lr=1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20, help="calls per window of the isolated timings")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3, help="train_step calls per window")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decode_param_grad: needs the GPU (no HIP device visible)")
    import test_tv_loss_gpu as TV
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd.decoders import MLP_PARAM_FLOATS, pack_triplanes
    imgs, poses, intr = TV._views(list(range(51, 51 + SCENES)), [30, 150])
    data = dict(scene_id=list(range(SCENES)), scene_name=[f"s{i}" for i in range(SCENES)], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr)
    models = {mode: _model(mode) for mode in ("eager", "fused")}

    # ---- the joint step's decode call, captured from a real train_step (the last point_decode with a trainable decoder and view directions)
    m, opt = models["fused"]
    dec = m.decoder
    seen = {}
    real = dec.point_decode

    def capture(xyzs, dirs, code, density_only=False):
        if dirs is not None and not density_only and torch.is_grad_enabled() and any(p.requires_grad for p in dec.parameters()):
            seen.update(xyzs=[x.detach().clone() for x in xyzs], dirs=[d.detach().clone() for d in dirs], code=code.detach().clone())
        return real(xyzs, dirs, code, density_only)
    dec.point_decode = capture
    torch.manual_seed(0)
    m.train_step(data, opt)
    del dec.point_decode
    xyzs, dirs, code = seen["xyzs"], seen["dirs"], seen["code"]
    num = [int(x.size(0)) for x in xyzs]
    total = sum(num)
    g = torch.Generator(device="cuda").manual_seed(1)
    gs, gc = torch.randn(total, device="cuda", generator=g) * 0.1, torch.randn(total, 3, device="cuda", generator=g)

    # ---- the launches alone, through the C ABI
    lib = C.lib()
    planes = pack_triplanes(code, dec.plane_dtype)
    S, _, hp, wp, _ = planes.shape
    xyz_all, dir_all = torch.cat(xyzs).contiguous(), torch.cat(dirs).contiguous()
    offsets = torch.tensor([sum(num[:s]) for s in range(S + 1)], dtype=torch.int32, device="cuda")
    P = dec.packed_params()
    gp = torch.empty(MLP_PARAM_FLOATS, device="cuda")
    grad_code = torch.empty(S, 3, 6, hp, wp, device="cuda")
    pw = int(lib.ssdnerf_point_decode_backward_params_workspace(C.u32(S), C.u32(total), C.u32(0)))
    cw = int(lib.ssdnerf_point_decode_backward_workspace(C.u32(S), C.u32(total), C.u32(hp), C.u32(wp)))
    ws_p, ws_c = torch.empty(pw, dtype=torch.uint8, device="cuda"), torch.empty(cw, dtype=torch.uint8, device="cuda")
    common = (C.ptr(planes), C.dtype_code(planes), C.u32(S), C.u32(hp), C.u32(wp), C.ptr(P), C.ptr(xyz_all), C.ptr(dir_all), C.ptr(offsets), C.u32(total),
              C.f32(dec.sigmoid_saturation), C.ptr(gs), C.ptr(gc))

    def param_launches():
        C.check(lib.ssdnerf_point_decode_backward_params(*common, C.ptr(gp), C.u32(0), C.ptr(ws_p), ctypes.c_size_t(pw), C.stream()), "point_decode_backward_params")

    def code_launches():
        C.check(lib.ssdnerf_point_decode_backward(*common, C.ptr(grad_code), C.ptr(ws_c), ctypes.c_size_t(cw), C.stream()), "point_decode_backward")

    # ---- forward + backward through point_decode, both modes, on one decoder
    leaf = code.clone().requires_grad_(True)
    params = list(dec.parameters())

    def fwd_bwd(mode):
        def run():
            dec.param_grad = mode
            sig, rgb, _ = dec.point_decode(xyzs, dirs, leaf)
            torch.autograd.grad((sig, rgb), [leaf] + params, (gs, gc))
        return run
    frozen = copy.deepcopy(dec).requires_grad_(False)

    def frozen_fwd_bwd():
        sig, rgb, _ = frozen.point_decode(xyzs, dirs, leaf)
        torch.autograd.grad((sig, rgb), [leaf], (gs, gc))
    iso = _alternate({"param_launches_ms": param_launches, "code_launches_ms": code_launches, "fused_fwd_bwd_ms": fwd_bwd("fused"), "eager_fwd_bwd_ms": fwd_bwd("eager"),
                      "frozen_fwd_bwd_ms": frozen_fwd_bwd}, args.iters, args.windows, warmup=3)
    dec.param_grad = "fused"
    res = dict(tool="bench_decode_param_grad", device=torch.cuda.get_device_name(0), scenes=SCENES, rays_per_scene=RAYS, samples_total=total,
               samples_per_scene=num, planes=[int(hp), int(wp)], plane_dtype=str(dec.plane_dtype).replace("torch.", ""),
               blocks=pw // (MLP_PARAM_FLOATS * 4), upstream="random, non-zero on every sample", calls_per_window=args.iters, windows=args.windows)
    res.update({k: _spread(ev) for k, (ev, _) in iso.items()})

    # ---- the whole training step, both modes, windows taken in turn
    torch.manual_seed(0)
    steps = _alternate({mode: (lambda m=m, opt=opt: m.train_step(data, opt)) for mode, (m, opt) in models.items()}, args.calls, args.windows, warmup=2)
    ts = {mode: _spread(wall) for mode, (_, wall) in steps.items()}
    disjoint = ts["fused"]["max"] < ts["eager"]["min"] or ts["eager"]["max"] < ts["fused"]["min"]
    res["train_step"] = dict(extra_scene_step=15, optimizer="HIPAdam", calls_per_window=args.calls, windows=args.windows, eager_ms=ts["eager"], fused_ms=ts["fused"],
                             gap_ms=round(ts["eager"]["median"] - ts["fused"]["median"], 4), gap_exceeds_spread=bool(disjoint))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
