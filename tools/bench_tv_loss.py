"""Total-variation regulariser (ssdnerf_tv_loss_forward / _backward, csrc/tv_loss.hip) at the stage-1 batch, 8 scenes x 3 planes x 6 channels x
128 x 128: forward + backward by HIP events (warm-up, then the mean of --reps pairs), the bytes they move and that figure over 8 TB/s; the same for
the eager fp32 restatement (diff, cat, stack, norm, pow, mean and its autograd); and ms per stage-1 inversion iteration (8 scenes, 2^14 rays, the
stage-1 model dict) with and without the TV term.  Prints one JSON line.   usage: python tools/bench_tv_loss.py [--reps 200] [--iters 64]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


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


def _eager(t, p):
    diffs = []
    for dim in (-2, -1):
        pad = list(t.shape)
        pad[dim] = 1
        diffs.append(torch.cat([torch.diff(t, dim=dim), t.new_zeros(pad)], dim=dim))
    return torch.stack(diffs, dim=0).norm(dim=0).pow(p).mean(dim=(-2, -1))


def _inversion_ms(with_tv, iters, warmup):
    from ssdnerf_amd import nerf, synthetic as S
    from ssdnerf_amd.density import get_density
    from ssdnerf_amd.registry import MODELS
    dec = dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3], use_dir_enc=True,
               dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256)
    cfg = dict(density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 14, loss_coef=0.1 / (128 * 128), n_inverse_steps=1,
               optimizer=dict(type="Adam", lr=0.08, weight_decay=0.), lr_scheduler=dict(type="ExponentialLR", gamma=0.998))
    m = MODELS.build(dict(type="MultiSceneNeRF", code_size=(3, 6, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64, decoder=dec,
                          decoder_use_ema=True, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
                          reg_loss=dict(type="TVLoss", power=1.5, loss_weight=1.0) if with_tv else None, init_from_mean=True, test_cfg=cfg)).cuda()
    m.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    codes = S.make_scene_batch(8, seed=90).cuda()
    with torch.no_grad():
        _, bits = get_density(m.decoder_ema, codes, 64, density_thresh=0.1, density_step=4)
        poses = S.spiral_poses()[[0, 60, 120, 180]].cuda()[None].expand(8, -1, -1, -1).contiguous()
        intr = S.cars_intrinsics(128, 128).cuda()[None, None].expand(8, 4, -1).contiguous()
        imgs, _ = nerf.render(m.decoder_ema, codes, bits, 128, 128, intr, poses)
        rays_o, rays_d = nerf.get_cam_rays(poses, intr, 128, 128)
    dt_gamma = 0.5 / intr[..., :2].mean(dim=(-2, -1))
    torch.manual_seed(0)
    code_ = m.get_init_code_(8, "cuda")
    grid, bitfield = m.get_init_density_grid(8, "cuda"), m.get_init_density_bitfield(8, "cuda")
    opt = m.build_optimizer(code_, cfg)
    sch = m.build_scheduler(opt, cfg)

    def run(steps):                                                   # one call: the density refresh every 16 iterations, as in val_step
        with torch.enable_grad():
            m.inverse_code(m.decoder_ema, imgs.clamp(0, 1), rays_o, rays_d, dt_gamma=dt_gamma, cfg=dict(cfg, n_inverse_steps=steps), code_=code_,
                           density_grid=grid, density_bitfield=bitfield, code_optimizer=opt, code_scheduler=sch)
    return _events_ms(lambda: run(iters), 1, warmup) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--power", type=float, default=1.5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tv_loss: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import _cabi as C
    x = torch.randn(args.scenes, 3, 6, 128, 128, device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
    n, h, w = x[..., 0, 0].numel(), 128, 128
    means, grad = torch.empty(x.shape[:-2], device="cuda"), torch.empty_like(x)
    g = torch.full(x.shape[:-2], 1.0 / n, device="cuda")
    lib, p = C.lib(), C.f32(args.power)

    def kernels():
        lib.ssdnerf_tv_loss_forward(C.ptr(x), n, h, w, p, C.ptr(means), C.stream())
        lib.ssdnerf_tv_loss_backward(C.ptr(x), C.ptr(g), n, h, w, p, C.ptr(grad), C.stream())
    C.check(lib.ssdnerf_tv_loss_forward(C.ptr(x), n, h, w, p, C.ptr(means), C.stream()), "tv_loss_forward")
    fwd_ms = _events_ms(lambda: lib.ssdnerf_tv_loss_forward(C.ptr(x), n, h, w, p, C.ptr(means), C.stream()), args.reps, args.warmup)
    bwd_ms = _events_ms(lambda: lib.ssdnerf_tv_loss_backward(C.ptr(x), C.ptr(g), n, h, w, p, C.ptr(grad), C.stream()), args.reps, args.warmup)
    both_ms = _events_ms(kernels, args.reps, args.warmup)
    nbytes = 3 * x.numel() * 4 + 2 * n * 4                           # forward reads x; backward reads x, writes dx; g and the means
    leaf = x.clone().requires_grad_(True)

    def eager():
        _eager(leaf, args.power).mean().backward()
        leaf.grad = None
    eager_ms = _events_ms(eager, max(args.reps // 4, 10), args.warmup)
    inv_tv = _inversion_ms(True, args.iters, 1)
    inv_none = _inversion_ms(False, args.iters, 1)
    print(json.dumps(dict(tool="bench_tv_loss", shape=list(x.shape), power=args.power, reps=args.reps,
                          forward_ms=round(fwd_ms, 5), backward_ms=round(bwd_ms, 5), fwd_bwd_ms=round(both_ms, 5), mbytes=round(nbytes / 1e6, 2),
                          min_ms_at_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3, 5), share_of_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3 / both_ms, 3),
                          eager_fwd_bwd_ms=round(eager_ms, 4), inversion_iter_ms_tv=round(inv_tv, 3), inversion_iter_ms_no_tv=round(inv_none, 3))))


if __name__ == "__main__":
    main()
