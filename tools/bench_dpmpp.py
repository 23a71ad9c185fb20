#!/usr/bin/env python
"""tools/bench_dpmpp.py -- the DPM-Solver++(2M) sampler on one MI355X; prints one JSON line (profiles/dpmpp.json).

  kernel     the bare ``ssdnerf_dpmpp_step_v`` launch through the C ABI at 8 x 18 x 128^2 (a second-order step: 12 B read + 8 B written per element)
             against the eager three-term tensor expression on the same GPU: HIP events over windows alternated in one process, once on ONE set of
             buffers (47 MB: resident in the 256 MiB last-level cache, as the sampler's latent is) and once rotating over 8 sets (377 MB: from HBM);
             bytes moved and their share of 8 TB/s
  sampling   scenes/s of unconditional sampling at ``--scenes`` x ``--views`` views (tools/bench_sample.py, one fresh process per figure, fp32 and bf16):
             DDIM 50 on this tree, dpmpp_2m at 20 and at 50 steps and, with ``--parent-tree DIR`` (a checkout of the parent commit with its library
             built), DDIM 50 there; the processes of a round are interleaved and ``--rounds`` rounds show the spread
  bounds     the worst error / bound ratios of tests/test_dpmpp_gpu.py's kernel cases and its two sampler-level differences
  guided     (``--guided``) the conditioning-view PSNR after the guided steps alone of tools/bench_finetune.py's batch under bench.py's synthetic prior, for
             DDIM at the config's 75 steps and dpmpp_2m at 75 and at 30.  For information: random UNet weights, no threshold."""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from ssdnerf_amd import _cabi as C

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8); ap.add_argument("--views", type=int, default=251)
ap.add_argument("--windows", type=int, default=7); ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--rounds", type=int, default=2); ap.add_argument("--parent-tree", default=None)
ap.add_argument("--skip-sampling", action="store_true"); ap.add_argument("--skip-bounds", action="store_true"); ap.add_argument("--guided", action="store_true")
a = ap.parse_args()
assert torch.cuda.is_available(), "bench_dpmpp.py measures on the GPU"
HBM_PEAK = 8.0e12


def spread(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


# ------------------------------------------------------------------------------------------------ kernel
def kernel_leg():
    from ssdnerf_amd.diffusion import NoiseSchedule, SamplingPlan
    s = SamplingPlan(NoiseSchedule(dict(type="linear"), 1000), "dpmpp_2m", 20).steps[10]
    n = a.scenes * 18 * 128 * 128
    g = torch.Generator().manual_seed(0)
    out = dict(elements=n, bytes_moved=20 * n, coefficients=dict(a=s.a, b=s.b, c=s.c, d=s.d, e=s.e), launches_per_window=a.launches, windows=a.windows)
    for name, n_sets in (("resident_one_buffer_set", 1), ("rotating_8_buffer_sets", 8)):
        sets = [[torch.randn(n, generator=g).cuda() for _ in range(3)] + [torch.empty(n, device="cuda") for _ in range(2)] for _ in range(n_sets)]
        fa, fb, fc, fd, fe = (torch.tensor(v, dtype=torch.float32).item() for v in (s.a, s.b, s.c, s.d, s.e))

        def hip(i):
            x, v, q, x0, xn = sets[i % n_sets]
            C.check(C.lib().ssdnerf_dpmpp_step_v(C.ptr(x), C.ptr(v), C.ptr(q), C.ctypes.c_uint64(n), C.f32(s.a), C.f32(s.b), C.f32(s.c), C.f32(s.d), C.f32(s.e),
                                                 C.f32(-2.0), C.f32(2.0), C.ptr(x0), C.ptr(xn), C.stream()), "dpmpp_step_v")

        def eager(i):
            x, v, q, x0, xn = sets[i % n_sets]
            torch.clamp(fa * x - fb * v, -2.0, 2.0, out=x0)
            torch.add(fc * x0 + fd * x, q, alpha=fe, out=xn)

        def window(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.launches            # us per call

        for fn in (hip, eager):                                      # warm-up: code objects, the allocator's pools
            for i in range(20):
                fn(i)
        torch.cuda.synchronize()
        x, v, q, x0, xn = sets[0]
        hip(0); k0, k1 = x0.clone(), xn.clone(); eager(0)
        diff = max(float((k0 - x0).abs().max()), float((k1 - xn).abs().max()))
        t_hip, t_eager = [], []
        for _ in range(a.windows):                                   # alternated
            t_hip.append(window(hip)); t_eager.append(window(eager))
        k, e = spread(t_hip), spread(t_eager)
        out[name] = dict(kernel_us=k, eager_us=e, eager_over_kernel=round(e["median"] / k["median"], 2), kernel_tb_per_s=round(20 * n / k["median"] * 1e-6, 3),
                         kernel_share_of_8_tb_per_s=round(20 * n / (k["median"] * 1e-6) / HBM_PEAK, 3), max_abs_kernel_minus_eager=diff)
        del sets
    return out


# ------------------------------------------------------------------------------------------------ sampling
def sample_once(tree, dtype, method, steps):
    cmd = [sys.executable, os.path.join(tree, "tools", "bench_sample.py"), "--scenes", str(a.scenes), "--views", str(a.views), "--steps", str(steps), "--dtype", dtype,
           "--reps", "3"] + ([] if method == "ddim" else ["--sample-method", method])
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]}")
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    return dict(scenes_per_s=round(line["value"], 2), sampler_ms=line["ddim_ms"], ms_per_step=line["ms_per_ddim_step"], total_s=line["total_s"])


def sampling_leg():
    runs = [("ddim_50_this_tree", ROOT, "ddim", 50), ("dpmpp_2m_20", ROOT, "dpmpp_2m", 20), ("dpmpp_2m_50", ROOT, "dpmpp_2m", 50)]
    if a.parent_tree:
        runs.insert(0, ("ddim_50_parent_commit", os.path.abspath(a.parent_tree), "ddim", 50))
    out = dict(scenes=a.scenes, views_per_scene=a.views, note="tools/bench_sample.py, best of 3 repetitions per process, one process per entry, the entries of a round interleaved; "
                                                              "random weights: timing only")
    for dtype in ("fp32", "bf16"):
        res = {name: [] for name, *_ in runs}
        for _ in range(a.rounds):
            for name, tree, method, steps in runs:
                res[name].append(sample_once(tree, dtype, method, steps))
                print(f"[bench_dpmpp] {dtype} {name}: {res[name][-1]}", file=sys.stderr, flush=True)
        out[dtype] = {name: dict(scenes_per_s=[r["scenes_per_s"] for r in rs], sampler_ms=[r["sampler_ms"] for r in rs], ms_per_step=[r["ms_per_step"] for r in rs])
                      for name, rs in res.items()}
    return out


# ------------------------------------------------------------------------------------------------ bounds, sampler differences
def bounds_leg():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_dpmpp_gpu as T
    return T.measure()


# ------------------------------------------------------------------------------------------------ guided reconstruction (information only)
def guided_leg():
    import numpy as np
    from bench import _KnownScenePrior
    from ssdnerf_amd.registry import MODELS
    from ssdnerf_amd import synthetic as S
    ns = a.scenes
    cfg = dict(type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
               diffusion=dict(type="GaussianDiffusion", num_timesteps=1000, betas_cfg=dict(type="linear"),
                              denoising=dict(type="DenoisingUnetMod", image_size=128, in_channels=18, base_channels=128, channels_cfg=[1, 2, 2, 4, 4],
                                             resblocks_per_downsample=2, dropout=0.0, use_scale_shift_norm=True, downsample_conv=True, upsample_conv=True,
                                             num_heads=4, attention_res=[32, 16, 8]),
                              timestep_sampler=dict(type="SNRWeightedTimeStepSampler", power=0.5), denoising_mean_mode="V",
                              ddpm_loss=dict(type="DDPMMSELossMod", rescale_mode="timestep_weight",
                                             log_cfgs=dict(type="quartile", prefix_name="loss_mse", total_timesteps=1000),
                                             data_info=dict(pred="v_t_pred", target="v_t"), weight_scale=4.0, scale_norm=True)),
               decoder=dict(type="TriPlaneDecoder", interp_mode="bilinear", base_layers=[18, 64], density_layers=[64, 1], color_layers=[64, 3],
                            use_dir_enc=True, dir_layers=[16, 64], activation="silu", sigma_activation="trunc_exp", sigmoid_saturation=0.001, max_steps=256),
               decoder_use_ema=True, freeze_decoder=False, bg_color=1, pixel_loss=dict(type="MSELoss", loss_weight=20.0),
               reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=0,
               test_cfg=dict(img_size=(128, 128), num_timesteps=75, clip_range=[-2, 2], density_thresh=0.1, dt_gamma_scale=0.5, n_inverse_rays=2 ** 14,
                             loss_coef=0.1 / (128 * 128), guidance_gain=3.2 * (2 ** 14), cond_mode="guide"))          # tools/bench_finetune.py's model, guided steps only
    model = MODELS.build(cfg)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in model.diffusion_ema.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    model.decoder_ema.load_state_dict(S.make_decoder_params(), strict=False)
    model = model.cuda().eval()
    codes = torch.stack([S.make_triplane(100 + i) for i in range(ns)]).cuda()
    poses = S.spiral_poses()[[64]].cuda()[None].expand(ns, -1, -1, -1).contiguous()
    intr = S.cars_intrinsics(128, 128).cuda()[None, None].expand(ns, 1, -1).contiguous()
    with torch.no_grad():
        other = codes.roll(1, 0)                                     # views of OTHER scenes than the prior's: a loss with something to fit
        target, _ = model.render(model.decoder_ema, other, model.get_density(model.decoder_ema, other, cfg=model.test_cfg)[1], 128, 128, intr, poses, cfg=model.test_cfg)
    data = dict(cond_imgs=target.clamp(0, 1), cond_intrinsics=intr, cond_poses=poses, test_poses=poses, test_intrinsics=intr)
    noise = torch.randn(ns, 3, 6, 128, 128, generator=g).cuda()
    cond = data["cond_imgs"][:, 0].permute(0, 3, 1, 2)
    prior = _KnownScenePrior(model, 0.8 * codes)
    out = dict(note="conditioning-view PSNR (dB, mean and min over the scenes) after the guided steps alone (cond_mode 'guide'), synthetic prior of bench.py "
                    "(_KnownScenePrior) on random UNet weights; for information, no threshold")
    try:
        for name, method, steps in (("ddim_75", None, 75), ("dpmpp_2m_75", "dpmpp_2m", 75), ("dpmpp_2m_30", "dpmpp_2m", 30)):
            for c in (model.test_cfg, model.diffusion_ema.test_cfg):
                c.pop("sample_method", None)
                c.update(num_timesteps=steps, **({} if method is None else dict(sample_method=method)))
            torch.manual_seed(1234); np.random.seed(1234)
            res = model.val_step(dict(data, noise=noise))
            mse = (res["pred_imgs"][:, 0].float() - cond.float()).square().flatten(-3).mean(dim=-1)
            psnr = 10.0 * (-torch.log10(mse + 1e-6))
            out[name] = dict(mean=round(float(psnr.mean()), 2), min=round(float(psnr.min()), 2), finite=bool(torch.isfinite(res["code"]).all()))
    finally:
        prior.remove()
    return out


result = dict(what="DPM-Solver++(2M) sampler: the fused step kernel, unconditional sampling rates, the kernel test's error / bound ratios", device=torch.cuda.get_device_name(0))
result["kernel"] = kernel_leg()
if not a.skip_bounds:
    result.update(bounds_leg())
if a.guided:
    result["guided_psnr_db"] = guided_leg()
if not a.skip_sampling:
    result["sampling"] = sampling_leg()
print(json.dumps(result))
