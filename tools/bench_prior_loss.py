#!/usr/bin/env python
"""tools/bench_prior_loss.py -- the diffusion prior loss on device noise on one MI355X; prints one JSON line and writes it to
``--out`` (profiles/prior_loss.json).

  kernel      the three launches around the UNet at 8 x 18 x 128^2 -- ``ssdnerf_prior_q_sample`` (4 B read + 4 B written per element),
              ``ssdnerf_prior_loss_v`` with its finishing pass (8 B read; 6 B with a bf16 prediction), ``ssdnerf_prior_loss_v_backward`` (8 B read + 8 B
              written; 6 + 6 with bf16, without grad_x0 4 B fewer) -- through the C ABI, and the whole chain around a fixed prediction (q_sample, loss,
              backward to the prediction and to x_0) three ways: the fused autograd functions, the eager tensor expressions on ``_device_noise``, the
              eager expressions on ``_host_noise``.  HIP events over windows alternated in one process, once on ONE set of buffers (cache-resident) and
              once rotating over 8 sets (from HBM); medians with min - max, bytes moved and their share of 8 TB/s.
  train_step  ms per ``DiffusionNeRF.train_step`` of the ``ssdnerf_cars_uncond`` model (the configs' UNet, 8 scenes, fp32; ``--dtype bf16`` for
              autocast) on host and on device noise, windows alternated in ONE process (the step varies by several ms between processes); and, with
              ``--parent-tree DIR`` (a checkout of the parent commit with its library built), the default path of this tree against the parent's, one
              process each, interleaved over ``--rounds`` rounds.
  bounds      the worst error / bound ratios of tests/test_prior_loss_gpu.py's kernel cases, the fused ``forward_train`` against the float64 chain, and the
              gradient errors of the fused and the generic path with a tiny UNet.

``--tree DIR`` imports the package from DIR instead of this file's tree and measures the default train_step alone (what ``--parent-tree`` runs)."""
import argparse, json, os, subprocess, sys, time

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8); ap.add_argument("--windows", type=int, default=7); ap.add_argument("--launches", type=int, default=100)
ap.add_argument("--steps", type=int, default=4, help="train_step calls per window"); ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"]); ap.add_argument("--extra-scene-step", type=int, default=3)
ap.add_argument("--parent-tree", default=None); ap.add_argument("--tree", default=None); ap.add_argument("--out", default=None)
ap.add_argument("--merge", default=None, help="a JSON file of an earlier run whose legs are kept where this run skips them")
ap.add_argument("--skip-kernel", action="store_true"); ap.add_argument("--skip-train-step", action="store_true"); ap.add_argument("--skip-bounds", action="store_true")
a = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(a.tree) if a.tree else HERE
sys.path.insert(0, ROOT)
import numpy as np
import torch
from ssdnerf_amd import _cabi as C

assert torch.cuda.is_available(), "bench_prior_loss.py measures on the GPU"
HBM_PEAK = 8.0e12


def spread(v, digits=3):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], digits), min=round(v[0], digits), max=round(v[-1], digits))


def event_window(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(calls):
        fn(i)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls                                 # us per call


# ------------------------------------------------------------------------------------------------ kernel
def kernel_leg():
    from ssdnerf_amd import diffusion as D
    B, n_per = a.scenes, 18 * 128 * 128
    n = B * n_per
    L = C.lib()
    g = torch.Generator().manual_seed(0)
    sched = D.NoiseSchedule(dict(type="linear"), 1000)
    t = torch.tensor(np.linspace(50, 950, B).astype(np.int64)).cuda()
    ab = sched.signal_noise("cuda")[:, t]
    av, bv = ab[0].contiguous(), ab[1].contiguous()
    a4, b4 = av.reshape(-1, 1, 1, 1), bv.reshape(-1, 1, 1, 1)
    kv = torch.full((B,), 2.0 / n_per / B, device="cuda")
    g_per = torch.full((B,), 1.0 / B, device="cuda")
    partials = torch.empty(int(L.ssdnerf_prior_loss_partials(B, n_per)), device="cuda")
    msd, x0sq = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    u64 = C.ctypes.c_uint64
    nbytes = dict(q_sample=8 * n, loss_fp32=8 * n, loss_bf16=6 * n, backward_fp32=16 * n, backward_bf16=12 * n, backward_fp32_no_grad_x0=12 * n)
    out = dict(elements=n, shape=[B, 18, 128, 128], blocks_per_sample=int(L.ssdnerf_prior_blocks_per_sample(n_per)), bytes_moved=nbytes,
               launches_per_window=a.launches, windows=a.windows,
               chain="q_sample + loss + backward around a fixed prediction (no UNet): fused autograd functions / eager on _device_noise / eager on _host_noise")
    for name, n_sets in (("resident_one_buffer_set", 1), ("rotating_8_buffer_sets", 8)):
        sets = []
        for _ in range(n_sets):
            x0, pred = (torch.randn(B, 18, 128, 128, generator=g).cuda() for _ in range(2))
            sets.append(dict(x0=x0, pred=pred, pred16=pred.to(torch.bfloat16), x_t=torch.empty_like(x0), gp=torch.empty_like(x0), gx=torch.empty_like(x0),
                             gp16=torch.empty_like(x0, dtype=torch.bfloat16)))

        def q_sample(i):
            s = sets[i % n_sets]
            L.ssdnerf_prior_q_sample(C.ptr(s["x0"]), C.ptr(av), C.ptr(bv), C.u32(B), u64(n_per), u64(1234), C.u32(i), C.ptr(s["x_t"]), C.stream())

        def loss(i, key="pred", code=C.F32):
            s = sets[i % n_sets]
            L.ssdnerf_prior_loss_v(C.ptr(s[key]), code, C.ptr(s["x0"]), C.ptr(av), C.ptr(bv), C.u32(B), u64(n_per), u64(1234), C.u32(i), C.ptr(partials),
                                   C.ptr(msd), C.ptr(x0sq), C.stream())

        def backward(i, key="pred", code=C.F32, out_key="gp", gx=True):
            s = sets[i % n_sets]
            L.ssdnerf_prior_loss_v_backward(C.ptr(s[key]), code, C.ptr(s["x0"]), C.ptr(av), C.ptr(bv), C.ptr(kv), C.u32(B), u64(n_per), u64(1234), C.u32(i),
                                            C.ptr(s[out_key]), C.ptr(s["gx"] if gx else None), C.stream())

        def chain(i, mode):
            s = sets[i % n_sets]
            x0, pred = s["x0"].detach().requires_grad_(True), s["pred"].detach().requires_grad_(True)
            if mode == "fused":
                x_t = D._PriorQSample.apply(x0, av, bv, 1234, i)
                per, _ = D._PriorLossV.apply(pred, x0, av, bv, 1234, i)
            else:
                z = D._device_noise(x0, 1234, i) if mode == "device" else D._host_noise(x0)
                x_t = x0 * a4 + z * b4
                per = (pred - (a4 * z - b4 * x0)).square().flatten(1).mean(dim=1)
            torch.autograd.backward([per, x_t], [g_per, s["gx"]])           # (a gradient arrives at x_t too, as the UNet's backward delivers one)

        fns = dict(q_sample=(q_sample, a.launches), loss_fp32=(loss, a.launches), loss_bf16=(lambda i: loss(i, "pred16", C.BF16), a.launches),
                   backward_fp32=(backward, a.launches), backward_bf16=(lambda i: backward(i, "pred16", C.BF16, "gp16"), a.launches),
                   backward_fp32_no_grad_x0=(lambda i: backward(i, gx=False), a.launches),
                   chain_fused=(lambda i: chain(i, "fused"), max(4, a.launches // 5)), chain_eager_device_noise=(lambda i: chain(i, "device"), max(4, a.launches // 5)),
                   chain_eager_host_noise=(lambda i: chain(i, "host"), max(4, a.launches // 20)))
        for fn, _ in fns.values():                                           # warm-up: code objects, the allocator's pools, the pinned ring
            for i in range(3):
                fn(i)
        torch.cuda.synchronize()
        times = {k: [] for k in fns}
        for _ in range(a.windows):                                           # alternated
            for k, (fn, calls) in fns.items():
                times[k].append(event_window(fn, calls))
        # the chains again with the device kept busy in front of them (two 8192^2 fp32 products, several ms), so that the host has queued the whole window
        # before its first launch starts: device time per chain, as behind the UNet's backlog in a training step, instead of the host-bound rate above
        big = torch.randn(8192, 8192, device="cuda")

        def fed_window(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                torch.mm(big, big)
            e0.record()
            for i in range(calls):
                fn(i)
            e1.record(); torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / calls

        for k in ("chain_fused", "chain_eager_device_noise"):
            times[k + "_device_bound"] = []
        for _ in range(a.windows):
            for k in ("chain_fused", "chain_eager_device_noise"):
                times[k + "_device_bound"].append(fed_window(fns[k][0], 16))
        del big
        leg = {k + "_us": spread(v) for k, v in times.items()}
        leg["eager_device_over_fused_device_bound"] = round(leg["chain_eager_device_noise_device_bound_us"]["median"] / leg["chain_fused_device_bound_us"]["median"], 2)
        for k in nbytes:
            rate = nbytes[k] / (leg[k + "_us"]["median"] * 1e-6)
            leg[k + "_tb_per_s"], leg[k + "_share_of_8_tb_per_s"] = round(rate * 1e-12, 3), round(rate / HBM_PEAK, 3)
        leg["eager_device_over_fused"] = round(leg["chain_eager_device_noise_us"]["median"] / leg["chain_fused_us"]["median"], 2)
        leg["eager_host_over_fused"] = round(leg["chain_eager_host_noise_us"]["median"] / leg["chain_fused_us"]["median"], 2)
        out[name] = leg
        del sets
    return out


# ------------------------------------------------------------------------------------------------ train_step
def _train_model():
    import ssdnerf_amd  # noqa: F401
    from ssdnerf_amd import synthetic as S
    from ssdnerf_amd.registry import MODELS
    hw = 128
    m = MODELS.build(dict(
        type="DiffusionNeRF", code_size=(3, 6, 128, 128), code_reshape=(18, 128, 128), code_activation=dict(type="TanhCode", scale=2), grid_size=64,
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
        reg_loss=dict(type="RegLoss", power=2, loss_weight=3e-3), cache_size=a.scenes, autocast_dtype=dict(fp32=None, bf16="bfloat16")[a.dtype],
        train_cfg=dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=a.extra_scene_step, n_inverse_rays=2 ** 12, n_decoder_rays=2 ** 12,
                       loss_coef=0.1 / (hw * hw), optimizer=dict(type="Adam", lr=1e-2, weight_decay=0.))))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for p in m.diffusion.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    m.decoder.load_state_dict(S.make_decoder_params(), strict=False)
    m = m.cuda().train()
    ns = a.scenes
    data = dict(scene_id=list(range(ns)), scene_name=[f"s{i}" for i in range(ns)], cond_imgs=torch.rand(ns, 2, hw, hw, 3, generator=g).cuda(),
                cond_poses=S.spiral_poses()[[30, 150]].cuda()[None].expand(ns, -1, -1, -1).contiguous(),
                cond_intrinsics=S.cars_intrinsics(hw, hw).cuda()[None, None].expand(ns, 2, -1).contiguous())
    opt = dict(diffusion=torch.optim.Adam(m.diffusion.parameters(), lr=1e-5), decoder=torch.optim.Adam(m.decoder.parameters(), lr=1e-3))
    return m, data, opt


def train_step_windows(sources):
    """ms per train_step (host clock around a synchronised window of ``--steps`` calls) per noise source, the windows alternated"""
    m, data, opt = _train_model()
    np.random.seed(0); torch.manual_seed(0)

    def window(source, calls):
        if source == "device":
            m.train_cfg.update(noise_source="device", noise_seed=0)
        else:
            m.train_cfg.pop("noise_source", None)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(calls):
            m.train_step(data, opt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / calls

    for s in sources:
        window(s, 3)                                                         # warm-up (graph capture of the gradient path, the cache, the pinned ring)
    times = {s: [] for s in sources}
    for _ in range(a.windows):
        for s in sources:
            times[s].append(window(s, a.steps))
    return {s + "_ms": spread(v, 2) for s, v in times.items()}


def train_step_leg():
    out = dict(scenes=a.scenes, unet="ssdnerf_cars_uncond (base 128, [1, 2, 2, 4, 4], 2 resblocks, attention at 32 / 16 / 8)", unet_dtype=a.dtype,
               extra_scene_step=a.extra_scene_step, steps_per_window=a.steps, windows=a.windows,
               note="host clock around synchronised windows, alternated in one process; random weights and views: timing only")
    out.update(train_step_windows(["host", "device"]))
    out["device_minus_host_ms"] = round(out["device_ms"]["median"] - out["host_ms"]["median"], 2)
    out["spread_between_windows_ms"] = round(max(out[k]["max"] - out[k]["min"] for k in ("host_ms", "device_ms")), 2)
    if a.parent_tree:
        runs = [("parent_commit", os.path.abspath(a.parent_tree)), ("this_tree", HERE)]
        res = {k: [] for k, _ in runs}
        for _ in range(a.rounds):
            for name, tree in runs:
                cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--scenes", str(a.scenes), "--windows", str(a.windows), "--steps", str(a.steps),
                       "--dtype", a.dtype, "--extra-scene-step", str(a.extra_scene_step)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                if r.returncode != 0:
                    raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-800:]}")
                res[name].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["host_ms"])
                print(f"[bench_prior_loss] {name}: {res[name][-1]}", file=sys.stderr, flush=True)
        out["default_path"] = dict(res, note="host noise, one process per entry, the entries of a round interleaved")
    return out


def bounds_leg():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_prior_loss_gpu as T
    return T.measure()


if a.tree:                                                                   # the default train_step of another checkout, alone
    print(json.dumps(train_step_windows(["host"])))
    sys.exit(0)

result = dict(what="the diffusion prior loss on device noise: the three launches around the UNet and the chain they replace, DiffusionNeRF.train_step on host "
                   "and on device noise, the kernel tests' error / bound ratios", device=torch.cuda.get_device_name(0))


def save():                                                                  # after every leg: a later leg that fails loses nothing
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if a.merge:
    with open(a.merge) as f:
        result.update(json.load(f))
if not a.skip_kernel:
    result["kernel"] = kernel_leg()
    save()
if not a.skip_bounds:
    result.update(bounds_leg())
    save()
if not a.skip_train_step:
    result["train_step"] = train_step_leg()
save()
print(json.dumps(result))
