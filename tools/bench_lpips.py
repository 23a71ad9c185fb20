"""LPIPS (ssdnerf_amd/lpips.py: the VGG16 trunk on csrc/conv_igemm.hip's fp32-class convolutions + csrc/lpips.hip) at the bench batch, 8 scenes x 251
views of 128 x 128.  By HIP events, after a warm-up of every shape, the mean of --reps repetitions of
  * the whole call ``LPIPSVGG(pred, target)`` (63 chunks of 32 pairs),
  * the eager restatement on the same GPU, alternated with it in this process: fp32 ``conv2d`` in channels_last through the library plus the
    elementwise ops, chunked the same way,
  * one full chunk taken apart: the input kernel, the thirteen convolutions, the ReLU passes and the five tap passes each on their own, with the bytes
    the three new kernels move and their share of 8 TB/s;
FLOP from the shapes (2 * 9 * Cin * Cout * H * W per layer, Cin = 3 on the first).  It also repeats the accuracy figures of tests/test_lpips_gpu.py at
64 x 64: the worst relative error against the float64 restatement next to that of the TF32 emulation (the tolerance).  Prints one JSON line
(kept as profiles/lpips.json).   usage: python tools/bench_lpips.py [--scenes 8] [--views 251] [--size 128] [--reps 10]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _timed(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--views", type=int, default=251)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import lpips as L, synthetic as S, unet_fast as UF
    from _lpips_ref import SCALE, SHIFT, lpips_ref, make_pairs, rel_err
    sd = S.make_lpips_params(1)
    net = L.LPIPSVGG.from_state_dict(sd)
    s, chunk = args.size, args.chunk
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.round(torch.rand(args.scenes, args.views, s, s, 3, device="cuda", generator=g) * 255) / 255
    target = (pred + 0.03 * torch.randn(pred.shape, device="cuda", generator=g)).clamp(0, 1)
    pairs = args.scenes * args.views

    # ---- the eager restatement: same chunks, fp32, channels_last
    convs = [(sd[f"features.{i}.weight"].cuda().contiguous(memory_format=torch.channels_last), sd[f"features.{i}.bias"].cuda()) for i in L.FEATURE_IDX]
    lins = [sd[f"lin{k}.model.1.weight"].cuda().reshape(1, -1, 1, 1) for k in range(5)]
    shift, scale = torch.tensor(SHIFT, device="cuda")[None, :, None, None], torch.tensor(SCALE, device="cuda")[None, :, None, None]

    def eager(a, b):
        out = []
        a, b = a.reshape(-1, s, s, 3), b.reshape(-1, s, s, 3)
        for lo in range(0, a.shape[0], chunk):
            n = min(chunk, a.shape[0] - lo)
            x = torch.cat([a[lo:lo + n], b[lo:lo + n]]).permute(0, 3, 1, 2)            # (2n, 3, h, w) as a channels_last view
            x = ((2 * x - 1) - shift) / scale
            acc = 0
            for i, (w, bias) in enumerate(convs):
                x = F.relu(F.conv2d(x, w, bias, 1, 1))
                if i in L.TAPS:
                    f = x / (x.square().sum(1, keepdim=True).sqrt() + 1e-10)
                    acc = acc + ((f[:n] - f[n:]).square() * lins[L.TAPS.index(i)]).sum(1).mean((1, 2))
                    if i != L.TAPS[-1]:
                        x = F.max_pool2d(x, 2, 2)
            out.append(acc)
        return torch.cat(out)

    with torch.no_grad():
        hip = net(pred, target, chunk=chunk)                                              # warm-up of every shape, both paths, last chunk included
        ref = eager(pred, target)
        torch.cuda.synchronize()
        agree = float(((hip.flatten() - ref).abs() / ref.abs()).max())
        hip_ms, eager_ms = [], []
        for _ in range(args.reps):                                                          # alternated: one call of each per round
            hip_ms.append(_timed(lambda: net(pred, target, chunk=chunk), 1, warmup=0))
            eager_ms.append(_timed(lambda: eager(pred, target), 1, warmup=0))
        call_ms, eager_call_ms = sum(hip_ms) / len(hip_ms), sum(eager_ms) / len(eager_ms)

        # ---- one chunk taken apart
        n = min(chunk, pairs)
        B = 2 * n
        a, b = pred.reshape(-1, s, s, 3)[:n].contiguous(), target.reshape(-1, s, s, 3)[:n].contiguous()
        prm, lin_dev = net._params(pred.device)
        ws = UF.shared_splitk_ws("cuda")
        reps = max(args.reps, 10)
        t = dict(input=_timed(lambda: L.lpips_input(a, b), reps), conv=0.0, relu_pool=0.0, lpips_layer=0.0)
        nbytes = dict(input=B * s * s * (12 + 32), relu_pool=0, lpips_layer=0)
        per_layer = []
        x, H, W = L.lpips_input(a, b), s, s
        split_in = False
        for i, ((cin, cout), (w_hi, w_lo, bias)) in enumerate(zip(L.CHANNELS, prm)):
            if split_in:
                conv = lambda: UF.conv2d_nhwc_f32x2_presplit(x, w_hi, w_lo, bias, splitk_ws=ws)          # noqa: E731
            else:
                conv = lambda: UF.conv2d_nhwc_f32x2(x, w_hi, w_lo, bias=bias, splitk_ws=ws)              # noqa: E731
            ms = _timed(conv, reps)
            raw = conv()
            t["conv"] += ms
            flop = 2 * 9 * (3 if i == 0 else cin) * cout * H * W * B
            per_layer.append(dict(conv=i + 1, cin=cin, cout=cout, h=H, w=W, presplit=bool(split_in), ms=round(ms, 4), tflops=round(flop / ms * 1e-9, 1)))
            nxt = L.CHANNELS[i + 1] if i + 1 < len(L.CHANNELS) else None
            if i in L.TAPS:
                last = i == L.TAPS[-1]
                split_in = (not last) and bool(UF.presplit_supported(torch.empty((B, cout, H // 2, W // 2), device="cuda").contiguous(
                    memory_format=torch.channels_last), nxt[1], 3))
                acc = torch.zeros(n, device="cuda")
                ms = _timed(lambda: L.lpips_layer(raw, lin_dev[L.TAPS.index(i)], acc, pool_out=not last, split_out=split_in), reps)
                t["lpips_layer"] += ms
                moved = B * H * W * cout * 4 + (0 if last else B * (H // 2) * (W // 2) * cout * 4)
                nbytes["lpips_layer"] += moved
                per_layer[-1].update(after="lpips_layer", after_ms=round(ms, 4), after_gbps=round(moved / ms * 1e-6, 1))
                if not last:
                    x = L.lpips_layer(raw, lin_dev[L.TAPS.index(i)], acc, split_out=split_in)
                    H, W = H // 2, W // 2
            else:
                split_in = bool(UF.presplit_supported(raw, nxt[1], 3))
                ms = _timed(lambda: L.relu_pool_nhwc(raw, split_out=split_in), reps)
                t["relu_pool"] += ms
                moved = 2 * B * H * W * cout * 4
                nbytes["relu_pool"] += moved
                per_layer[-1].update(after="relu_pool", after_ms=round(ms, 4), after_gbps=round(moved / ms * 1e-6, 1))
                x = L.relu_pool_nhwc(raw, split_out=split_in)
        torch.cuda.synchronize()

    # ---- accuracy at 64 x 64 (the figures of tests/test_lpips_gpu.py)
    pa, pb = make_pairs(64, 64)
    exact = lpips_ref(pa, pb, sd)
    tf32 = float(rel_err(lpips_ref(pa, pb, sd, mode="tf32"), exact).max())
    measured = float(rel_err(net(pa.cuda(), pb.cuda()), exact).max())

    flop_img = L.flops_per_image(s, s)
    new_ms = t["input"] + t["relu_pool"] + t["lpips_layer"]
    new_bytes = sum(nbytes.values())
    print(json.dumps(dict(
        tool="bench_lpips", pairs=pairs, h=s, w=s, chunk=chunk, reps=args.reps,
        call_ms=round(call_ms, 2), call_ms_min=round(min(hip_ms), 2), call_ms_max=round(max(hip_ms), 2),
        eager_call_ms=round(eager_call_ms, 2), eager_call_ms_min=round(min(eager_ms), 2), eager_call_ms_max=round(max(eager_ms), 2),
        hip_no_slower_than_eager=bool(call_ms <= eager_call_ms), hip_vs_eager_max_rel_diff=agree,
        gflop_per_image=round(flop_img / 1e9, 3), tflop_per_call=round(flop_img * 2 * pairs / 1e12, 2),
        call_tflops=round(flop_img * 2 * pairs / call_ms * 1e-9, 1), eager_tflops=round(flop_img * 2 * pairs / eager_call_ms * 1e-9, 1),
        chunk_ms=dict(input=round(t["input"], 4), conv=round(t["conv"], 4), relu_pool=round(t["relu_pool"], 4), lpips_layer=round(t["lpips_layer"], 4),
                      sum=round(new_ms + t["conv"], 4)),
        chunk_conv_tflops=round(flop_img * B / t["conv"] * 1e-9, 1),
        new_kernels=dict(bytes_per_chunk=new_bytes, ms_per_chunk=round(new_ms, 4), gbps=round(new_bytes / new_ms * 1e-6, 1),
                         share_of_8tbps=round(new_bytes / new_ms * 1e-6 / 8000, 3),
                         by_kernel={k: dict(bytes=nbytes[k], ms=round(t[k], 4), gbps=round(nbytes[k] / t[k] * 1e-6, 1)) for k in nbytes}),
        layers=per_layer,
        accuracy_64x64=dict(worst_rel_err_vs_fp64=measured, tf32_emulation_worst_rel_err=tf32, within_tolerance=bool(measured <= tf32)),
        mean_lpips=float(hip.mean()))))


if __name__ == "__main__":
    main()
