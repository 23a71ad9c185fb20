"""Test-view PSNR / SSIM (ssdnerf_image_metrics, csrc/metrics.hip) at the bench batch, 8 scenes x 251 views x 128 x 128: the kernel's time by HIP
events (warm-up, then the mean of --reps calls), the rate of the bytes it has to read, and the float64 restatement of the tests on the CPU per image
pair for comparison.  Prints one JSON line.   usage: python tools/bench_eval_metrics.py [--scenes 8] [--views 251] [--size 128] [--reps 50]"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--views", type=int, default=251)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-pairs", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics: needs the GPU (no HIP device visible)")
    from ssdnerf_amd.metrics import image_metrics
    from _metrics_ref import mse_psnr_ref, ssim_ref
    s = args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    pred = torch.round(torch.rand(args.scenes, args.views, s, s, 3, device="cuda", generator=g) * 255) / 255
    target = (pred + 0.03 * torch.randn(pred.shape, device="cuda", generator=g)).clamp(0, 1)
    for _ in range(args.warmup):
        image_metrics(pred, target)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.reps):
        psnr, ssim = image_metrics(pred, target)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.reps
    nbytes = 2 * pred.numel() * pred.element_size()                     # both images read once; 8 B written per pair
    p, t = pred[0].cpu().numpy(), target[0].cpu().numpy()
    k = min(args.cpu_pairs, args.views)
    t0 = time.perf_counter()
    for i in range(k):
        ssim_ref(p[i], t[i])
        mse_psnr_ref(p[i], t[i])
    cpu_ms = (time.perf_counter() - t0) / k * 1e3
    print(json.dumps(dict(tool="bench_eval_metrics", pairs=pred[..., 0, 0, 0].numel(), h=s, w=s, reps=args.reps,
                          kernel_ms=round(ms, 4), gb_read=round(nbytes / 1e9, 4), effective_gbps=round(nbytes / ms * 1e-6, 1),
                          cpu_restatement_ms_per_pair=round(cpu_ms, 3), cpu_restatement_ms_batch=round(cpu_ms * pred[..., 0, 0, 0].numel(), 1),
                          mean_psnr=round(float(psnr.mean()), 4), mean_ssim=round(float(ssim.mean()), 6))))


if __name__ == "__main__":
    main()
