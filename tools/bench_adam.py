"""The optimizer step of stage-1 fitting, ``torch.optim.Adam`` per scene (the default path) against ``HIPAdam`` + ``step_all`` (csrc/adam.hip):

  * the optimizer alone at the stage-1 shape -- 8 leaves of 3 x 6 x 128 x 128 through 8 optimizers, and one (8, 3, 6, 128, 128) leaf through
    one -- per step by HIP events and by the host clock over a synchronised window, windows alternated between the two paths; the bytes the
    step moves (4 reads + 3 writes per element) and their share of 8 TB/s for the HIP kernel (timed as bare launches through the C ABI:
    at this size the Python around a launch takes longer than the kernel);
  * ``MultiSceneNeRF.train_step`` with the stage-1 model dict, 8 scenes, ``extra_scene_step=15``, 2^12 rays: ms per call with each optimizer,
    calls alternated;
  * the largest |difference| of the cached codes between the two optimizers after the train_step of tests/test_adam_gpu.py (the tolerance
    that test asserts 8 x of), between two runs of the same optimizer, and between the first such call of the process and a later one
    with torch's Adam on both sides.

Prints one JSON line.   usage: python tools/bench_adam.py [--steps 1000] [--windows 7] [--calls 5] > profiles/adam.json"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
LEAF = (3, 6, 128, 128)


def _window(fn, steps):
    """(HIP-event ms per step, host wall ms per step) of ``steps`` calls between two synchronisations"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps, (time.perf_counter() - t0) * 1e3 / steps


def _spread(vals):
    return dict(median=round(statistics.median(vals), 5), min=round(min(vals), 5), max=round(max(vals), 5))


def _alternate(fns, steps, windows, warmup):
    """{name: {event_ms, wall_ms}}: ``windows`` windows per path, taken in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    got = {name: ([], []) for name in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            ev, wall = _window(fn, steps)
            got[name][0].append(ev)
            got[name][1].append(wall)
    return {name: dict(event_ms=_spread(ev), wall_ms=_spread(wall)) for name, (ev, wall) in got.items()}


def _optimizer_alone(shapes, steps, windows, warmup):
    from ssdnerf_amd import _cabi as C
    from ssdnerf_amd.optim import HIPAdam, step_all
    g = torch.Generator(device="cuda").manual_seed(0)

    def leaves():
        ls = [(torch.randn(s, device="cuda", generator=g) * 0.1).requires_grad_(True) for s in shapes]
        for l in ls:
            l.grad = torch.randn(l.shape, device="cuda", generator=g) * 1e-2
        return ls
    ref_leaves, hip_leaves = leaves(), leaves()
    ref_opts = [torch.optim.Adam([l], lr=1e-2, weight_decay=0.) for l in ref_leaves]
    hip_opts = [HIPAdam([l], lr=1e-2, weight_decay=0.) for l in hip_leaves]

    def torch_loop():
        for o in ref_opts:
            o.step()
    step_all(hip_opts)                                                   # creates the moments the bare launches below reuse
    # the launch alone: the same table straight through the C ABI, without the per-optimizer Python around it (its event time is the kernel's)
    table = (C.AdamTensor * len(hip_leaves))()
    for e, l, o in zip(table, hip_leaves, hip_opts):
        st = o.state[l]
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = l.data_ptr(), l.grad.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
        e.numel, e.step_size, e.bc2_sqrt, e.weight_decay = l.numel(), 1e-2, 1.0, 0.0
    lib, n, stream = C.lib(), len(hip_leaves), C.stream()

    def bare():
        lib.ssdnerf_adam_step_multi(table, n, 0.9, 0.999, 1e-8, stream)
    C.check(lib.ssdnerf_adam_step_multi(table, n, 0.9, 0.999, 1e-8, stream), "adam_step_multi")
    out = _alternate({"torch_adam": torch_loop, "hip_adam": lambda: step_all(hip_opts), "hip_launch_alone": bare}, steps, windows, warmup)
    numel = sum(l.numel() for l in hip_leaves)
    nbytes = 7 * 4 * numel
    out.update(tensors=len(shapes), elements=numel, mbytes=round(nbytes / 1e6, 2), min_ms_at_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3, 5),
               kernel_share_of_8tbps=round(nbytes / HBM_BYTES_PER_S * 1e3 / out["hip_launch_alone"]["event_ms"]["median"], 3))
    return out


def _train_step_ms(calls, rounds, scenes=8):
    import test_tv_loss_gpu as TV
    from ssdnerf_amd.models import _torch_factory
    imgs, poses, intr = TV._views(list(range(51, 51 + scenes)), [30, 150])
    data = dict(scene_id=list(range(scenes)), scene_name=[f"s{i}" for i in range(scenes)], cond_imgs=imgs, cond_poses=poses, cond_intrinsics=intr)
    runs = {}
    for kind in ("Adam", "HIPAdam"):
        cfg = dict(dt_gamma_scale=0.5, density_thresh=0.1, extra_scene_step=15, n_inverse_rays=2 ** 12, n_decoder_rays=2 ** 12,
                   loss_coef=0.1 / (64 * 64), optimizer=dict(type=kind, lr=1e-2, weight_decay=0.))
        m = TV._stage1_model(train_cfg=cfg).train()
        cls, kw = _torch_factory(torch.optim, dict(type=kind, lr=1e-3))
        opt = dict(decoder=cls(m.decoder.parameters(), **kw))
        runs[kind] = (lambda m=m, opt=opt: m.train_step(data, opt))
    torch.manual_seed(0)
    got = _alternate(runs, calls, rounds, warmup=2)
    return dict(scenes=scenes, extra_scene_step=15, rays=2 ** 12, optimizer_steps_per_call=16 * scenes + 1, calls_per_window=calls, windows=rounds,
                adam_ms=got["Adam"]["wall_ms"], hipadam_ms=got["HIPAdam"]["wall_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adam: needs the GPU (no HIP device visible)")
    from ssdnerf_amd import optim
    import test_adam_gpu as TA
    res = dict(tool="bench_adam", device=torch.cuda.get_device_name(0), steps_per_window=args.steps, windows=args.windows, capacity=optim.CAPACITY)
    res["eight_leaves"] = _optimizer_alone([LEAF] * 8, args.steps, args.windows, args.warmup)
    res["one_leaf"] = _optimizer_alone([(8,) + LEAF], args.steps, args.windows, args.warmup)
    res["train_step"] = _train_step_ms(args.calls, args.rounds)
    first, _, _, _ = TA.train_step_codes("Adam")                           # the first train_step of this shape in a process: see first_call_diff
    hip, _, launched, _ = TA.train_step_codes("HIPAdam")
    ref, _, _, _ = TA.train_step_codes("Adam")
    ref2, _, _, _ = TA.train_step_codes("Adam")
    hip2, _, _, _ = TA.train_step_codes("HIPAdam")
    res["train_step_code_max_abs_diff"] = float((hip - ref).abs().max())
    res["train_step_code_repeat_diff"] = dict(adam=float((ref - ref2).abs().max()), hipadam=float((hip - hip2).abs().max()))
    res["train_step_code_first_call_diff"] = float((first - ref).abs().max())   # torch's Adam on both sides: the process's first call against a later one
    res["train_step_code_abs_max"] = float(ref.abs().max())
    res["train_step_launches"] = launched
    print(json.dumps(res))


if __name__ == "__main__":
    main()
