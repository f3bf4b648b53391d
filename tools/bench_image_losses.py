"""HFEN, image-gradient and total-variation losses: device time of each loss alone and of the whole training step.  Prints one JSON
line:

    python tools/bench_image_losses.py [--iters 100] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step]

loss[shape][name]  HIP events around forward + backward of the built loss function (fp32 NCHW operands, as `fake_H` / `real_H` are):
    ms              mean over --iters calls after warm-up, the smallest of three such batches (the module path: autograd, the
                    output allocations and the scalar `weight * f` ops included, so small shapes show the launch overhead)
    gb_min          bytes the algorithm must move.  grad / tv: x (and y) read once in the forward and once in the backward, the
                    gradient written once.  hfen: the same plus the rho'(e) map written by the forward and read by the backward
    gbs, hbm_share  gb_min / ms, as a share of the 6.3 TB/s achievable HBM bandwidth
    gflop           hfen only: 225 FMAs x 2 per response, forward and backward
    lds_reads       hfen only: LDS dwords read, 15 rows x 18 per 4 responses, forward and backward
    ms_at_*_bound   the time each resource would take at its peak (HBM 6.3 TB/s, vector ALU 157 TFLOP/s fp32, LDS 128 B / clk / CU
                    x 256 CUs x 2.4 GHz); `bound` names the largest: the resource that binds
launches[name]     forward and backward entry point each alone on preallocated tensors at 16 x 3 x 512 x 512: ms, bytes it must move,
                   its largest floor and which resource that is, and ms / floor
step               the whole G+D step at bench.py's configuration (model built by bench.make_model) without and with the recipe's
                   three terms (hfen-l1 1e-6, grad-4d-l1 4e-1, tv-l1 1e-5), alternating --step-rounds times in this one process
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS, VALU_PEAK_GFLOPS, LDS_PEAK_GBS = 6300.0, 157300.0, 128 * 256 * 2.4
NAMES = ("hfen-l1", "grad-4d-l1", "tv-l1")
RECIPE = (("hfen-l1", 1e-6), ("tv-l1", 1e-5), ("grad-4d-l1", 4e-1))


def counted(name, N, C, H, W):
    """-> (bytes that must move, FMA-counted flop, LDS bytes read) of one forward + backward."""
    plane = N * C * H * W * 4.0
    if name.startswith("hfen"):
        return 2 * plane + plane + plane + plane, 2 * 2.0 * 225 * N * C * H * W, 2 * (15 * 18 / 4.0) * N * C * H * W * 4.0
    if name.startswith("grad"):
        return 2 * plane + 2 * plane + plane, 0.0, 0.0
    return plane + plane + plane, 0.0, 0.0


def bench_loss(name, N, C, H, W, iters, warmup):
    from trainner_amd.models import losses
    f = losses.get_loss_fn(name, 1, device="cuda")["function"]
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(N, C, H, W, generator=g).cuda()
    sr = (hr + 0.05 * torch.randn(N, C, H, W, generator=g).cuda()).requires_grad_(True)
    call = (lambda: f(sr)) if "tv" in name else (lambda: f(sr, hr))

    def once():
        sr.grad = None
        call().backward()

    ms = _time(once, iters, warmup)
    nbytes, flop, lds = counted(name, N, C, H, W)
    bounds = {"hbm": nbytes / HBM_ACHIEVABLE_GBS / 1e6, "valu": flop / VALU_PEAK_GFLOPS / 1e6, "lds": lds / LDS_PEAK_GBS / 1e6}
    gbs = nbytes / ms / 1e6
    return {"ms": round(ms, 4), "gb_min": round(nbytes / 1e9, 4), "gbs": round(gbs, 1), "hbm_share_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4),
            "gflop": round(flop / 1e9, 3), "lds_gb_read": round(lds / 1e9, 3), "ms_at_hbm_bound": round(bounds["hbm"], 4),
            "ms_at_valu_bound": round(bounds["valu"], 4), "ms_at_lds_bound": round(bounds["lds"], 4), "bound": max(bounds, key=bounds.get)}


def _time(fn, iters, warmup, repeats=3):
    """Minimum over `repeats` of the mean ms per call over `iters` back-to-back calls (HIP events), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    best = float("inf")
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) / iters)
    return best


def bench_launches(name, N, C, H, W, iters, warmup):
    """Each entry point alone, through the ops wrappers on preallocated tensors (no autograd, no allocation): ms, the bytes it must
    move, and its floors."""
    from trainner_amd import ops
    from trainner_amd.models import losses
    f = losses.get_loss_fn(name, 1, device="cuda")["function"]
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(N, C, H, W, generator=g).cuda()
    sr = hr + 0.05 * torch.randn(N, C, H, W, generator=g).cuda()
    out, gx = torch.empty((), device="cuda"), torch.empty_like(sr)
    plane, n = N * C * H * W * 4.0, N * C * H * W
    if name.startswith("hfen"):
        dmap = torch.empty_like(sr)
        calls = {"fwd": (lambda: ops.filter_loss_fwd(sr, hr, 0, f.taps, 15, f.criterion.crit, 1.0, out, dmap), 3 * plane),
                 "bwd": (lambda: ops.filter_loss_bwd(dmap, 0, f.taps, 15, 1.0, None, gx), 2 * plane)}
        flop, lds = 2.0 * 225 * n, (15 * 18 / 4.0) * n * 4.0
    else:
        y = None if "tv" in name else hr
        crit = ops.CRIT_L1
        calls = {"fwd": (lambda: ops.fd_loss_fwd(sr, y, 0, f.dirs, crit, 1.0, out), plane * (1 if y is None else 2)),
                 "bwd": (lambda: ops.fd_loss_bwd(sr, y, 0, f.dirs, crit, 1.0, None, gx), plane * (2 if y is None else 3))}
        flop = lds = 0.0
    res = {}
    for tag, (fn, nbytes) in calls.items():
        ms = _time(fn, iters, warmup)
        bounds = {"hbm": nbytes / HBM_ACHIEVABLE_GBS / 1e6, "valu": flop / VALU_PEAK_GFLOPS / 1e6, "lds": lds / LDS_PEAK_GBS / 1e6}
        floor = max(bounds.values())
        res[tag] = {"ms": round(ms, 4), "gb_min": round(nbytes / 1e9, 4), "gbs": round(nbytes / ms / 1e6, 1),
                    "floor_ms": round(floor, 4), "floor": max(bounds, key=bounds.get), "times_floor": round(ms / floor, 2)}
    return res


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.models import losses
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    gl = model.generatorlosses
    built = {n: losses.get_loss_fn(n, w, device=model.device) for n, w in RECIPE}
    plain = (list(gl.loss_list), list(gl.precise_loss_list))
    terms = ([gl.loss_list[0], built["hfen-l1"], built["tv-l1"]] + gl.loss_list[1:], [built["grad-4d-l1"]] + gl.precise_loss_list)
    times = {"plain": [], "recipe_terms": []}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, (regular, precise) in (("plain", plain), ("recipe_terms", terms)):
            gl.loss_list, gl.precise_loss_list = regular, precise
            run(1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(steps)
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) / steps)
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps,
            "ms_per_step": {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                                "samples": [round(x, 3) for x in v]} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_image_losses", "device": torch.cuda.get_device_name(0), "loss": {}}
    for shape in ((16, 3, 512, 512), (16, 3, 128, 128)):
        out["loss"]["x".join(map(str, shape))] = {n: bench_loss(n, *shape, args.iters, args.warmup) for n in NAMES}
    out["launches"] = {n: bench_launches(n, 16, 3, 512, 512, args.iters, args.warmup) for n in NAMES}
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
