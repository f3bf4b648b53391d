"""SSIM / MS-SSIM training losses: device time of the loss alone and of the whole training step.  Prints one JSON line:

    python tools/bench_ssim_loss.py [--iters 20] [--warmup 3] [--step-rounds 3] [--steps 4] [--no-step]

loss[shape][type]  HIP events around forward + backward of the module (fp32 NCHW operands, as `fake_H` / `real_H` are):
    ms              mean over --iters calls after warm-up
    launches        tnr_* kernel entry points per call (the two scalar torch ops of `weight * (1 - f)` are not part of it)
    gb_min          bytes the algorithm must move: per level X and Y read once in the forward, once in the backward, gX written
                    (and, between levels, the pooled X and Y written and the coarse gX read and added: one read + one write)
    gbs, hbm_share  gb_min / ms, as a share of the 6.3 TB/s achievable and the 8 TB/s peak HBM bandwidth
    gflop, bound    counted fp32 FMAs x 2 of the filters (forward: 5 maps x 2K per position with the tile halo; backward: the same on
                    the double halo plus 3 maps x 2K of the transposed window) and which of HBM (at 6.3 TB/s) or the vector ALU
                    (157 TFLOP/s fp32 peak) would take longer at its peak: the resource that binds
step               the whole G+D step at bench.py's configuration (model built by bench.make_model), `ssim_weight` absent / `ssim` /
                   `ms-ssim`, alternating --step-rounds times in this one process: mean and min..max ms per step of each
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_ACHIEVABLE_GBS, HBM_PEAK_GBS, VALU_PEAK_GFLOPS = 6300.0, 8000.0, 157300.0
ENTRY = ("ssim_fwd", "ssim_bwd", "avgpool2_pad_fwd", "avgpool2_pad_bwd", "msssim_combine")
LAUNCHES = {"ssim_fwd": 2, "ssim_bwd": 1, "avgpool2_pad_fwd": 1, "avgpool2_pad_bwd": 1, "msssim_combine": 1}


def counted(kind, N, C, H, W, shave=4):
    """-> (bytes that must move, FMA-counted flop) of one forward + backward."""
    from trainner_amd.models.modules.ssim import msssim_levels
    h, w = H - 2 * shave, W - 2 * shave
    levels = msssim_levels(h, w) if kind == "ms-ssim" else ((h, w, 11, 1.5),)
    nbytes = flop = 0.0
    for i, (lh, lw, k, _) in enumerate(levels):
        full = (H * W if i == 0 else lh * lw) * N * C * 4.0
        region = lh * lw * N * C * 4.0
        nbytes += 2 * region * 2 + full                      # X, Y read in the forward and in the backward; gX written
        if i > 0:
            nbytes += 2 * region + 2 * region                # pooled X, Y written; this level's gX read and added into the finer one
            nbytes += region * 4                             # ... which is read and written again (4 fine pixels per coarse one)
        oh, ow = lh - k + 1, lw - k + 1
        fwd = 5 * (k * (1 + (32 + k - 1) / 32.0) + 0) * oh * ow          # row pass on the 32-row tile's halo rows + column pass
        bwd = 5 * k * ((16 + 2 * k - 2) * (32 + k - 1) + (16 + k - 1) * (32 + k - 1)) / 512.0 * lh * lw \
            + 3 * k * ((16 + k - 1) * 32 + 512) / 512.0 * lh * lw
        flop += 2.0 * N * C * (fwd + bwd)
    return nbytes, flop


def bench_loss(kind, N, C, H, W, iters, warmup):
    from trainner_amd import ops
    from trainner_amd.models.modules.ssim import MS_SSIM, SSIM
    kw = dict(window_size=11, window_sigma=1.5, size_average=True, data_range=1., channels=C)
    mod = SSIM(**kw) if kind == "ssim" else MS_SSIM(normalize="relu", **kw)
    g = torch.Generator().manual_seed(7)
    hr = torch.rand(N, C, H, W, generator=g).cuda()
    sr = (hr + 0.05 * torch.randn(N, C, H, W, generator=g).cuda()).requires_grad_(True)
    calls, real = [], {n: getattr(ops, n) for n in ENTRY}
    for n in ENTRY:
        setattr(ops, n, lambda *a, _n=n, **k: (calls.append(_n), real[_n](*a, **k))[1])
    try:
        mod(sr, hr).backward()
    finally:
        for n in ENTRY:
            setattr(ops, n, real[n])
    launches = sum(LAUNCHES[n] for n in calls)
    for _ in range(warmup):
        sr.grad = None
        mod(sr, hr).backward()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        sr.grad = None
        mod(sr, hr).backward()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / iters
    nbytes, flop = counted(kind, N, C, H, W)
    gbs = nbytes / ms / 1e6
    t_hbm, t_alu = nbytes / HBM_ACHIEVABLE_GBS / 1e6, flop / VALU_PEAK_GFLOPS / 1e6
    return {"ms": round(ms, 4), "launches": launches, "gb_min": round(nbytes / 1e9, 4), "gbs": round(gbs, 1),
            "hbm_share_achievable": round(gbs / HBM_ACHIEVABLE_GBS, 4), "hbm_share_peak": round(gbs / HBM_PEAK_GBS, 4),
            "gflop": round(flop / 1e9, 3), "ms_at_hbm_bound": round(t_hbm, 4), "ms_at_valu_bound": round(t_alu, 4),
            "bound": "hbm" if t_hbm >= t_alu else "valu"}


def bench_step(rounds, steps, warmup):
    import bench
    from trainner_amd.models import losses
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    entries = {None: []}
    for kind in ("ssim", "ms-ssim"):
        entries[kind] = [losses.get_loss_fn(kind, 1, opt=model.opt["train"], device=model.device)]
    times = {str(k): [] for k in entries}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for kind, lst in entries.items():
            model.generatorlosses.precise_loss_list = lst
            run(1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(steps)
            b.record()
            torch.cuda.synchronize()
            times[str(kind)].append(a.elapsed_time(b) / steps)
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps,
            "ms_per_step": {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                                "samples": [round(x, 3) for x in v]} for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_ssim_loss", "device": torch.cuda.get_device_name(0), "loss": {}}
    for shape in ((16, 3, 512, 512), (16, 3, 128, 128)):
        out["loss"]["x".join(map(str, shape))] = {k: bench_loss(k, *shape, args.iters, args.warmup) for k in ("ssim", "ms-ssim")}
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, args.warmup)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
