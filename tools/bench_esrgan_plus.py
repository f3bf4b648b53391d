"""ESRGAN+ residual paths (network_G `plus: true`): device time of the weight-space fold and unfold launches for RRDBNet-23, and the
whole SR training step with `plus` on against off.  Prints one JSON line and writes it to profiles/esrgan_plus_bench.json:

    python tools/bench_esrgan_plus.py [--window-ms 200] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step] [--no-kernels]

launch      RRDBNet(3, 3, 64, 23, plus=True).  `fold_ms`: ops.DensePlus.fold over the 69 dense blocks (one launch per weight generation,
    i.e. per optimiser step).  `unfold_ms`: one unfold launch over the three blocks of an RRDB, `unfold_net_ms` the 23 of a backward
    back to back, `clear_ms` the fill that clears the shadow gradient once per backward.  HIP events around back-to-back calls, the
    smallest of three windows.  `copy_ms` is `dst.copy_(src)` over `floats`, the conv3..conv5 weights of the 69 blocks, timed in
    alternation with the fold: the fold reads and writes every one of them once, so the copy is its memory floor.
step        bench.py's shape (batch 16, crop 512, RRDBNet-23 + Discriminator_VGG(512) + VGG19 features), inputs resident in device
    memory, `optimize_parameters` + `update_learning_rate` per step.  ms per step with `plus` off (bench.py's own configuration) and
    on, alternating --step-rounds times in this one process (host clock, synchronised): mean, min, max, samples; `on_minus_off_ms`
    beside `off_spread_ms` (max - min of the off samples)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_swa import _stats, time_beside  # noqa: E402


def bench_launch(window_ms, warmup):
    from trainner_amd import ops
    from trainner_amd.models.modules.architectures import RRDBNet_arch
    net = RRDBNet_arch.RRDBNet(3, 3, 64, 23, gaussian_noise=False, plus=True).cuda()
    net._prepare(torch.empty(1, 3, 8, 8, device="cuda"))
    dp = net._plus
    dp.gflat.normal_(0.0, 1e-3)
    n = dp.flat.numel()
    src, dst = torch.randn(n, device="cuda"), torch.empty(n, device="cuda")
    copy = lambda: dst.copy_(src)                                   # noqa: E731
    fold, cp, wins = time_beside(dp.fold, copy, window_ms, warmup)
    one, clear, _ = time_beside(lambda: dp.unfold(33, 3), dp.begin_backward, window_ms, warmup)
    dp.gflat.normal_(0.0, 1e-3)
    whole, _, wins_u = time_beside(lambda: [dp.unfold(3 * b, 3) for b in range(22, -1, -1)], copy, window_ms, warmup)
    net.flat_params().grad.zero_()
    return {"blocks": len(dp.blocks), "floats": n, "fold_ms": round(fold, 4), "fold_windows_ms": [round(x, 4) for x in wins],
            "copy_ms": round(cp, 4), "fold_times_copy": round(fold / cp, 2), "unfold_ms": round(one, 4), "unfold_net_ms": round(whole, 4),
            "unfold_net_windows_ms": [round(x, 4) for x in wins_u], "clear_ms": round(clear, 4),
            "per_step_ms": round(fold + whole + clear, 4)}


def bench_steps(rounds, steps, warmup):
    import bench

    def make(flag):
        yaml = bench.YAML
        if flag:
            bench.YAML = yaml.replace("  type: esrgan\n", "  type: esrgan\n  plus: true\n")
            assert bench.YAML.count("plus: true") == 1
        try:
            m = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0, 1)
        finally:
            bench.YAML = yaml
        lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, m.device)
        return m, {"LR": lr, "HR": hr}

    variants = {"off": make(False), "on": make(True)}
    assert variants["on"][0].netG.plus and not variants["off"][0].netG.plus
    times = {k: [] for k in variants}
    count = {k: 0 for k in variants}

    def run(key, n):
        m, data = variants[key]
        for _ in range(n):
            count[key] += 1
            m.feed_data(data)
            m.optimize_parameters(count[key])
            m.update_learning_rate(count[key], warmup_iter=-1)
        m.get_current_log()

    for key in variants:
        run(key, warmup)
    for _ in range(rounds):
        for key in variants:
            run(key, 1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(key, steps)
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) * 1e3 / steps)
    r = {"steps_per_sample": steps, "clock": "host, synchronised", "ms_per_step": {k: _stats(v) for k, v in times.items()}}
    r["on_minus_off_ms"] = round(r["ms_per_step"]["on"]["mean"] - r["ms_per_step"]["off"]["mean"], 3)
    r["off_spread_ms"] = round(r["ms_per_step"]["off"]["max"] - r["ms_per_step"]["off"]["min"], 3)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=200.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "esrgan_plus_bench.json"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_esrgan_plus", "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["launch"] = bench_launch(args.window_ms, args.warmup)
    if not args.no_step:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["step"] = bench_steps(args.step_rounds, args.steps, min(args.warmup, 3))
    line = json.dumps(out)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
