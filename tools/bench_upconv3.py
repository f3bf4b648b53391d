"""RRDBNet's x3 up-conv layer: device time of its three launches (csrc/conv_up3.hip) beside the x2 layer's present launches at the same
LR size, timed in the same process, and the whole x3 SR training step beside the x4 step.  Prints one JSON line:

    python tools/bench_upconv3.py [--window-ms 300] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step] [--no-kernels]

launch      batch 16, LR 128 x 128, nf 64, in bf16x3 and bf16.  HIP events around back-to-back calls, the smallest of three windows, the
    x3 launch and its x2 counterpart alternating (engine.ConvOp of one layer each: forward = tnr_upconv3_fwd | TNR_CONV_3x3_UP2, data
    gradient = tnr_upconv3_dgrad | the folded four-tap stride-2 launch, weight gradient = tnr_upconv3_wgrad + tnr_bias_grad | the x2 path
    ops.upconv_plan names).  `TFLOPs_exec` counts the taps a launch executes per LR pixel and channel pair (x3: 25; x2: 36 for the 3x3
    forward over 4 HR pixels, 16 for the folded gradients), `TFLOPs_alg` the layer written out in the HR domain (x3: 81, x2: 36).
step        bench.py's trunk (batch 16, LR 128, RRDBNet-23 + Discriminator_VGG + VGG19 features): the x4 recipe (HR 512) and the x3 recipe
    (HR 384), alternating --step-rounds times in this one process (host clock, synchronised): mean, min, max, samples."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def bench_launches(window_ms, warmup):
    from bench_swa import time_beside
    from trainner_amd import engine, hip, ops
    from trainner_amd.models.modules.architectures import block as B
    N, nf, T = 16, 64, 128
    dev = torch.device("cuda")
    mod = B.Conv2dHIP(nf, nf, 3, 1).to(dev)
    for p in mod.parameters():
        p.grad = torch.zeros_like(p)
    packer = ops.WeightPacker(dev)
    layers = {3: engine.ConvOp(mod, packer, ups=3), 2: engine.ConvOp(mod, packer, ups=True)}
    packer.run()
    x, gx, mask = (ops.View(torch.randn(N, T, T, nf, device=dev)) for _ in range(3))
    hr = {s: (ops.View(ops.new_act(N, s * T, s * T, nf, dev)), ops.View(torch.randn(N, s * T, s * T, nf, device=dev))) for s in (2, 3)}
    px = float(N * T * T * nf * nf * 2)
    taps = {"fwd": {3: (25, 81), 2: (36, 36)}, "dgrad": {3: (25, 81), 2: (16, 36)}, "wgrad": {3: (25, 81), 2: (16, 36)}}
    out = {"lr": [N, T, T, nf], "x2_plan": list(ops.upconv_plan(x)[0])}
    for arith, code in (("bf16x3", hip.MMA_BF16X3), ("bf16", hip.MMA_BF16)):
        prev = ops.MMA, ops.FP32_MMA
        ops.MMA = ops.FP32_MMA = code
        try:
            r = {}
            for name in ("fwd", "dgrad", "wgrad"):
                def run(s):
                    u, (y, g) = layers[s], hr[s]
                    if name == "fwd":
                        return lambda: u.fwd_up2(x, y, act=ops.ACT_LRELU, slope=0.2)
                    if name == "dgrad":
                        return lambda: u.dgrad_up2(g, gx, mask=mask, m_slope=0.2)
                    return lambda: u.wgrad(x, g)
                ms3, ms2, wins = time_beside(run(3), run(2), window_ms, warmup)
                r[name] = {"x3_ms": round(ms3, 4), "x3_windows_ms": [round(v, 4) for v in wins], "x2_ms": round(ms2, 4)}
                for s, ms in ((3, ms3), (2, ms2)):
                    r[name]["x%d_TFLOPs_exec" % s] = round(px * taps[name][s][0] / ms / 1e9, 1)
                    r[name]["x%d_TFLOPs_alg" % s] = round(px * taps[name][s][1] / ms / 1e9, 1)
            out[arith] = r
        finally:
            ops.MMA, ops.FP32_MMA = prev
    return out


def bench_steps(rounds, steps, warmup):
    import bench
    from bench_swa import _stats

    def make(scale):
        yaml = bench.YAML
        bench.YAML = yaml.replace("\nscale: 4\n", "\nscale: %d\n" % scale)
        assert bench.YAML.count("\nscale: %d\n" % scale) == 1
        try:
            m = bench.make_model(bench.BATCH_PER_GPU, bench.CROP * scale // 4, 0, 1)
        finally:
            bench.YAML = yaml
        _, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP * scale // 4, 1, m.device)
        return m, {"LR": torch.nn.functional.avg_pool2d(hr, scale), "HR": hr}

    variants = {"x4": make(4), "x3": make(3)}
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
    return {"steps_per_sample": steps, "clock": "host, synchronised", "lr": [bench.BATCH_PER_GPU, bench.CROP // 4, bench.CROP // 4],
            "ms_per_step": {k: _stats(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip
    hip.require_device()
    out = {"tool": "bench_upconv3", "device": torch.cuda.get_device_name(0)}
    if not args.no_kernels:
        out["launch"] = bench_launches(args.window_ms, args.warmup)
    if not args.no_step:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out["step"] = bench_steps(args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
