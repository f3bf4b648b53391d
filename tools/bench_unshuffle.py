"""The pixel-unshuffle generator input: device time of the unshuffle layer's forward and weight-gradient launches beside a device copy
of the bytes each must move, and the whole SR training step of an x2 `use_unshuffle` configuration beside the x4 step at the same trunk
size.  Prints one JSON line:

    python tools/bench_unshuffle.py [--window-ms 300] [--warmup 10] [--step-rounds 3] [--steps 4] [--no-step] [--no-kernels]

launch      batch 16, nf 64: s = 2 over a 256 x 256 image and s = 4 over a 512 x 512 image, both onto a 128 x 128 trunk.  HIP events
    around back-to-back calls, the smallest of three windows, per arithmetic of ops.MMA (bf16x3, f32, bf16) for the forward;
    `floor_ms` is `dst.copy_(src)` over half the bytes the launch must move (a copy reads and writes each of its bytes: the same
    traffic), timed in alternation -- forward: the image (16 B per pixel) read + the output written; weight gradient: the image and
    the gradient read.  `times_floor` the ratio, `TFLOPs` from 2 x 27 s^2 x nf per output pixel.
step        bench.py's shape (batch 16, HR crop 512, RRDBNet-23 + Discriminator_VGG(512) + VGG19 features): the x4 recipe (LR 128) and
    the x2 recipe with use_unshuffle (LR 256, unshuffle 2: the same 128 x 128 trunk), alternating --step-rounds times in this one
    process (host clock, synchronised): mean, min, max, samples."""
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
    from trainner_amd import hip, ops
    out = {}
    N, nf, T = 16, 64, 128
    for s in (2, 4):
        H = T * s
        img = torch.rand(N, H, H, 4, device="cuda")
        w = (torch.rand(nf, 3 * s * s, 3, 3, device="cuda") - 0.5) * 0.2
        b = torch.rand(nf, device="cuda")
        packer = ops.WeightPacker(torch.device("cuda"))
        wp = packer.get(packer.add(w, ops.PACK_UNSHUFFLE_FWD))
        packer.run()
        y, g = ops.View(ops.new_act(N, T, T, nf, "cuda")), ops.View(torch.randn(N, T, T, nf, device="cuda"))
        dw, db = torch.zeros_like(w), torch.zeros_like(b)
        flops = 2.0 * 27 * s * s * nf * N * T * T
        r = {"image": [N, H, H], "trunk": [N, T, T, nf]}
        for name, fn, nbytes in [("fwd_" + m, (lambda: ops.conv_unshuffle(ops.View(img), wp, y, s, bias=b)), img.numel() * 4 + y.buf.numel() * 4)
                                 for m in ("bf16x3", "f32", "bf16")] + \
                                [("wgrad", (lambda: ops.wgrad_unshuffle(g, ops.View(img), dw, db, s, alpha=1.0, beta=0.0)), img.numel() * 4 + g.buf.numel() * 4)]:
            prev = ops.MMA
            ops.MMA = {"fwd_f32": hip.MMA_F32, "fwd_bf16": hip.MMA_BF16}.get(name, hip.MMA_BF16X3)
            src, dst = torch.empty(nbytes // 8, device="cuda"), torch.empty(nbytes // 8, device="cuda")
            try:
                ms, floor, wins = time_beside(fn, lambda: dst.copy_(src), window_ms, warmup)
            finally:
                ops.MMA = prev
            r[name] = {"ms": round(ms, 4), "windows_ms": [round(x, 4) for x in wins], "bytes": nbytes, "floor_ms": round(floor, 4),
                       "times_floor": round(ms / floor, 2), "TFLOPs": round(flops / ms / 1e9, 1)}
        out["s%d" % s] = r
    return out


def bench_steps(rounds, steps, warmup):
    import bench
    from bench_swa import _stats

    def make(unshuffle):
        yaml = bench.YAML
        if unshuffle:
            bench.YAML = yaml.replace("\nscale: 4\n", "\nscale: 2\nuse_unshuffle: true\n").replace("network_G:\n  type: esrgan\n", "network_G:\n  type: esrgan\n  scale: 4\n")
            assert bench.YAML.count("use_unshuffle") == 1 and bench.YAML.count("  scale: 4\n") == 1
        try:
            m = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0, 1)
        finally:
            bench.YAML = yaml
        _, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, m.device)
        return m, {"LR": torch.nn.functional.avg_pool2d(hr, 2 if unshuffle else 4), "HR": hr}

    variants = {"x4": make(False), "x2_unshuffle": make(True)}
    assert variants["x2_unshuffle"][0].unshuffle is not None and variants["x4"][0].unshuffle is None
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
    r["x2_minus_x4_ms"] = round(r["ms_per_step"]["x2_unshuffle"]["mean"] - r["ms_per_step"]["x4"]["mean"], 3)
    return r


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
    out = {"tool": "bench_unshuffle", "device": torch.cuda.get_device_name(0)}
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
