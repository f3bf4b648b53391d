"""Style loss and multi-layer perceptual taps: device time of each Gram launch, of the whole feature term, and of the training step with
the step record's loss configuration against the single-conv5_4 configuration.  Prints one JSON line:

    python tools/bench_style_loss.py [--iters 20] [--warmup 3] [--step-rounds 3] [--steps 4] [--no-step]

gram[tap]   tnr_gram_fwd (both launches: tiles + reduction) and tnr_gram_bwd alone, through the ops wrappers on preallocated buffers, at
            the shape the tap has for a 16 x 3 x 512 x 512 image: ms, the bytes the launch must move from HBM (forward: X once + G;
            backward: X once + dX once), fp32-equivalent FLOP (forward: the computed blocks of the upper triangle), GB/s, TFLOP/s and the
            share of the bound DESIGN.md section 14 names for that C (HBM_GBS for C = 64 / 128, MATRIX_TFLOPS above)
term        PerceptualLoss forward + backward on one image pair: the single conv5_4 tap, and STEP config (five taps, two Gram terms)
step        the whole G+D step at bench.py's configuration with either feature term, alternating --step-rounds times in one process
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.bench_freqsep import _time  # noqa: E402

BATCH, SIZE = 16, 512
TAPS = (("conv1_2", 64, 1), ("relu2_2", 128, 2), ("conv3_4", 256, 4), ("relu4_2", 512, 8), ("conv5_4", 512, 16))      # name, C, down-sampling
STYLE = {"style_weight": 30.0, "perceptual_opt": {"perceptual_layers": {"conv1_2": 0.1, "conv3_4": 1, "conv5_4": 1},
                                                  "style_layers": {"relu2_2": 1, "relu4_2": 1}}}
HBM_GBS = 8000.0            # peak HBM3E bandwidth of the part
MATRIX_TFLOPS = 219.0       # sustained fp32-equivalent rate of the training step in bf16x3 (DESIGN.md section 3.1 / bench.py step_tflops)


def bench_gram(iters, warmup):
    from trainner_amd import ops
    out = {}
    for name, C, ds in TAPS:
        H = W = SIZE // ds
        x = ops.View(torch.rand(BATCH, H, W, C, device="cuda") - 0.5)
        G = torch.empty(BATCH, C, C, device="cuda")
        S = torch.rand(BATCH, C, C, device="cuda") - 0.5
        dx = ops.View(torch.empty(BATCH, H, W, C, device="cuda"))
        scale = 1.0 / (C * H * W)
        xb = 4.0 * BATCH * H * W * C
        nb = C // 64
        T = nb * (nb + 1) // 2
        f_flop = 2.0 * 4096 * (T - nb / 4.0) * BATCH * H * W
        b_flop = 2.0 * BATCH * H * W * C * C
        rec = {"shape": [BATCH, H, W, C]}
        for tag, fn, nbytes, flop in (("fwd", lambda: ops.gram_fwd(x, scale, G), xb + 4.0 * BATCH * C * C, f_flop),
                                      ("bwd", lambda: ops.gram_bwd(x, S, scale, dx), 2 * xb, b_flop)):
            ms = _time(fn, iters, warmup)
            gbs, tfl = nbytes / ms / 1e6, flop / ms / 1e9
            bound = "hbm" if C <= 128 else "matrix"
            rec[tag] = {"ms": round(ms, 4), "gb_min": round(nbytes / 1e9, 4), "gflop": round(flop / 1e9, 2), "gbs": round(gbs, 1),
                        "tflops": round(tfl, 2), "bound": bound,
                        "share_of_bound": round(gbs / HBM_GBS if bound == "hbm" else tfl / MATRIX_TFLOPS, 3)}
        out[name] = rec
        del x, dx
        torch.cuda.empty_cache()
    return out


def _fea_entry(model, extra):
    """A `fea` loss entry built like GeneratorLoss builds it, for model.opt with `extra` merged into its train block; the VGG weights are
    the model's own feature network's."""
    from trainner_amd.models import losses as L
    opt = copy.deepcopy(model.opt)
    opt["train"].update(extra)
    entry = L.get_loss_fn("fea-vgg19-l1", 1, opt=opt, device=model.device)
    old = [l for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]["function"].network
    entry["function"].network.load_state_dict(old.state_dict())
    return entry


def bench_term(model, entries, iters, warmup):
    import bench
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    sr = torch.rand_like(hr)
    out = {}
    for key, entry in entries.items():
        f = entry["function"]

        def run():
            x = sr.detach().requires_grad_(True)
            p, s = f(x, hr)
            (p if s is None else p + s).backward()
        out[key] = round(_time(run, iters, warmup), 3)
    out["added_ms"] = round(out["style_multi"] - out["conv5_4"], 3)
    return out


def bench_step(model, entries, rounds, steps, warmup):
    import bench
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    idx = [i for i, l in enumerate(model.generatorlosses.loss_list) if "fea" in l["name"]][0]
    times = {k: [] for k in entries}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, entry in entries.items():
            model.generatorlosses.loss_list[idx] = entry
            run(1)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run(steps)
            b.record()
            torch.cuda.synchronize()
            times[key].append(a.elapsed_time(b) / steps)
    ms = {k: {"mean": round(sum(v) / len(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "samples": [round(x, 3) for x in v]}
          for k, v in times.items()}
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps, "ms_per_step": ms,
            "added_ms": round(ms["style_multi"]["mean"] - ms["conv5_4"]["mean"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    args = ap.parse_args()
    from trainner_amd import hip, ops
    hip.require_device()
    out = {"tool": "bench_style_loss", "device": torch.cuda.get_device_name(0), "image": [BATCH, 3, SIZE, SIZE],
           "mma": {hip.MMA_F32: "f32", hip.MMA_BF16X3: "bf16x3"}[ops.FP32_MMA], "config": STYLE,
           "bounds": {"hbm_gbs": HBM_GBS, "matrix_tflops": MATRIX_TFLOPS}}
    out["gram"] = bench_gram(args.iters, args.warmup)
    if not args.no_step:
        import bench
        model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
        entries = {"conv5_4": _fea_entry(model, {}), "style_multi": _fea_entry(model, STYLE)}
        out["term"] = bench_term(model, entries, max(3, args.iters // 4), 2)
        out["step"] = bench_step(model, entries, args.step_rounds, args.steps, min(args.warmup, 3))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
