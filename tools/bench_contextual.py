"""Contextual loss: device time per layer (forward + gradient) at the training step's shapes, the same loss and gradient from the
plain-torch restatement on the same device, and the step's delta with the recipe's two layers.  Prints one JSON line and writes it to
--out (default profiles/contextual_bench.json):

    python tools/bench_contextual.py [--iters 10] [--warmup 2] [--step-rounds 3] [--steps 4] [--no-step] [--out PATH]

layer[name]  a 16 x 3 x 512 x 512 crop: conv3_2 is 16 x 256 x 128^2 pooled to 4096 positions (two index lists), conv4_2 16 x 512 x 64^2.
             ops.cx_layer with and without the gradient view: ms; every launch on its own (the ops' C entry points on the layer's own
             buffers): ms, fp32-equivalent FLOP and the bytes it must move, TFLOP/s, GB/s; tools.make_golden_contextual.cx_forward in fp32
             on the same device through autograd: ms, and the ratio of the two times.
             Agreement at that shape, before any time is reported: the loss and dX of both arithmetics against the fp64 restatement on the
             device (dX under the run's own pattern), by the rule of tests/test_gpu_contextual.py -- f32 within 4 x e32, bf16x3 within
             1.5 x the f32 error + 2e-7 x scale -- with e32 the restatement's own fp32-vs-fp64 deviation on the first E32_IMAGES images run
             as a batch of their own (its gradient scaled by E32_IMAGES / 16: d loss / d X carries 1 / N).
step         the whole G+D step at bench.py's configuration with and without the `contextual` entry (cx_weight 0.5, conv_3_2 and conv_4_2),
             alternating --step-rounds times in one process.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import make_golden_contextual as T  # noqa: E402
from tools.bench_freqsep import _time  # noqa: E402

BATCH, SIZE = 16, 512
LAYERS = (("conv3_2", 256, 4, 4096), ("conv4_2", 512, 8, None))      # name, C, down-sampling, pooled positions
CX = {"cx_type": "contextual", "cx_weight": 0.5, "cx_vgg_layers": {"conv_3_2": 1, "conv_4_2": 1}}
E32_IMAGES = 2
SEED = 8731


def _inputs(C, H, W, keep):
    g = torch.Generator().manual_seed(SEED + C)
    X = torch.rand((BATCH, C, H, W), generator=g) * 2 - 1
    Y = X + (torch.rand((BATCH, C, H, W), generator=g) * 2 - 1)          # the tests' 'corr 1.0' regime
    idx = None if keep is None else tuple(torch.randperm(H * W, generator=g)[:keep].contiguous() for _ in range(2))
    return X.cuda(), Y.cuda(), idx


def _engine(ops, X, Y, idx, grad=True):
    N, C, H, W = X.shape
    xv, yv = (ops.View(t.permute(0, 2, 3, 1).contiguous()) for t in (X, Y))
    ix = iy = inv = None
    if idx is not None:
        ix, iy = (i.to(torch.int32).cuda() for i in idx)
        inv = torch.full((H * W,), -1, dtype=torch.int32)
        inv[idx[0]] = torch.arange(idx[0].numel(), dtype=torch.int32)
        inv = inv.cuda()
    dx = ops.View(torch.empty((N, H, W, C), device="cuda")) if grad else None
    return (lambda: ops.cx_layer(xv, yv, ix, iy, inv, b=T.B, h=T.BAND, dx=dx)), dx


def _restatement32(X, Y, idx):
    didx = (None, None) if idx is None else tuple(i.cuda() for i in idx)

    def run():
        xx = X.detach().requires_grad_(True)
        T.cx_forward(xx if didx[0] is None else T.pool(xx, didx[0]), Y if didx[1] is None else T.pool(Y, didx[1]))["loss"].backward()
        return xx.grad
    return run


def check_agreement(ops, hip, name, X, Y, idx):
    """-> the figures of the agreement check (asserted)."""
    didx = (None, None) if idx is None else tuple(i.cuda() for i in idx)
    sub = slice(0, E32_IMAGES)
    f64, g64 = T.own_gradient(X[sub].double(), Y[sub].double(), *didx)
    f32, g32 = T.own_gradient(X[sub], Y[sub], *didx)
    g64_p32 = T.grad_under_pattern(X[sub], Y[sub], f32["argmax"], f32["argmin"], f32["passes"], *didx)
    e32_loss = T.e32(f32["loss"].cpu(), f64["loss"].cpu())
    e32_dx = T.e32(g32.cpu(), g64_p32.cpu()) * E32_IMAGES / BATCH
    del f64, g64, f32, g32, g64_p32
    torch.cuda.empty_cache()
    runs, saved = {}, ops.FP32_MMA
    try:
        for mode, code in (("f32", hip.MMA_F32), ("bf16x3", hip.MMA_BF16X3)):
            ops.FP32_MMA = code
            fn, dx = _engine(ops, X, Y, idx)
            out = fn()
            assert (out["rowmin"] > 0).all(), "a clamped entry: the bench's pattern is 'all pass'"
            runs[mode] = (out["loss"].double(), dx.buf.permute(0, 3, 1, 2).double(), out["argmax"].long(), out["argmin"].long())
    finally:
        ops.FP32_MMA = saved
    P = runs["f32"][2].shape[1]
    passes = torch.ones((1, P, P), dtype=torch.bool, device="cuda").expand(BATCH, P, P)
    with torch.no_grad():
        loss64 = T.cx_forward(*(t.double() if i is None else T.pool(t.double(), i) for t, i in ((X, didx[0]), (Y, didx[1]))))["loss"]
    torch.cuda.empty_cache()
    err = {}
    for mode, (loss, dx, amax, amin) in runs.items():
        g = T.grad_under_pattern(X, Y, amax, amin, passes, *didx)
        err[mode] = {"loss": abs(loss.item() - loss64.item()), "dx": (dx - g).abs().max().item(), "loss64": loss64.item(),
                     "dx_absmax": g.abs().max().item()}
        del g
        torch.cuda.empty_cache()
    rec = {"e32_loss": e32_loss, "e32_dx": e32_dx, "err": err}
    print("agreement %s: %s" % (name, json.dumps(rec)), flush=True)
    assert err["f32"]["loss"] <= 4 * e32_loss and err["f32"]["dx"] <= 4 * e32_dx, (name, rec)
    assert err["bf16x3"]["loss"] <= 1.5 * err["f32"]["loss"] + 2e-7 * abs(err["bf16x3"]["loss64"]), (name, rec)
    assert err["bf16x3"]["dx"] <= 1.5 * err["f32"]["dx"] + 2e-7 * err["bf16x3"]["dx_absmax"], (name, rec)
    return rec


def bench_stages(ops, hip, N, P, C, HW, iters, warmup):
    """Every launch of a layer on scratch buffers of the layer's size: ms, GFLOP, the GB it must move, TFLOP/s, GB/s."""
    lib, st = hip.load(), hip.stream()
    f = dict(dtype=torch.float32, device="cuda")
    xh = torch.nn.functional.normalize(torch.rand((N, P, C), **f) - 0.5, dim=2)
    yh = torch.nn.functional.normalize(xh + 0.1 * (torch.rand((N, P, C), **f) - 0.5), dim=2)
    ld = (P + 3) // 4 * 4
    D, dxh = torch.empty((N, P, ld), **f), torch.empty((N, P, C), **f)
    rowmin, rowE, colmax, dwin = (torch.empty((N, P), **f) for _ in range(4))
    argmin, argmax = (torch.empty((N, P), dtype=torch.int32, device="cuda") for _ in range(2))
    colpack = torch.empty((N, P), dtype=torch.int64, device="cuda")
    CS, gcoef, loss = torch.empty(N, **f), torch.empty(N, **f), torch.empty((), **f)
    p = lambda t: t.data_ptr()          # noqa: E731
    mat, fea = 4.0 * N * P * P, 4.0 * N * P * C
    stages = (
        ("distance", lambda: lib.tnr_cx_distance(p(xh), p(yh), N, P, C, ops.FP32_MMA, p(D), st), 2.0 * N * P * P * C, 2 * fea + mat),
        ("rows", lambda: lib.tnr_cx_rows(p(D), N, P, T.B, T.BAND, p(rowmin), p(argmin), p(rowE), p(colpack), st), 0.0, 2 * mat),
        ("finalize", lambda: lib.tnr_cx_finalize(p(colpack), N, P, p(colmax), p(argmax), p(CS), p(gcoef), p(loss), st), 0.0, 16.0 * N * P),
        ("grad_rows", lambda: lib.tnr_cx_grad_rows(p(D), p(xh), p(yh), N, P, C, T.BAND, p(rowmin), p(argmin), p(rowE), p(argmax), p(gcoef),
                                                   p(dwin), st), 0.0, 2 * mat + 2 * fea),
        ("grad_gemm", lambda: lib.tnr_cx_grad_gemm(p(D), p(yh), N, P, C, ops.FP32_MMA, p(dxh), st), 2.0 * N * P * P * C, mat + 2 * fea),
    )
    out = {}
    for name, fn, flop, nbytes in stages:          # in order: each stage reads what the one before it left in D
        def run(fn=fn, name=name):
            hip.check(fn(), name)
        ms = _time(run, iters, warmup)
        out[name] = {"ms": round(ms, 4), "gflop": round(flop / 1e9, 2), "gb_min": round(nbytes / 1e9, 4), "tflops": round(flop / ms / 1e9, 2),
                     "gbs": round(nbytes / ms / 1e6, 1)}
    return out


def bench_layers(iters, warmup):
    from trainner_amd import hip, ops
    out = {}
    for name, C, ds, keep in LAYERS:
        H = W = SIZE // ds
        X, Y, idx = _inputs(C, H, W, keep)
        rec = {"shape": [BATCH, C, H, W], "positions": keep or H * W, "agreement": check_agreement(ops, hip, name, X, Y, idx)}
        fn, _ = _engine(ops, X, Y, idx)
        rec["engine_ms"] = round(_time(fn, iters, warmup), 4)
        fwd, _ = _engine(ops, X, Y, idx, grad=False)
        rec["engine_forward_only_ms"] = round(_time(fwd, iters, warmup), 4)
        rec["restatement_fp32_ms"] = round(_time(_restatement32(X, Y, idx), max(2, iters // 3), 1), 4)
        rec["restatement_over_engine"] = round(rec["restatement_fp32_ms"] / rec["engine_ms"], 2)
        rec["stages"] = bench_stages(ops, hip, BATCH, keep or H * W, C, H * W, iters, warmup)
        print("layer %s: %s" % (name, json.dumps({k: v for k, v in rec.items() if k != "agreement"})), flush=True)
        out[name] = rec
        del X, Y
        torch.cuda.empty_cache()
    return out


def bench_step(rounds, steps, warmup):
    import copy
    import bench
    from trainner_amd.models import losses as L
    model = bench.make_model(bench.BATCH_PER_GPU, bench.CROP, 0)
    opt = copy.deepcopy(model.opt)
    opt["train"].update(CX)
    opt["train"]["perceptual_allow_random_init"] = True
    entry = L.get_loss_fn("contextual", CX["cx_weight"], opt=opt, device=model.device)
    base = list(model.generatorlosses.loss_list)
    pos = [i for i, l in enumerate(base) if "fea" in l["name"]][0]
    lists = {"without": base, "with_contextual": base[:pos] + [entry] + base[pos:]}
    lr, hr = bench.synthetic(bench.BATCH_PER_GPU, bench.CROP, 1, model.device)
    times = {k: [] for k in lists}
    step = [0]

    def run(n):
        for _ in range(n):
            step[0] += 1
            model.feed_data({"LR": lr, "HR": hr})
            model.optimize_parameters(step[0])
        model.get_current_log()

    run(warmup)
    for _ in range(rounds):
        for key, ll in lists.items():
            model.generatorlosses.loss_list = ll
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
    return {"batch": bench.BATCH_PER_GPU, "crop": bench.CROP, "steps_per_sample": steps, "loss_names": [l["name"] for l in lists["with_contextual"]],
            "ms_per_step": ms, "added_ms": round(ms["with_contextual"]["mean"] - ms["without"]["mean"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contextual_bench.json"))
    args = ap.parse_args()
    from trainner_amd import hip, ops
    hip.require_device()
    out = {"tool": "bench_contextual", "device": torch.cuda.get_device_name(0), "image": [BATCH, 3, SIZE, SIZE],
           "mma": {hip.MMA_F32: "f32", hip.MMA_BF16X3: "bf16x3"}[ops.FP32_MMA], "config": CX}
    out["layer"] = bench_layers(args.iters, args.warmup)
    if not args.no_step:
        out["step"] = bench_step(args.step_rounds, args.steps, min(args.warmup, 3))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
