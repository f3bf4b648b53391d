"""LPIPS validation metric (net-lin / squeeze / v0.1) on one image pair: 2040 x 1356 (a DIV2K-sized image), crop 4, seeded weights.
Prints one JSON line:

    python tools/bench_lpips.py [--iters 20] [--warmup 3] [--threads 16]

ms_per_pair        HIP events around whole distance_u8 calls on device-resident uint8 images (after warm-up; the fp64 [1] result
                   comes back to the host in each call, as in validation)
launches_per_pair  kernel launches of one call (tnr_* entry points: stem, pools, Fire convolutions, heads, finalize)
families           per entry-point family: ms (events around each launch, a separate pass), launches, GFLOP / TFLOP/s for the
                   convolutions, GB and GB/s (and the share of the 8 TB/s HBM peak) for the head
backbone_gflop     2 x MAC of the backbone for the pair (both images), its TFLOP/s over the whole call
cpu_ms             the fp32 / fp64 torch CPU restatement (tools/make_golden_lpips.restate) on --threads threads: the stand-in for
                   the reference's CPU metric (utils/metrics.py:37, use_gpu=False)
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
FAMILIES = ("tnr_lpips_stem", "tnr_maxpool3s2_ceil_fwd", "tnr_conv_forward", "tnr_lpips_head", "tnr_lpips_finalize")


class _Timed:
    """A stand-in for the loaded library: every call of FAMILIES is bracketed by HIP events (or only counted)."""

    def __init__(self, lib, timed):
        self._lib, self._timed, self.log = lib, timed, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("tnr_") or name.endswith(("_bytes", "_dims", "_pack", "_last_error", "version")):
            return fn

        def call(*args):
            fam, flop, nbytes = name, 0.0, 0.0
            if name == "tnr_conv_forward":
                d = args[0]._obj
                taps = {0: 9, 4: 1}.get(d.mode, 0)
                fam = "conv_%s%s" % ({0: "3x3", 4: "1x1"}.get(d.mode, str(d.mode)), "_wino" if d.wq_form == 1 else "")
                flop = 2.0 * d.N * d.Ho * d.Wo * d.Cin * d.Cout * taps
            elif name == "tnr_lpips_head":
                N, H, W, C = args[2:6]
                nbytes = 2.0 * N * H * W * C * 4
            elif name == "tnr_lpips_stem":
                N = args[3]
                ho, wo = (args[4] - 2 * args[7] - 3) // 2 + 1, (args[5] - 2 * args[7] - 3) // 2 + 1
                flop = 2.0 * 2 * N * ho * wo * 64 * 27
                nbytes = 2.0 * N * ho * wo * 64 * 4
            if not self._timed:
                self.log.append((fam, 0.0, flop, nbytes))
                return fn(*args)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self.log.append((fam, (a, b), flop, nbytes))
            return rc
        return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--H", type=int, default=1356)
    ap.add_argument("--W", type=int, default=2040)
    ap.add_argument("--skip-cpu", action="store_true")
    args = ap.parse_args()
    from oracle import detrand
    from tools import make_golden_lpips as G
    from trainner_amd import hip, ops
    from trainner_amd.models.modules.LPIPS.perceptual_loss import PerceptualLoss
    hip.require_device()
    H, W, crop = args.H, args.W, 4
    tv = G.seeded_backbone_state()
    lin = {"lin%d.model.1.weight" % l: detrand.uniform((1, c, 1, 1), 70 + l, 0.0, 0.1) for l, c in enumerate([64, 128, 256, 384, 384, 512, 512])}
    m = PerceptualLoss(allow_random_init=True)
    m.load_torchvision_state(tv)
    m.load_heads(lin)
    a = (detrand.uniform01(H * W * 3, 1) * 256).floor().clamp(0, 255).to(torch.uint8).reshape(1, H, W, 3)
    noise = (detrand.uniform01(H * W * 3, 2) * 21).floor().to(torch.int16).reshape(1, H, W, 3) - 10
    b = (a.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
    ad, bd = a.cuda(), b.cuda()
    for _ in range(args.warmup):
        val = float(m.distance_u8(ad, bd, crop=crop)[0])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.iters):
        m.distance_u8(ad, bd, crop=crop)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.iters

    lib = hip.load()
    fams = {}
    try:
        hip._lib = prof = _Timed(lib, timed=True)
        m.distance_u8(ad, bd, crop=crop)
        torch.cuda.synchronize()
    finally:
        hip._lib = lib
    for fam, ev, flop, nbytes in prof.log:
        f = fams.setdefault(fam, dict(ms=0.0, launches=0, gflop=0.0, gb=0.0))
        f["ms"] += ev[0].elapsed_time(ev[1])
        f["launches"] += 1
        f["gflop"] += flop / 1e9
        f["gb"] += nbytes / 1e9
    for f in fams.values():
        if f["gflop"]:
            f["tflops"] = round(f["gflop"] / f["ms"], 3)
        if f["gb"]:
            f["gbs"] = round(f["gb"] / (f["ms"] / 1e3), 1)
            f["hbm_peak_frac"] = round(f["gbs"] / HBM_PEAK_GBS, 3)
        f["ms"], f["gflop"], f["gb"] = round(f["ms"], 4), round(f["gflop"], 3), round(f["gb"], 4)
    backbone_gflop = sum(f["gflop"] for k, f in fams.items() if k.startswith("conv_") or k == "tnr_lpips_stem")
    out = dict(metric="lpips_squeeze_v0.1", H=H, W=W, crop=crop, mma={0: "f32", 1: "bf16", 2: "bf16x3"}[ops.FP32_MMA],
               ms_per_pair=round(ms, 3), launches_per_pair=len(prof.log), backbone_gflop=round(backbone_gflop, 2),
               backbone_tflops_over_call=round(backbone_gflop / ms, 3), value=val, families=fams)
    if not args.skip_cpu:
        torch.set_num_threads(args.threads)
        for dt, key in ((torch.float32, "cpu_ms_fp32"), (torch.float64, "cpu_ms_fp64")):
            t0 = time.perf_counter()
            v, _ = G.restate(tv, lin, a[0], b[0], crop=crop, dtype=dt)
            out[key] = round((time.perf_counter() - t0) * 1e3, 1)
            out[key.replace("ms", "value")] = v
        out["cpu_threads"] = args.threads
    print(json.dumps(out))


if __name__ == "__main__":
    main()
