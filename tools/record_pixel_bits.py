"""Output bits of the pixel-major matrix-core kernels (csrc/conv_up3.hip, conv_upconv_i2i.hip, conv_unshuffle.hip over csrc/mma_pixel.h),
recorded on the device (tests/golden/pixel_bits.json): the sha256 of every output buffer of every entry point, sentinels around the view
included, on deterministic inputs at the smallest shapes of tests/test_gpu_upconv3.py, test_gpu_upconv_i2i.py and test_gpu_unshuffle.py.

    python tools/record_pixel_bits.py

The table is recorded from the kernels BEFORE a change, never from the code under test: it stores trainner_amd.build.source_hash() of the
tree it ran on.  tests/test_gpu_pixel_bits.py recomputes every group with group() below and compares.

GROUPS names the groups; a group is one layer shape.  Forward and data gradient run in the three arithmetics (ops.MMA), the weight gradients
(fp32 in every mode) once, and the first x3 and i2i shapes also keep their packed weight images per arithmetic (the folds of common.h)."""
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden", "pixel_bits.json")
ARITHS = (("f32", 0), ("bf16", 1), ("bf16x3", 2))                      # hip.MMA_*
NAN = float("nan")
X3_SHAPES = {"px1": (1, 1, 1), "tile+1": (2, 9, 17), "odd": (2, 17, 23)}          # N, H, W of the LR tensor
I2I_CASES = [(64, 32, 9, 17, True), (1024, 512, 1, 2, False), (128, 64, 5, 7, True), (256, 128, 3, 3, False)]      # Cin, Cout, H, W, bias
UNSHUFFLE_SHAPES = {2: {"px1": (1, 1, 1), "line": (1, 1, 19), "odd": (2, 17, 23), "tile+1": (2, 9, 17)},           # N, Ho, Wo
                    4: {"px1": (1, 1, 1), "line": (1, 1, 19), "odd": (2, 9, 19), "tile+1": (2, 9, 17)}}
GROUPS = ([("x3", nf, cls) for nf in (32, 64) for cls in X3_SHAPES] + [("i2i",) + c for c in I2I_CASES] +
          [("unshuffle", s, nf, cls) for s in (2, 4) for nf in (32, 64) for cls in UNSHUFFLE_SHAPES[s]])
PACKED = (GROUPS[0], ("i2i",) + I2I_CASES[0])                           # the groups that also record their weight images


def group_id(g):
    return "-".join(str(v) for v in g)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _x3(ops, K, M, g, out):
    _, nf, cls = g
    N, H, W = X3_SHAPES[cls]
    x, w, b = K.rnd(N, nf, H, W, seed=4300), K.rnd(nf, nf, 3, 3, seed=4301, lo=-0.1, hi=0.1), K.rnd(nf, seed=4302)
    gr, m, dw0 = K.rnd(N, nf, 3 * H, 3 * W, seed=4303), K.rnd(N, nf, H, W, seed=4304), K.rnd(nf, nf, 3, 3, seed=4305)
    for arith, code in ARITHS:
        ops.MMA = code
        wf, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_UP3_FWD)
        wd, _keep2 = K.pack(ops, w.to(K.DEV), ops.PACK_UP3_DGRAD)
        if g in PACKED:
            out["pack-fwd-" + arith], out["pack-dgrad-" + arith] = sha(wf.t), sha(wd.t)
        yv = M.blank(N, 3 * H, 3 * W, nf, 8, inner=NAN)
        ops.upconv3_fwd(M.win(x, 4), wf, yv, bias=b.to(K.DEV), act=ops.ACT_LRELU, slope=0.2)
        out["fwd-" + arith] = sha(yv.buf)
        for masked in (False, True):
            gxv = M.blank(N, H, W, nf, 8, inner=NAN)
            ops.upconv3_dgrad(M.win(gr, 4), wd, gxv, mask=M.win(m, 8) if masked else None, m_slope=0.2)
            out["dgrad-%s-%s" % ("mask" if masked else "plain", arith)] = sha(gxv.buf)
    dw = dw0.to(K.DEV)
    ops.upconv3_wgrad(M.win(x, 4), M.win(gr, 8), dw, None, alpha=0.75, beta=1.0)
    out["wgrad"] = sha(dw)


def _i2i(ops, K, M, g, out):
    _, cin, cout, H, W, bias = g
    x, w = K.rnd(2, cin, H, W, seed=5100), K.rnd(cout, cin, 3, 3, seed=5101, lo=-0.1, hi=0.1)
    b, gr = K.rnd(cout, seed=5102).to(K.DEV) if bias else None, K.rnd(2, cout, 2 * H, 2 * W, seed=5103)
    for arith, code in ARITHS:
        ops.MMA = code
        wts = ops.UpconvI2IWeights(w.to(K.DEV))
        wts.pack()
        if g in PACKED:
            out["pack-fwd-" + arith], out["pack-dgrad-" + arith] = sha(wts.fwd), sha(wts.dgrad)
        yv, gxv = M.blank(2, 2 * H, 2 * W, cout, 8, inner=NAN), M.blank(2, H, W, cin, 8, inner=NAN)
        ops.upconv_i2i_fwd(M.win(x, 4), wts, yv, bias=b)
        ops.upconv_i2i_dgrad(M.win(gr, 4), wts, gxv)
        out["fwd-" + arith], out["dgrad-" + arith] = sha(yv.buf), sha(gxv.buf)
    dw = torch.full((cout, cin, 3, 3), NAN, device=K.DEV)
    ops.upconv_i2i_wgrad(M.win(x, 4), M.win(gr, 8), dw, None, alpha=1.0, beta=0.0)
    out["wgrad"] = sha(dw)


def _unshuffle(ops, K, M, g, out):
    _, s, nf, cls = g
    N, Ho, Wo = UNSHUFFLE_SHAPES[s][cls]
    x, w, b = K.rnd(N, 3, Ho * s, Wo * s, seed=4100 + s), K.rnd(nf, 3 * s * s, 3, 3, seed=4101 + s, lo=-0.2, hi=0.2), K.rnd(nf, seed=4102)
    gr, dw0, db0 = K.rnd(N, nf, Ho, Wo, seed=4103), K.rnd(nf, 3 * s * s, 3, 3, seed=4104), K.rnd(nf, seed=4105)
    x4 = K.nhwc_buf(x, ctot=4, fill=7.5)
    for arith, code in ARITHS:
        ops.MMA = code
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_UNSHUFFLE_FWD)
        yv = M.blank(N, Ho, Wo, nf, 8, inner=NAN)
        ops.conv_unshuffle(ops.View(x4), wp, yv, s, bias=b.to(K.DEV))
        out["fwd-" + arith] = sha(yv.buf)
    dw, db = dw0.to(K.DEV), db0.to(K.DEV)
    ops.wgrad_unshuffle(M.win(gr, 8), ops.View(x4), dw, db, s, alpha=0.75, beta=1.0)
    out["wgrad-dw"], out["wgrad-db"] = sha(dw), sha(db)


def group(g):
    """{output name: sha256} of one entry of GROUPS, computed on the device by the library under test"""
    import test_gpu_kernels as K
    import test_gpu_membound_kernels as M
    from trainner_amd import ops
    out, prev = {}, ops.MMA
    try:
        {"x3": _x3, "i2i": _i2i, "unshuffle": _unshuffle}[g[0]](ops, K, M, g, out)
        torch.cuda.synchronize()
    finally:
        ops.MMA = prev
    return out


def main():
    from trainner_amd import build, hip
    hip.require_device()
    doc = {"source_hash": build.source_hash(), "bits": {group_id(g): group(g) for g in GROUPS}}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", sum(len(v) for v in doc["bits"].values()), "outputs of", len(GROUPS), "groups from source", doc["source_hash"])


if __name__ == "__main__":
    main()
