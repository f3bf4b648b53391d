"""The i2i up-conv layer (csrc/conv_upconv_i2i.hip): device time of tnr_upconv_i2i_fwd / _dgrad / _wgrad at the decoders' sizes (batch 16, 256 x 256
images), bf16x3; HIP events, the smallest of three windows.  Prints one JSON line.  TNR_HIP_LIB selects the library (A/B against another build)."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    from bench_swa import _window
    from trainner_amd import hip, ops
    hip.require_device()
    ops.MMA = ops.FP32_MMA = hip.MMA_BF16X3
    out = {"tool": "bench_upconv_i2i", "lib": os.environ.get("TNR_HIP_LIB", "in-tree")}
    # ResNet-9 decoder (256 -> 128 at 64 x 64, 128 -> 64 at 128 x 128) and the U-Net's weight-bound end (1024 -> 512 at 2 x 2)
    for cin, cout, T in ((256, 128, 64), (128, 64, 128), (1024, 512, 2)):
        N = 16
        x, gx = (ops.View(torch.randn(N, T, T, cin, device="cuda")) for _ in range(2))
        y, g = (ops.View(torch.randn(N, 2 * T, 2 * T, cout, device="cuda")) for _ in range(2))
        w = (torch.rand(cout, cin, 3, 3, device="cuda") - 0.5) * 0.2
        wts = ops.UpconvI2IWeights(w)
        wts.pack()
        dw = torch.zeros_like(w)
        for name, fn in (("fwd", lambda: ops.upconv_i2i_fwd(x, wts, y)), ("dgrad", lambda: ops.upconv_i2i_dgrad(g, wts, gx)),
                         ("wgrad", lambda: ops.upconv_i2i_wgrad(x, g, dw, None, alpha=1.0, beta=0.0))):
            for _ in range(10):
                fn()
            iters = max(20, int(200.0 / max(_window(fn, 20), 1e-4)))
            wins = [_window(fn, iters) for _ in range(3)]
            out["%dto%d_%d_%s" % (cin, cout, T, name)] = {"ms": round(min(wins), 4), "windows_ms": [round(v, 4) for v in wins]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
