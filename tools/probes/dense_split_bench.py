"""Block-level price of the split dense block (ops.dense_block, TNR_DENSE_SPLIT) at the training shape 16 x 128 x 128, TNR_MMA=bf16x3,
forward and gradient shape: the five-stage sweep, the four-stage sweep, the Winograd last stage, their sum -- and the split form as
ops.dense_block issues it (two launches back to back).  Break-even for the four-stage launch = five-stage - Winograd.
    TNR_MMA=bf16x3 python tools/probes/dense_split_bench.py"""
import os
import sys

os.environ.setdefault("TNR_MMA", "bf16x3")
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from trainner_amd import hip, ops  # noqa: E402
from tools.microbench_conv import timeit  # noqa: E402
from tools.probes.sweep_check import block  # noqa: E402


def main():
    assert ops.MMA == hip.MMA_BF16X3
    ops.DENSE_SPLIT = True
    N, H, W = 16, 128, 128
    print("%-5s %10s %10s %10s %10s %10s %12s" % ("shape", "sweep5 us", "sweep4 us", "wino5 us", "4 + wino", "split us", "break-even"))
    for grad_shape in (False, True):
        _, _, st = block(N, H, W, seed=5, grad_shape=grad_shape)("layers")
        assert ops.dense_split_applies(st)
        last = {k: v for k, v in st[4].items() if k != "fresh_from"}
        rows = []
        for rep in range(2):          # (twice: the clock may still be ramping at a process's first launches)
            t5 = timeit(lambda: ops.conv_chain(st))
            t4 = timeit(lambda: ops.conv_chain(st[:4]))
            tw = timeit(lambda: ops.conv(wino=True, **last))
            ts = timeit(lambda: ops.dense_block(st))
            rows.append((t5, t4, tw, ts))
        t5, t4, tw, ts = (min(r[i] for r in rows) for i in range(4))
        print("%-5s %10.1f %10.1f %10.1f %10.1f %10.1f %12.1f" % ("grad" if grad_shape else "fwd", t5, t4, tw, t4 + tw, ts, t5 - tw), flush=True)
    print("chain error flag:", ops.chain_error_flag())


if __name__ == "__main__":
    main()
