"""Characterisation table of the dense-block dispatch in trainner_amd/ops.py, recorded on the CPU (tests/golden/dense_plan.json).

For every combination of block kind x arithmetic x process switches x calibrated choice x buckets-in-flight x on-device it records what
ops.dense_block and ops.conv_chain reach -- `sweep<n>` / `chain<n>` (the tnr_conv_sweep / tnr_conv_chain entries and their stage count),
`direct` / `wino` (ops.conv with wino=False / True; `direct*5`: five in a row) -- the ops.COUNTERS deltas of each call, and the answers of dense_split_applies,
dense_block_form_applies and dense_blocks_overlap_collectives.  tests/test_cpu_dense_plan.py replays every row on the code under test.

The table is recorded from the ops.py of the commit BEFORE a change to the dispatch, never from the code under test:
    git show <commit>:trainner_amd/ops.py > /tmp/ops_at_commit.py
    python tools/record_dense_plan.py --ops /tmp/ops_at_commit.py --commit <commit>
The file is loaded as a module of the trainner_amd package beside the tree's own ops and driven UNEDITED.  Stand-ins: hip.load returns a
fake library (its *_bytes entries return fixed sizes -- 0 from tnr_conv_sweep_image_bytes for the "unsweepable" kind -- and every other
entry records its name and succeeds), hip.stream returns 0, ops.conv is a recorder, ops._cus returns 4, and "on the device" is a
CPU tensor subclass whose is_cuda answers True (every version of the dispatch asks the stages' buffers exactly that).
"""
import argparse
import contextlib
import importlib.util
import itertools
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from trainner_amd import hip  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "dense_plan.json")
NF, GC, CUS = 64, 32, 4
KINDS = ("train", "grad", "chain3", "ineligible", "big_grid", "unsweepable")
MMAS = {"f32": hip.MMA_F32, "bf16": hip.MMA_BF16, "bf16x3": hip.MMA_BF16X3}
DEFAULTS = dict(CONV_CHAIN=True, CONV_SWEEP=True, CHAIN_X3=True, AMP_SWEEP=True, SWEEP_AUTO=True, DENSE_SPLIT=True, CHAIN_WITH_COLLECTIVES=False)
# every switch alone against the defaults, then the pairs that interact (buckets-in-flight is a dimension of its own below)
FLIPS = [()] + [(k,) for k in DEFAULTS] + [("CONV_SWEEP", "AMP_SWEEP"), ("CHAIN_WITH_COLLECTIVES", "CONV_CHAIN")]
CHOICES = (None, "sweep", "layers")
STATES = list(itertools.product(CHOICES, (False, True), (False, True)))      # (choice, buckets in flight, on device)


class _OnDevice(torch.Tensor):
    __torch_function__ = torch._C._disabled_torch_function_impl          # (a plain tensor in every other respect, and as fast)
    is_cuda = property(lambda self: True)


class _Owner:
    gen = 1


class FakeLib:
    """Every tnr_* entry: *_bytes return a fixed size, the rest record (name, second argument) and return 0."""

    def __init__(self):
        self.calls, self.sweepable = [], True

    def __getattr__(self, name):
        def entry(*args):
            if name == "tnr_conv_sweep_image_bytes":
                return 4096 if self.sweepable else 0
            if name.endswith("_bytes"):
                return 1024
            self.calls.append((name, args))
            return 0
        return entry


def load_ops(path=None):
    """The tree's ops module, or the ops.py at `path` as trainner_amd.<its file name>."""
    if path is None:
        from trainner_amd import ops
        return ops
    name = "trainner_amd." + os.path.splitext(os.path.basename(path))[0]
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def stages(ops, kind, on_device):
    """A residual dense block (nf 64, gc 32) over an 8 x 32 grid and its variations; views over CPU tensors."""
    H, W = (24, 64) if kind == "big_grid" else (8, 32)          # 3 x 2 tiles > CUS
    owner = _Owner()

    def t(*shape):
        x = torch.zeros(shape)
        return x.as_subclass(_OnDevice) if on_device else x

    buf, out, maskbuf = t(1, H, W, NF + 4 * GC), t(1, H, W, NF), t(1, H, W, NF + 4 * GC)

    def wp(cin, cout):
        return ops.Packed(torch.zeros(8), cout, cin, ops.PACK_FWD, owner)

    st = []
    for k in range(4):
        cin = NF + GC * k
        if kind == "grad":
            st.append(dict(x=ops.View(buf, 0, cin), wp=wp(cin, GC), y=ops.View(buf, cin, GC), fresh_from=(cin - GC if k else None),
                           mask=ops.View(maskbuf, NF + (3 - k) * GC, GC), m_lo=0, m_hi=GC, m_slope=0.2))
        else:
            st.append(dict(x=ops.View(buf, 0, cin), wp=wp(cin, GC), y=ops.View(buf, cin, GC), bias=None, act=ops.ACT_LRELU, slope=0.2,
                           fresh_from=(cin - GC if k else None)))
    st.append(dict(x=ops.View(buf), wp=wp(NF + 4 * GC, NF), y=ops.View(out), fresh_from=NF + 3 * GC, r1=ops.View(buf, 0, NF), beta1=0.2))
    if kind == "chain3":
        st = st[:3]
    if kind == "ineligible":          # y.C % 32 != 0 in the second stage
        st[1] = dict(st[1], y=ops.View(buf, NF + GC, 16), wp=wp(NF + GC, 16))
    return st


@contextlib.contextmanager
def stand_ins(ops, lib):
    saved_hip = (hip.load, hip.stream)
    names = list(DEFAULTS) + ["MMA", "FP32_MMA", "COLLECTIVES_IN_FLIGHT", "PROFILE", "conv", "_cus", "_FAULT"]
    saved = {k: getattr(ops, k) for k in names}
    state = dict(ops.SWEEP_AUTO_STATE)
    counters = dict(ops.COUNTERS)
    hip.load, hip.stream = (lambda *a, **k: lib), (lambda: 0)
    ops.conv = lambda *a, **k: lib.calls.append(("conv", k.get("wino")))
    ops._cus = lambda dev: CUS
    ops.PROFILE, ops._FAULT = None, None
    try:
        yield
    finally:
        hip.load, hip.stream = saved_hip
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.SWEEP_AUTO_STATE.clear()
        ops.SWEEP_AUTO_STATE.update(state)
        ops.COUNTERS.update(counters)
        for key in [k for k in ops.WS.bufs if isinstance(k, tuple) and k[0] == "chain" and k[1] == "cpu"]:
            del ops.WS.bufs[key], ops._chain_epoch[key]


def run_of(entry, n):
    return entry if n == 1 else "%s*%d" % (entry, n)


def _reached(ops, lib, fn, st):
    """-> "<entries reached>/<one_launch delta>,<per_layer delta>" of fn(st)."""
    del lib.calls[:]
    before = dict(ops.COUNTERS)
    fn(st)
    seq = []
    for name, args in lib.calls:
        if name == "conv":
            seq.append("wino" if args else "direct")
        elif name in ("tnr_conv_sweep", "tnr_conv_chain"):
            seq.append(name[9:] + str(args[1] if name == "tnr_conv_sweep" else args[2]))
    seq = [run_of(e, len(list(g))) for e, g in itertools.groupby(seq)]
    return "%s/%d,%d" % ("+".join(seq), ops.COUNTERS["one_launch_next_to_collectives"] - before["one_launch_next_to_collectives"],
                         ops.COUNTERS["per_layer_next_to_collectives"] - before["per_layer_next_to_collectives"])


def configure(ops, lib, kind, mma, flips, state):
    """Set the live module to one row's state -> the row's stages."""
    choice, in_flight, on_device = state
    for k, v in DEFAULTS.items():
        setattr(ops, k, (not v) if k in flips else v)
    ops.MMA = MMAS[mma]
    ops.FP32_MMA = hip.MMA_BF16X3 if mma == "bf16" else MMAS[mma]        # (bf16 operands: an amp region of a bf16x3 process)
    ops.SWEEP_AUTO_STATE["choice"] = choice
    ops.COLLECTIVES_IN_FLIGHT = in_flight
    lib.sweepable = kind != "unsweepable"
    return stages(ops, kind, on_device)


def row(ops, lib, st):
    return "%s;%s;%d%d%d" % (_reached(ops, lib, ops.dense_block, st), _reached(ops, lib, ops.conv_chain, st),
                             bool(ops.dense_split_applies(st)), bool(ops.dense_block_form_applies(st)), bool(ops.dense_blocks_overlap_collectives()))


def flips_id(flips):
    return ",".join(flips) or "defaults"


def table(ops):
    """{kind: {mma: {flipped switches: [row per STATES entry]}}}"""
    lib = FakeLib()
    with stand_ins(ops, lib):
        return {kind: {mma: {flips_id(f): [row(ops, lib, configure(ops, lib, kind, mma, f, s)) for s in STATES] for f in FLIPS} for mma in MMAS}
                for kind in KINDS}


def host_cost(ops, calls):
    """Host microseconds per ops.dense_block and per ops.conv_chain call on the training-shaped block (defaults, bf16x3, on the device):
    the form decision, the descriptors and the cache look-ups, with the fake library's entries returning at once."""
    import time
    lib, out = FakeLib(), {}
    with stand_ins(ops, lib):
        st = configure(ops, lib, "train", "bf16x3", (), (None, False, True))
        for name in ("dense_block", "conv_chain"):
            fn = getattr(ops, name)
            fn(st)
            del lib.calls[:]
            best = []
            for _ in range(5):          # (the minimum of five runs of CALLS: the host is shared)
                t0 = time.perf_counter()
                for _ in range(calls):
                    fn(st)
                best.append(1e6 * (time.perf_counter() - t0) / calls)
                del lib.calls[:]
            out[name] = min(best)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--ops", help="the ops.py to drive (a copy of a commit's trainner_amd/ops.py; default: the tree's)")
    ap.add_argument("--commit", help="the commit that file is from (written into the table)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--host-cost", type=int, metavar="CALLS", help="instead of recording: time CALLS launches of the training-shaped block on the host")
    a = ap.parse_args()
    if a.host_cost:
        print(json.dumps({"ops": a.ops or "trainner_amd/ops.py", "calls": a.host_cost,
                          "us_per_call": {k: round(v, 2) for k, v in host_cost(load_ops(a.ops), a.host_cost).items()}}))
        return
    assert a.ops and a.commit, "recording needs --ops and --commit: the table comes from a commit's ops.py, never from the code under test"
    doc = {"recorded_at_commit": a.commit, "states": [list(s) for s in STATES], "rows": table(load_ops(a.ops))}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote", a.out, sum(len(r) for k in doc["rows"].values() for m in k.values() for r in m.values()), "rows")


if __name__ == "__main__":
    main()
