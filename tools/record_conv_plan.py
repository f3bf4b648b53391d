"""Characterisation table of the single-convolution dispatch (trainner_amd/ops.py + engine.py), recorded on the CPU (tests/golden/conv_plan.json).

For every combination of layer x direction, epilogue, arithmetic, process switches, the caller's `wino` and the library's three late answers it
records what ConvOp.fwd / ConvOp.dgrad / ConvOp.fwd_shuffle2 / a bare ops.conv reach: the library entries in order (thin_pack, thin, im2col,
wq_pack, wino_pack, forward) and, for each tnr_conv_forward, the descriptor fields mode, mma, wq != 0, wq_form, ws != 0, shuffle, Cout, m_hi --
copied at call time --, then fwd_shuffle2's return value, or the type of the exception the call raised.  tests/test_cpu_conv_plan.py replays
every row on the code under test.

The table is recorded from the ops.py and engine.py of the commit BEFORE a change to the dispatch, never from the code under test:
    python tools/record_conv_plan.py --commit <commit>
`git show <commit>:trainner_amd/{ops,engine}.py` go to temporary files, are loaded UNEDITED as extra modules of the trainner_amd package, and the
old engine's `ops` global is pointed at the old ops.  Stand-ins: hip.load returns a fake library whose tnr_conv_workspace_bytes /
tnr_conv_wino_bytes / tnr_conv_wq_bytes answers are set per row (1024 = yes, 0 = decline; every other *_bytes entry says 1024, every other entry
records its name and succeeds), hip.stream returns 0, the packer hands out one-off packings with the library's padded dimensions, and the
tensors are CPU tensors whose is_cuda answers True.  Nothing is computed.  The caller's `wino` travels through ConvOp.fwd / dgrad as a keyword
(they hand their keywords to ops.conv); fwd_shuffle2 has no such argument, its rows repeat over that dimension.
"""
import argparse
import contextlib
import itertools
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools.record_dense_plan import _OnDevice, load_ops  # noqa: E402
from trainner_amd import hip  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
MMAS = {"f32": hip.MMA_F32, "bf16": hip.MMA_BF16, "bf16x3": hip.MMA_BF16X3}
DEFAULTS = dict(WINO=True, X3_D4=True, S2_D4=True, IMAGE_C4=True, SMALL_GEMM=True, SHUFFLE_FOLD=True, WINO_MIN_CIN=64, WINO_MIN_PIXELS=4096)
# each switch alone against the defaults, the two thresholds alone, one pair
SWITCHES = [{}] + [{k: False} for k in ("WINO", "X3_D4", "S2_D4", "IMAGE_C4", "SMALL_GEMM", "SHUFFLE_FOLD")] + \
    [{"WINO_MIN_CIN": 128}, {"WINO_MIN_PIXELS": 8192}, {"WINO": False, "X3_D4": False}]
EPIS = ("plain", "act", "r1", "mask")
WINOS = (None, True, False)
ANSWERS = list(itertools.product((1024, 0), repeat=3))          # (split-K workspace, Winograd image, weight stream): every yes / decline
STATES = list(itertools.product(EPIS, WINOS, ANSWERS))
# name: (how it is driven, k, stride, cin, cout, input H = W, nearest-x2, reflect)
LAYERS = {
    "3x3_3to64": ("fwd", 3, 1, 3, 64, 16, False, False), "3x3_64to3": ("fwd", 3, 1, 64, 3, 16, False, False),
    "3x3_3to64_dgrad": ("dgrad", 3, 1, 3, 64, 16, False, False), "3x3_64to64_64": ("fwd", 3, 1, 64, 64, 64, False, False),
    "3x3_64to64_32": ("fwd", 3, 1, 64, 64, 32, False, False), "3x3_64to32_32": ("fwd", 3, 1, 64, 32, 32, False, False),
    "3x3_512to512_64": ("fwd", 3, 1, 512, 512, 64, False, False), "3x3_512to512_4": ("fwd", 3, 1, 512, 512, 4, False, False),
    "3x3_512to512_4_dgrad": ("dgrad", 3, 1, 512, 512, 4, False, False), "3x3_256to256_8": ("fwd", 3, 1, 256, 256, 8, False, False),
    "3x3_256to256_64_reflect": ("fwd", 3, 1, 256, 256, 64, False, True), "3x3_up2_64to64_16": ("fwd", 3, 1, 64, 64, 16, True, False),
    "4x4s2_64to64_32": ("fwd", 4, 2, 64, 64, 32, False, False), "4x4s2_64to64_32_dgrad": ("dgrad", 4, 2, 64, 64, 32, False, False),
    "1x1_64to64_32_bare": ("bare", 1, 1, 64, 64, 32, False, False), "shuffle_64to256_32": ("shuffle", 3, 1, 64, 256, 32, False, False),
    "shuffle_64to256_16": ("shuffle", 3, 1, 64, 256, 16, False, False), "shuffle_20to80_32": ("shuffle", 3, 1, 20, 80, 32, False, False),
}
ENTRIES = {"tnr_conv_thin_pack": "thin_pack", "tnr_conv_thin": "thin", "tnr_im2col": "im2col", "tnr_conv_wq_pack": "wq_pack",
           "tnr_conv_wino_pack": "wino_pack", "tnr_conv_forward": "forward"}


def round_up(a, b):
    return (a + b - 1) // b * b


def note(calls, name, args):
    """Append what the table keeps of one library entry: its short name, and tnr_conv_forward's descriptor fields as they are at the call."""
    if name == "tnr_conv_forward":
        d = args[0]._obj
        calls.append("forward(mode=%d,mma=%d,wq=%d,wq_form=%d,ws=%d,shuffle=%d,Cout=%d,m_hi=%d)" % (
            d.mode, d.mma, bool(d.wq), d.wq_form, bool(d.ws), d.shuffle, d.Cout, d.m_hi))
    elif name in ENTRIES:
        calls.append(ENTRIES[name])


LATE = ("tnr_conv_workspace_bytes", "tnr_conv_wino_bytes", "tnr_conv_wq_bytes")          # the library's three late answers, in ANSWERS' order


class FakeLib:
    """The C ABI without a device: the three late answers are set per row, every other *_bytes / *_floats entry says 1024, the rest succeed."""

    def __init__(self):
        self.calls, self.answers = [], (1024, 1024, 1024)

    def __getattr__(self, name):
        def entry(*args):
            if name in LATE:
                return self.answers[LATE.index(name)]
            if name.endswith("_bytes") or name.endswith("_floats"):
                return 1024
            note(self.calls, name, args)
            return 0
        return entry


_FORWARD = re.compile(r"forward\(mode=(\d+),mma=\d+,wq=(\d),wq_form=(\d),ws=(\d),shuffle=(\d),")


def plan_matches(ops, plan, got):
    """Is conv_plan's answer `plan` the form the outcome string `got` shows?  The form-to-entries mapping, written once for the CPU replay
    and the GPU test."""
    form, why = plan
    if got == "thin_pack+thin":
        return plan == ("thin", None)
    if got in ("=False", "!AssertionError"):          # a shuffle that is not folded; a forced Winograd launch the library declined
        return why is not None and form in (("tile",) if got == "=False" else ("tile", "stream"))
    m = _FORWARD.search(got)
    mode, wq, wq_form, ws, shuffle = (int(g) for g in m.groups())
    head = got[:m.start()]
    if head == "im2col+":
        return form == "im2col" and mode == ops.CONV_1x1 and not wq          # (its 1x1 launch takes a split-K workspace or not: the library's word)
    if mode == ops.CONV_3x3_C4:
        return form == "c4" and head == "" and not wq and not ws
    if ws:
        return plan == ("tile", "splitk") and head == "" and not wq
    if wq:
        return (form, head) == (("wino", "wino_pack+") if wq_form else ("stream", "wq_pack+")) and (shuffle == 2) == got.endswith("=True")
    return form == "tile" and why != "splitk" and head == "" and not shuffle


class FakePacker:
    """WeightPacker's add / get with the library's padded dimensions (csrc/pack_api.hip) and no device: one-off packings (owner None)."""

    def __init__(self, ops):
        self.ops, self.packed = ops, []

    def add(self, w, kind):
        o = self.ops
        Cout, Cin, kh, kw = w.shape
        if kind in (o.PACK_DGRAD_3x3, o.PACK_DGRAD_S2, o.PACK_C4_DGRAD3, o.PACK_COL_DGRAD3):
            Cout, Cin = Cin, Cout
        ki = {o.PACK_COL_FWD: kh * kw * Cin, o.PACK_COL_DGRAD3: kh * kw * Cin, o.PACK_C4_FWD: 36, o.PACK_C4_DGRAD3: 36}.get(kind, Cin)
        self.packed.append(o.Packed(torch.zeros(8), round_up(Cout, 32), round_up(ki, 16), kind, None))
        return len(self.packed) - 1

    def get(self, i):
        return self.packed[i]


class _Mod:
    def __init__(self, k, stride, cin, cout):
        self.kernel_size, self.stride, self.in_channels, self.out_channels = k, stride, cin, cout
        self.weight, self.bias = torch.zeros(cout, cin, k, k), torch.zeros(cout)


def load_parent(commit):
    """-> (ops, engine) of `commit`, loaded unedited beside the tree's own modules."""
    mods = []
    for name in ("ops", "engine"):
        src = subprocess.run(["git", "show", "%s:trainner_amd/%s.py" % (commit, name)], cwd=ROOT, check=True, capture_output=True).stdout
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "_%s_at_parent.py" % name)
            with open(path, "wb") as f:
                f.write(src)
            mods.append(load_ops(path))
    mods[1].ops = mods[0]
    return tuple(mods)


def load_tree():
    from trainner_amd import engine, ops
    return ops, engine


_cases = {}


def case(ops, engine, name, epi_name):
    """One layer x epilogue over cached tensors -> dict(how, op, x, y, wp, mode, epi); op: the layer's ConvOp (None: a bare ops.conv)."""
    key = (id(ops), name, epi_name)
    if key in _cases:
        return _cases[key]
    how, k, stride, cin, cout, H, ups, reflect = LAYERS[name]

    def view(C, side):          # <= 4 channels: the first C of an NHWC4 image buffer
        return ops.View(torch.empty(1, side, side, max(C, 4) if C <= 4 else C).as_subclass(_OnDevice), 0, C)

    Ho = 2 * H if (ups or how == "shuffle") else H // stride
    x, y = view(cin, H), view(cout // 4 if how == "shuffle" else cout, Ho)
    if how == "dgrad":          # x = the gradient of the layer's output, y = the gradient of its input
        x, y = view(cout, Ho), view(cin, H)
    epi = {"plain": {}, "act": dict(act=ops.ACT_LRELU, slope=0.2), "r1": dict(r1=view(y.C, y.H), beta1=0.2), "mask": dict(mask=view(y.C, y.H), m_slope=0.2)}[epi_name]
    if reflect:
        epi = dict(epi, reflect=True)
    c = dict(how=how, x=x, y=y, epi=epi, op=None, mode=ops.CONV_1x1, wp=ops.Packed(torch.zeros(8), round_up(cout, 32), round_up(cin, 16), ops.PACK_FWD, None))
    if how != "bare":
        c["op"] = engine.ConvOp(_Mod(k, stride, cin, cout), FakePacker(ops), ups=ups)
    _cases[key] = c
    return c


@contextlib.contextmanager
def stand_ins(ops, lib):
    saved_hip = (hip.load, hip.stream)
    names = list(DEFAULTS) + ["MMA", "PROFILE"]
    saved = {k: getattr(ops, k) for k in names}
    images = {name: dict(d) for name, d in ops._ONEOFF_IMAGES.items()}
    hip.load, hip.stream = (lambda *a, **k: lib), (lambda: 0)
    ops.PROFILE = None
    try:
        yield
    finally:
        hip.load, hip.stream = saved_hip
        for k, v in saved.items():
            setattr(ops, k, v)
        for name, d in ops._ONEOFF_IMAGES.items():
            d.clear()
            d.update(images[name])
        for key in [k for k in ops.WS.bufs if k[1] == "cpu" and k[0].split("@")[0] in ("splitk", "im2col", "thin_w")]:
            del ops.WS.bufs[key]


def configure(ops, mma, switches):
    for k, v in DEFAULTS.items():
        setattr(ops, k, switches.get(k, v))
    ops.MMA = MMAS[mma]


def run(lib, c, wino, answers):
    """Drive one row -> "<entries reached>" + "=<return value>" for fwd_shuffle2, or + "!<exception type>"."""
    del lib.calls[:]
    lib.answers = answers
    kw = c["epi"] if wino is None else dict(c["epi"], wino=wino)
    try:
        if c["how"] == "bare":
            ret = c["conv"](c["x"], c["wp"], c["y"], mode=c["mode"], **kw)
        elif c["how"] == "shuffle":
            ret = c["op"].fwd_shuffle2(c["x"], c["y"], **c["epi"])
        else:
            ret = getattr(c["op"], c["how"])(c["x"], c["y"], **kw)
        tail = "" if ret is None else "=%s" % ret
    except Exception as e:          # (recorded, not hidden: the table names the type)
        tail = "!" + type(e).__name__
    return "+".join(lib.calls) + tail


def switches_id(sw):
    return ",".join("%s=%s" % (k, int(v)) for k, v in sw.items()) or "defaults"


def rows_of(ops, engine, lib, name, mma, switches):
    """The outcome strings of one (layer, arithmetic, switches) over STATES."""
    configure(ops, mma, switches)
    out = []
    for epi_name, wino, answers in STATES:
        c = case(ops, engine, name, epi_name)
        c["conv"] = ops.conv
        out.append(run(lib, c, wino, answers))
    return out


def table(ops, engine):
    """-> (outcomes, {layer: {mma: {switches: [index into outcomes per STATES entry]}}})"""
    lib, seen = FakeLib(), {}
    with stand_ins(ops, lib):
        rows = {name: {mma: {switches_id(sw): [seen.setdefault(r, len(seen)) for r in rows_of(ops, engine, lib, name, mma, sw)] for sw in SWITCHES}
                       for mma in MMAS} for name in LAYERS}
    return list(seen), rows


def host_cost(ops, engine, calls, repeats=3):
    """Host microseconds per ConvOp.fwd of the 64 -> 64 32 x 32 layer (defaults, bf16x3) over the fake library, one figure per repeat."""
    lib, out = FakeLib(), []
    with stand_ins(ops, lib):
        configure(ops, "bf16x3", {})
        c = case(ops, engine, "3x3_64to64_32", "plain")
        fwd, x, y = c["op"].fwd, c["x"], c["y"]
        fwd(x, y)
        for _ in range(repeats):
            del lib.calls[:]
            t0 = time.perf_counter()
            for _ in range(calls):
                fwd(x, y)
            out.append(round(1e6 * (time.perf_counter() - t0) / calls, 2))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", help="the commit whose ops.py and engine.py are driven (default for --host-cost: the tree's own)")
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--host-cost", type=int, metavar="CALLS", help="instead of recording: time CALLS ConvOp.fwd calls on the host, three repeats")
    a = ap.parse_args()
    if a.host_cost:
        ops, engine = load_parent(a.commit) if a.commit else load_tree()
        print(json.dumps({"code": a.commit or "tree", "calls": a.host_cost, "us_per_call": host_cost(ops, engine, a.host_cost)}))
        return
    assert a.commit, "recording needs --commit: the table comes from a commit's ops.py and engine.py, never from the code under test"
    outcomes, rows = table(*load_parent(a.commit))
    doc = {"recorded_at_commit": a.commit, "states": [[e, w, list(ans)] for e, w, ans in STATES], "outcomes": outcomes, "rows": rows}
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('],"', '],\n"').replace('","', '",\n"') + "\n")          # (one list per line)
    print("wrote", a.out, sum(len(r) for k in rows.values() for m in k.values() for r in m.values()), "rows,", len(outcomes), "distinct outcomes")


if __name__ == "__main__":
    main()
