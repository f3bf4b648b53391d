"""Characterisation table of the weight-gradient tile classes (trainner_amd/csrc/wgrad_tile.hip), recorded on the CPU (tests/golden/wgrad_classes.json).

The class a descriptor runs on depends on finitely many facts; GRID is their whole cross product: mode, Cout <= 32 or more, the number of
32-channel input blocks (1..5, >= 6), the arithmetic, pad_mode, and which buffer, if any, is pushed to 2^30 elements
(through the view's total channel count).  Every cell is walked over SIZES (input N, H, W) and GROUP_JOBS (0: the layer alone; the job sums a dense
block's groups produce), and per (cell, size) the table keeps: the kernel's template arguments {MODE, A_T, B_T, THG, BF, WPS, DB} (null: the
launcher refuses the descriptor), the workspace bytes, and (splits, tiles_per_split) per GROUP_JOBS entry.  tests/test_cpu_wgrad_plan.py replays
every cell on the code under test through the library's own tnr_wgrad_tile_class.

The table is recorded from the commit BEFORE a change to the planning, never from the code under test:
    python tools/record_wgrad_classes.py --commit <commit>
`git archive <commit>` goes to a temporary directory, the library is built there and driven through ctypes: that commit's own
tnr_wgrad_tile_class(d, group_jobs, out) and tnr_wgrad_workspace_bytes(d), so the parent needs the three-argument query (any commit from the one
that sliced the table on, profiles/r34a_wgrad_env_cleanout.txt; the first record, of a launcher without the query, took a patch:
profiles/r25a_wgrad_class_table.txt).  --lib names an already built library of that commit instead.  Nothing is launched.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from trainner_amd.hip import WgradDesc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_classes.json")
MODES = (0, 1, 2)                      # TNR_CONV_3x3, _3x3_UP2, _4x4_S2
COUTS = (32, 64)
CIN_BLOCKS = (1, 2, 3, 4, 5, 6)
MMAS = (0, 1, 2)                       # TNR_MMA_F32, _BF16, _BF16X3
PAD_MODES = (0, 1)
OVER = ("none", "x", "g")              # the buffer whose element count is pushed to 2^30
GRID = list(itertools.product(MODES, COUTS, CIN_BLOCKS, MMAS, PAD_MODES, OVER))
SIZES = [(n, h, w) for n in (1, 16) for h, w in ((8, 8), (16, 24), (128, 128), (512, 512))]
GROUP_JOBS = (0, 3, 6, 12, 18)         # an RRDB's groups: three conv5 / six 32-channel pieces / 64-cout pairs + conv5 over three dense blocks


def desc(cell, size):
    """The WgradDesc of one cell at one input size (no buffers: the planning reads shapes only)."""
    mode, cout, blocks, mma, pad_mode, over = cell
    n, h, w = size
    ho, wo = (2 * h, 2 * w) if mode == 1 else (h // 2, w // 2) if mode == 2 else (h, w)
    d = WgradDesc()
    d.N, d.H, d.W, d.Cin, d.Ho, d.Wo, d.Cout = n, h, w, 32 * blocks, ho, wo, cout
    d.mode, d.mma, d.pad_mode = mode, mma, pad_mode
    d.x.ctot, d.g.ctot = d.Cin, d.Cout
    if over == "x":
        d.x.ctot = max(d.Cin, (-(-(1 << 30) // (n * h * w)) + 3) // 4 * 4)
    if over == "g":
        d.g.ctot = max(d.Cout, (-(-(1 << 30) // (n * ho * wo)) + 3) // 4 * 4)
    return d


def query(lib, d, group_jobs):
    """tnr_wgrad_tile_class -> the 12 integers, or None where it refuses."""
    out = (C.c_int32 * 12)()
    return list(out) if lib.tnr_wgrad_tile_class(C.byref(d), group_jobs, C.byref(out)) == 0 else None


def walk(lib, ws_bytes):
    """-> (classes, records, cells): cells[i] lists, per SIZES entry, the index into records of GRID[i]'s record
    [index into classes, workspace bytes, splits and tiles_per_split per GROUP_JOBS entry ...].  ws_bytes(d) -> workspace bytes."""
    classes, records, cells = {}, {}, []
    for cell in GRID:
        row = []
        for size in SIZES:
            d = desc(cell, size)
            got = [query(lib, d, gj) for gj in GROUP_JOBS]
            cls = None if got[0] is None else tuple(got[0][:7])
            assert all((g is None) == (cls is None) and (g is None or tuple(g[:7]) == cls) for g in got), "the class depends on group_jobs"
            rec = (classes.setdefault(cls, len(classes)), ws_bytes(d)) + tuple(v for g in got if g is not None for v in g[8:10])
            row.append(records.setdefault(rec, len(records)))
        cells.append(row)
    return [None if c is None else list(c) for c in classes], [list(r) for r in records], cells


def load_commit(commit, lib):
    if lib is None:
        tmp = tempfile.mkdtemp(prefix="wgrad_record_")
        tar = subprocess.run(["git", "archive", commit], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        subprocess.run([sys.executable, "-m", "trainner_amd.build", "--force"], cwd=tmp, check=True)
        lib = os.path.join(tmp, "trainner_amd", "lib", "libtrainner_hip.so")
    lib = C.CDLL(lib)
    lib.tnr_wgrad_tile_class.restype = C.c_int32
    lib.tnr_wgrad_tile_class.argtypes = [C.POINTER(WgradDesc), C.c_int32, C.POINTER(C.c_int32 * 12)]
    lib.tnr_wgrad_workspace_bytes.restype = C.c_int64
    lib.tnr_wgrad_workspace_bytes.argtypes = [C.POINTER(WgradDesc)]
    return lib


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", required=True, help="the commit whose planning and launcher are recorded: never the code under test")
    ap.add_argument("--lib", help="an already built library of that commit")
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    lib = load_commit(a.commit, a.lib)
    classes, records, cells = walk(lib, lambda d: lib.tnr_wgrad_workspace_bytes(C.byref(d)))
    doc = {"recorded_at_commit": a.commit,
           "dims": dict(mode=MODES, cout=COUTS, cin_blocks=CIN_BLOCKS, mma=MMAS, pad_mode=PAD_MODES, over=OVER),
           "sizes": SIZES, "group_jobs": GROUP_JOBS, "classes": classes, "records": records, "cells": cells}
    with open(a.out, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace('],"', '],\n"').replace("]],[[", "]],\n[[") + "\n")
    print("wrote", a.out, len(cells), "cells x", len(SIZES), "sizes x", len(GROUP_JOBS), "group sizes,", len(records), "distinct records,",
          len([c for c in classes if c is not None]), "classes")


if __name__ == "__main__":
    main()
