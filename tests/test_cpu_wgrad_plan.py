"""The weight-gradient tile classes (csrc/wgrad_tile.hip: WG_ROWS, wgrad_class, plan_wgrad) against the table recorded from the commit before
the class table existed (tests/golden/wgrad_classes.json, tools/record_wgrad_classes.py), through the host-only tnr_wgrad_tile_class.  No GPU."""
import ctypes as C
import json

import pytest

from tools import record_wgrad_classes as rec
from trainner_amd import hip, ops


@pytest.fixture(scope="module")
def golden():
    with open(rec.GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def replay():
    """The recorder's walk over this tree's library."""
    lib = hip.load()
    return rec.walk(lib, lambda d: lib.tnr_wgrad_workspace_bytes(C.byref(d)))


def test_grid_is_the_cross_product(golden):
    dims = golden["dims"]
    assert dims == dict(mode=[0, 1, 2], cout=[32, 64], cin_blocks=[1, 2, 3, 4, 5, 6], mma=[0, 1, 2], pad_mode=[0, 1],
                        over=["none", "x", "g"])
    assert [list(v) for v in (rec.MODES, rec.COUTS, rec.CIN_BLOCKS, rec.MMAS, rec.PAD_MODES, rec.OVER)] == list(dims.values())
    assert len(rec.GRID) == len(set(rec.GRID)) == 3 * 2 * 6 * 3 * 2 * 3 == len(golden["cells"])
    assert golden["sizes"] == [list(s) for s in rec.SIZES] and golden["group_jobs"] == list(rec.GROUP_JOBS)
    assert all(len(row) == len(rec.SIZES) for row in golden["cells"])
    # the 2^30 dimension is real: "x" / "g" cells stand at or above the bound, and some "none" cell of every size below it
    for cell in rec.GRID:
        for size in rec.SIZES:
            d = rec.desc(cell, size)
            nx, ng = d.N * d.H * d.W * d.x.ctot, d.N * d.Ho * d.Wo * d.g.ctot
            assert nx < 2 ** 31 and ng < 2 ** 31
            if cell[5] != "none":
                assert (nx if cell[5] == "x" else ng) >= 2 ** 30
            elif cell[0] == 0:
                assert nx < 2 ** 30 and ng < 2 ** 30


def test_every_cell_equals_the_record(golden, replay):
    classes, records, cells = replay
    bad = []
    for cell, want_row, got_row in zip(rec.GRID, golden["cells"], cells):
        for size, wi, gi in zip(rec.SIZES, want_row, got_row):
            want, got = list(golden["records"][wi]), list(records[gi])
            want[0], got[0] = golden["classes"][want[0]], classes[got[0]]
            if want != got:
                bad.append((cell, size, want, got))
    assert not bad, "%d of %d cells differ, first: %r" % (len(bad), len(cells) * len(rec.SIZES), bad[:3])


def test_table_rows_are_the_recorded_classes(golden):
    """No row unreached, none missing: the classes the record reaches are exactly the rows of WG_ROWS (the query's index enumerates them)."""
    recorded = {tuple(c) for c in golden["classes"] if c is not None}
    lib = hip.load()
    rows = {}
    for cell in rec.GRID:
        for size in rec.SIZES[:1] + rec.SIZES[-1:]:
            q = rec.query(lib, rec.desc(cell, size), 0)
            if q is not None:
                assert rows.setdefault(q[11], tuple(q[:7])) == tuple(q[:7])
    assert set(rows.values()) == recorded
    assert sorted(rows) == list(range(len(recorded))), "a table row no descriptor reaches"          # indices 0 .. n-1, each seen
    out = (C.c_int32 * 12)()
    d = rec.desc((0, 32, 4, 5, 0, "none"), (1, 8, 8))          # an arithmetic the table has no row for: no kernel
    assert lib.tnr_wgrad_tile_class(C.byref(d), 0, C.byref(out)) == -1
    msg = lib.tnr_last_error().decode()
    assert "128 -> 32 channels" in msg and "mode 0" in msg


def test_workspace_bytes(golden):
    """tnr_wgrad_workspace_bytes itself, on every cell."""
    lib = hip.load()
    n = 0
    for cell, row in zip(rec.GRID, golden["cells"]):
        for size, ri in zip(rec.SIZES, row):
            d = rec.desc(cell, size)
            assert lib.tnr_wgrad_workspace_bytes(C.byref(d)) == golden["records"][ri][1], (cell, size)
            n += 1
    assert n == len(rec.GRID) * len(rec.SIZES)


def test_group_needs_one_class():
    """A 32-cout and a 64-cout layer do not share a launch: tnr_conv_wgrad_group compares the rows of the table."""
    lib = hip.load()
    a, b = rec.desc((0, 32, 2, 0, 0, "none"), (1, 16, 24)), rec.desc((0, 64, 2, 0, 0, "none"), (1, 16, 24))
    qa, qb = ops.wgrad_tile_class(a), ops.wgrad_tile_class(b)
    assert qa["row"] != qb["row"] and (qa["a_t"], qb["a_t"]) == (1, 2)
    # through the launcher: host-side dummies pass the pointer check, the class comparison fails before anything touches a device
    dummy = (C.c_float * 16)()
    descs = (hip.WgradDesc * 2)()
    for d, src in zip(descs, (a, b)):
        C.memmove(C.byref(d), C.byref(src), C.sizeof(hip.WgradDesc))
        d.x.ptr = d.g.ptr = d.dw = d.ws = C.addressof(dummy)
        d.cin_total = d.Cin
    assert lib.tnr_conv_wgrad_group(descs, 2, None) == -1
    assert "is not in the tile class of layer 0" in lib.tnr_last_error().decode()
