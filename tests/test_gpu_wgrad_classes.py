"""One launch on every weight-gradient tile class (csrc/wgrad_tile.hip WG_ROWS), in the
arithmetic of the row, against torch.autograd.grad on the CPU under test_wgrad's criterion: 5e-5 x (max |ref| + 1) for dw and db, alpha = 0.5,
beta = 1 over a random start.  TNR_MMA_BF16 rounds its operands to bf16 in front of the matrix core and their products are exact in fp32, so its
rows are held to the same criterion against autograd on the bf16-ROUNDED x and g (db: the fp32 sum of the un-rounded gradient), as
test_bf16_operand_mode does.  Before the launch the case asserts, through tnr_wgrad_tile_class, that it lands on the row it names.

Shapes, the smallest at which a class can still go wrong: N = 1, 20 x 18 outputs (two tile columns with a ragged edge, more than one tile row for
every THG <= 16); the 4x4-s2 mode from a 24 x 36 input, nearest-x2 from 10 x 9.

The half-height two-workgroup rows of TNR_CONV_3x3, which zero-padded launches reach only from 2^30 elements on, run here through reflection
padding.  test_cases_cover_the_table: no row of the table is left to tests/test_cpu_wgrad_plan.py alone.
"""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from test_gpu_kernels import DEV, _bf, nhwc_buf, rnd

pytestmark = pytest.mark.gpu

F32, BF16, X3 = 0, 1, 2
# (Cin, Cout) -> (A_T, B_T, THG, WPS, DB)
PLAIN = {(32, 32): (1, 1, 16, 1, 0), (64, 32): (1, 2, 16, 1, 0), (96, 32): (1, 3, 4, 2, 0), (128, 32): (1, 4, 8, 1, 0), (160, 32): (1, 3, 4, 2, 0),
         (32, 64): (2, 1, 16, 1, 0), (64, 64): (2, 2, 8, 1, 0)}
HALF = {(32, 32): (1, 1, 8, 2, 0), (64, 32): (1, 2, 4, 2, 0), (96, 32): (1, 3, 4, 2, 0), (128, 32): (1, 2, 4, 2, 0), (160, 32): (1, 3, 4, 2, 0),
        (32, 64): (2, 1, 4, 2, 0), (64, 64): (2, 2, 4, 2, 0)}
PIPELINED = {k: v if v[1] == 3 else v[:3] + (1, 1) for k, v in HALF.items()}
CASES = [(mode, mma, cin, cout, False, row) for mode in ("3x3", "up2") for mma in (F32, BF16) for (cin, cout), row in PLAIN.items()]
CASES += [("3x3", X3, cin, cout, False, row) for (cin, cout), row in PIPELINED.items()]
CASES += [("3x3", X3, cin, cout, True, row) for (cin, cout), row in HALF.items() if row[1] != 3 and cin != 128]
CASES += [("up2", X3, cin, cout, False, row) for (cin, cout), row in HALF.items()]
CASES += [("s2", mma, cin, cout, False, row) for mma in (F32, BF16, X3)
          for (cin, cout), row in (((32, 32), (1, 4, 4, 2, 0)), ((64, 64), (2, 2, 4 if mma == X3 else 8, 2, 0)))]
MODES = {"3x3": 0, "up2": 1, "s2": 2}
_refs = {}


def reference(mode, cin, cout, reflect, mma=F32):
    """x, g, and autograd's dw, db of one layer on the CPU (mma = BF16: dw from the bf16-rounded x and g): computed once per shape, shared by
    the arithmetics it holds for, never written."""
    key = (mode, cin, cout, reflect, mma == BF16)
    if key not in _refs:
        rounded = _bf if mma == BF16 else (lambda t: t)
        k = 4 if mode == "s2" else 3
        H, W = {"3x3": (20, 18), "up2": (10, 9), "s2": (24, 36)}[mode]
        x0 = rnd(1, cin, H, W, seed=24)
        x = rounded(x0)
        w = rnd(cout, cin, k, k, seed=25).requires_grad_(True)
        if mode == "s2":
            y = F.conv2d(x, w, None, stride=2, padding=1)
        elif mode == "up2":
            y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, None, padding=1)
        else:
            y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, None) if reflect else F.conv2d(x, w, None, padding=1)
        g = rnd(*y.shape, seed=26)
        (ref_w,) = torch.autograd.grad(y, w, rounded(g))
        _refs[key] = (x0, g, ref_w, g.sum(dim=(0, 2, 3)))
    return _refs[key]


def lands_on(ops, item, mode, mma, row, group_jobs=0):
    """Assert through the host-only query that `item` runs on {mode, A_T, B_T, THG, BF = mma, WPS, DB} = row."""
    d = ops.WgradDesc()
    ops._wgrad_desc(d, item["x"], item["g"], item["dw"], item.get("db"), MODES[mode], item.get("cin_begin", 0), 1.0, 1.0, item.get("reflect", False))
    q = ops.wgrad_tile_class(d, group_jobs)
    assert (q["mode"], q["a_t"], q["b_t"], q["thg"], q["bf"], q["wps"], q["db"]) == (MODES[mode], *row[:3], mma, *row[3:]), q
    return q


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-mma%d-%dto%d%s-row%s" % (c[0], c[1], c[2], c[3], "-reflect" if c[4] else "", "_".join(map(str, c[5]))))
def test_row(case, monkeypatch):
    from trainner_amd import ops
    mode, mma, cin, cout, reflect, row = case
    monkeypatch.setattr(ops, "MMA", mma)
    x, g, ref_w, ref_b = reference(mode, cin, cout, reflect, mma)
    xb, gb = nhwc_buf(x), nhwc_buf(g)
    dw0, db0 = rnd(*ref_w.shape, seed=27), rnd(cout, seed=28)
    dw, db = dw0.to(DEV), db0.to(DEV)
    item = dict(x=ops.View(xb, 0, cin), g=ops.View(gb, 0, cout), dw=dw, db=db, reflect=reflect)
    lands_on(ops, item, mode, mma, row)
    ops.wgrad(item["x"], item["g"], dw, db, mode=MODES[mode], alpha=0.5, beta=1.0, reflect=reflect)
    err_w = (dw.cpu() - (dw0 + 0.5 * ref_w)).abs().max().item()
    err_b = (db.cpu() - (db0 + 0.5 * ref_b)).abs().max().item()
    print("dw err %.3e (bound %.3e)  db err %.3e (bound %.3e)" % (err_w, 5e-5 * (ref_w.abs().max().item() + 1), err_b, 5e-5 * (ref_b.abs().max().item() + 1)))
    assert err_w <= 5e-5 * (ref_w.abs().max().item() + 1.0), "wgrad weights"
    assert err_b <= 5e-5 * (ref_b.abs().max().item() + 1.0), "wgrad bias"


def test_cases_cover_the_table(monkeypatch):
    """CASES lands on every row of WG_ROWS: the rows its descriptors name through the host-only query (no launch, shapes only) are 0 .. n - 1,
    n the number of classes of the recorded table (tests/golden/wgrad_classes.json), whose classes tests/test_cpu_wgrad_plan.py holds equal
    to the table's rows."""
    from trainner_amd import ops
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_classes.json")) as f:
        n = len([c for c in json.load(f)["classes"] if c is not None])
    rows = set()
    for mode, mma, cin, cout, reflect, row in CASES:
        monkeypatch.setattr(ops, "MMA", mma)
        k = 4 if mode == "s2" else 3
        (H, W), (Ho, Wo) = {"3x3": ((20, 18), (20, 18)), "up2": ((10, 9), (20, 18)), "s2": ((24, 36), (12, 18))}[mode]
        item = dict(x=ops.View(torch.empty(1, H, W, cin)), g=ops.View(torch.empty(1, Ho, Wo, cout)), dw=torch.empty(cout, cin, k, k), reflect=reflect)
        rows.add(lands_on(ops, item, mode, mma, row)["row"])
    assert rows == set(range(n))


@pytest.mark.parametrize("mma", [F32, BF16, X3])
def test_two_item_group(mma, monkeypatch):
    """Two items of a 160 -> 32 layer onto one 32-cout gradient in ONE launch: the second item's jobs start at job_begin = 1.  A 64- and a
    96-channel piece are in different classes (32 x 64 and 32 x 96), and a group of the two is refused, before and after the class table; so
    the items that run are the 64-channel windows at input channels 0 and 96 (what the dense block's conv4 launches beside its middle piece),
    and the literal 64 + 96 group is asserted to fail with the tile-class message."""
    from trainner_amd import ops
    monkeypatch.setattr(ops, "MMA", mma)
    x, g, ref_w, ref_b = reference("3x3", 160, 32, False, mma)
    xb, gb = nhwc_buf(x), nhwc_buf(g)
    dw0, db0 = rnd(*ref_w.shape, seed=27), rnd(32, seed=28)
    dw, db = dw0.to(DEV), db0.to(DEV)
    gv = ops.View(gb, 0, 32)

    def items(pieces):
        return [dict(x=ops.View(xb, lo, n), g=gv, dw=dw, db=db if lo == 0 else None, cin_begin=lo, alpha=0.5, beta=1.0) for lo, n in pieces]
    with pytest.raises(RuntimeError, match="tile class"):
        ops.wgrad_group(items(((0, 64), (64, 96))))
    assert torch.equal(dw.cpu(), dw0) and torch.equal(db.cpu(), db0)          # (refused before any launch)
    group = items(((0, 64), (96, 64)))
    rows = [lands_on(ops, it, "3x3", mma, PIPELINED[(64, 32)] if mma == X3 else PLAIN[(64, 32)], group_jobs=2)["row"] for it in group]
    assert rows[0] == rows[1]
    ops.wgrad_group(group)
    want = dw0 + 0.5 * ref_w
    want[:, 64:96] = dw0[:, 64:96]          # the channels no item covers keep their start
    assert (dw.cpu() - want).abs().max().item() <= 5e-5 * (ref_w.abs().max().item() + 1.0), "wgrad weights"
    assert torch.equal(dw.cpu()[:, 64:96], dw0[:, 64:96])
    assert (db.cpu() - (db0 + 0.5 * ref_b)).abs().max().item() <= 5e-5 * (ref_b.abs().max().item() + 1.0), "wgrad bias"
