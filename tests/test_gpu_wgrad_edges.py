"""Edge-shape parity of the weight-gradient kernels (csrc/wgrad_tile.hip with wgrad_reduce_kernel, csrc/wgrad_thin.hip) against
torch.autograd.grad of the plain F.conv2d statement of the layer in FLOAT64 on the CPU.  test_gpu_wgrad_classes.py launches every tile
class at one small shape; here the classes run at the shapes at which such kernels go wrong (the class is part of the test id).

wgrad_tile (a tile is 16 pixels wide and THG = T rows tall; e = the smallest ragged edge: 1 pixel, 2 for nearest-x2 whose outputs are even):
  px1      one output pixel (3x3, 4x4-s2 from 2 x 2), 2 x 2 outputs (nearest-x2 from 1 x 1; reflection, which needs 2 x 2)
  line     Ho = e with Wo = 16 + e, and Wo = e with Ho = T + e
  one      tiles_total == 1, ragged inside the tile (3 x 5; nearest-x2: 2 x 4)
  lone     13 tiles in splits of 4, 4, 4, 1: the last split is ONE tile, and that tile is e pixel rows tall
  images   N = 3, 6 tiles per image in splits of 4, 4, 4, 4, 2: splits begin in one image and end in the next; the last tile column
           and the last tile row are e pixels wide / tall
  oddC     the `images` shape with Cin / Cout = 100 / 12, 36 / 36, 20 / 12 (multiples of 4, not of 32), NaN directly behind the last channel
  splitsK  K = 7, 8, 9 (body and tail of the reduce form with eight rows per block), 32 (its last), 33 and 40 (one block per row: the
           stride-32 loop and the stride-8 tail), the last split always 2 tiles short; K = 33 on the 4x4-s2 tap map, on a cout pair
           ([g4 | g3], two dw of different cin_total, both db) and K = 9 / 33 on a two-item group planned with group_jobs = 2
  beta0    dw / db start as NaN and beta = 0: the kernels promise not to read the destination
wgrad_thin / wgrad_thin7 (both flips, Cbig 16 / 32 / 64, Csmall 1 / 3):
  px1 / min, lineH, lineW   the smallest sizes the entry accepts (wgrad_thin7 with rpad = 3 needs H, W >= 4 and refuses 3)
  pass     W on both sides of the staged-row width (WT_MAXW = 512, W7_MAXW = 320 columns of the big grid)
  rows     more rows than the grid (1025 > WT_GRID, 513 > W7_GRID): two rows per workgroup, the last workgroup short, H odd, so one
           workgroup's two rows lie in two images
  beta0    as above

Traps in every case.  x and g are views at two different non-zero channel offsets of two wider buffers of different width whose other
channels hold NaN (the sources hold the same bits afterwards).  Every launch runs once over input channels [5, 5 + Cin) of a dw with
cin_total = Cin + 9 (the other entries bit-unchanged, no db: the entry allows db only with cin_begin == 0) and once with cin_begin == 0
and db.  Every workspace buffer the launch uses is filled with NaN before it.  Every launch runs twice and returns the same bits.  An
output whose reference is an EMPTY sum (counted with all-ones inputs) equals beta x start bit for bit.  The thin operand's pad channels
(channel 3 and channels >= Csmall) hold a finite non-zero sentinel, and the stored result has the bits of a launch with zeros there.

Bounds.  alpha = 0.5, beta = 1 over a random start.  err(device) against fp64 <= 2 x err(the same statement in fp32 on the CPU: autograd and
the beta x start + alpha x sum around it) + 2e-7 x max|ref| per output tensor (test_gpu_membound_kernels.yardstick: the factor allows
another, equally valid summation order, the additive term one output rounding).  TNR_MMA_BF16: dw against the bf16-ROUNDED x and g
(products of bf16 values are exact), db against the un-rounded g.  TNR_MMA_BF16X3 is also held to 1.5 x (error of the fp32-matrix-core
launch on the same inputs) + 2e-7 x scale.  No comparison leaves out an element.

test_inputs_and_references (no device) builds every case's inputs and references and asserts through tnr_wgrad_tile_class the class row
and split arithmetic each case names, that no yardstick denominator is zero and that the planted empty sums are empty.  So the module has
no module-level `pytestmark`: every other test carries the gpu mark itself.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K
import test_gpu_membound_kernels as M
import test_gpu_wgrad_classes as WC

gpu = pytest.mark.gpu
NAN = float("nan")
D = torch.double
F32, BF16, X3 = WC.F32, WC.BF16, WC.X3
ARITH = {F32: "f32", BF16: "bf16", X3: "bf16x3"}
ALPHA = 0.5
PAD_SENT = 7.5                                                   # the thin operand's pad channels
cache = functools.lru_cache(maxsize=None)
ROW = {(mode, mma, cin, cout, reflect): row for mode, mma, cin, cout, reflect, row in WC.CASES}


def cdiv(a, b):
    return -(-a // b)


def up32(c):
    return cdiv(c, 32) * 32


def same_bits(a, b):
    """torch.equal on the bit patterns (the buffers hold NaN on purpose)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nan_outside(v):
    v.buf[..., :v.coff] = NAN
    v.buf[..., v.coff + v.C:] = NAN
    return v


def g_offset(cin, cout):
    """channel offset of the g view: 8, or 12 where the two buffers would otherwise be equally wide"""
    return 8 if 8 + cout + M.hi_pad(8, cout) != 4 + cin + M.hi_pad(4, cin) else 12


def views(x, g):
    """x at channel offset 4 and g at 8 (12) of two NaN-filled buffers of different width"""
    xv, gv = nan_outside(M.win(x, 4)), nan_outside(M.win(g, g_offset(x.shape[1], g.shape[1])))
    assert xv.ctot != gv.ctot and xv.coff != gv.coff
    return xv, gv


def held(what, got, exp64, exp32):
    """the device against fp64, held to the fp32 statement on the CPU (prints the YARDSTICK line)"""
    # worst device / bound measured on an MI355X: 0.73 (wgrad_thin `rows`, db of the flipped form), 0.51 (wgrad_thin7 `pass`), tiles 0.48
    # (dw, `lineH` f32) and 0.44 (db, `images`); per class and arithmetic in DESIGN.md 20
    return M.yardstick(what, got, exp64, exp32)


def held_x3(what, got_x3, got_f32, exp64):
    """the project's own bf16x3 criterion: err <= 1.5 x err(fp32-matrix-core launch on the same inputs) + 2e-7 x scale"""
    e64 = exp64.to(got_x3.device)
    scale = float(exp64.abs().max())
    e_x3, e_f32 = float((got_x3.double() - e64).abs().max()), float((got_f32.double() - e64).abs().max())
    bound = 1.5 * e_f32 + 2e-7 * scale
    print("YARDSTICK-X3 %-41s x3 %.3e  f32-mma %.3e  scale %.3e  x3/bound %.3f" % (what, e_x3, e_f32, scale, e_x3 / bound if bound else float("inf")))
    assert e_x3 <= bound, (what, e_x3, e_f32, scale)         # worst x3 / bound measured on an MI355X: 0.64 (dw, `images`); DESIGN.md 20


# =====================================================================================================================
# 1. wgrad_tile + wgrad_reduce
# =====================================================================================================================
def statement(mode, reflect, x, w):
    if mode == "s2":
        return F.conv2d(x, w, None, stride=2, padding=1)
    if mode == "up2":
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, None, padding=1)
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, None) if reflect else F.conv2d(x, w, None, padding=1)


def in_size(mode, Ho, Wo):
    return (2 * Ho, 2 * Wo) if mode == "s2" else ((Ho // 2, Wo // 2) if mode == "up2" else (Ho, Wo))


@cache
def tile_inputs(mode, cin, cout, N, Ho, Wo):
    H, W = in_size(mode, Ho, Wo)
    return K.rnd(N, cin, H, W, seed=1100 + cin), K.rnd(N, cout, Ho, Wo, seed=1200 + cout)


def grad_w(mode, reflect, x, g, cout, dtype):
    k = 4 if mode == "s2" else 3
    w = torch.zeros(cout, x.shape[1], k, k, dtype=dtype, requires_grad=True)
    (dw,) = torch.autograd.grad(statement(mode, reflect, x.to(dtype), w), w, g.to(dtype))
    return dw


@cache
def tile_refs(mode, reflect, cin, cout, N, Ho, Wo, rounded):
    """dw, db of the layer in fp64 and in fp32 (rounded: dw from the bf16-rounded x and g, db from g as it is), and the number of
    terms of every dw element (its sum is empty where that is 0)"""
    x, g = tile_inputs(mode, cin, cout, N, Ho, Wo)
    xr, gr = (K._bf(x), K._bf(g)) if rounded else (x, g)
    count = grad_w(mode, reflect, torch.ones_like(x), torch.ones_like(g), cout, D)
    return (grad_w(mode, reflect, xr, gr, cout, D), g.double().sum((0, 2, 3)), grad_w(mode, reflect, xr, gr, cout, torch.float32),
            g.sum((0, 2, 3)), count)


SPLIT_TILES = {7: (1, 2, 13), 8: (3, 2, 5), 9: (1, 2, 17), 32: (3, 2, 21), 33: (5, 2, 13), 40: (1, 2, 79)}      # K -> N, tile columns, tile rows


def shape_of(cls, mode, T, reflect=False):
    """N, Ho, Wo of a class on a row with THG = T"""
    e = 2 if mode == "up2" else 1
    if cls == "px1":
        return (1, 2, 2) if (mode == "up2" or reflect) else (1, 1, 1)
    if cls.startswith("splits"):
        N, tx, ty = SPLIT_TILES[int(cls[6:])]
        return (N, (ty - 1) * T + e, 16 * (tx - 1) + 4)
    return {"lineH": (1, e, 16 + e), "lineW": (1, T + e, e), "one": (1, 3, 5) if e == 1 else (1, 2, 4), "lone": (1, 12 * T + e, 12 + e),
            "images": (3, 2 * T + e, 16 + e), "oddC": (3, 2 * T + e, 16 + e), "beta0": (3, 2 * T + e, 16 + e)}[cls]


def tile_case(cls, mode, mma, cin, cout, reflect=False):
    row = ROW[(mode, mma, up32(cin), up32(cout), reflect)]
    return (cls, mode, mma, cin, cout, reflect, row) + shape_of(cls, mode, row[2], reflect)


def tile_id(c):
    return "%s-%s-%s-%dto%d%s-row%s" % (c[0], c[1], ARITH[c[2]], c[3], c[4], "-reflect" if c[5] else "", "_".join(map(str, c[6])))


EVERY_ROW = [tile_case(cls, mode, mma, cin, cout, reflect) for cls in ("one", "lone", "images") for mode, mma, cin, cout, reflect, _ in WC.CASES]
SMALL = [tile_case(cls, mode, mma, cin, cout) for cls in ("px1", "lineH", "lineW") for mma in ARITH
         for mode, cin, cout in (("3x3", 32, 32), ("3x3", 64, 64), ("up2", 64, 32), ("s2", 32, 32))]      # A_T = 1, A_T = 2, one up2 and one s2 row
SMALL += [tile_case("px1", "3x3", X3, 64, 64, True)]                                                     # reflection: 2 x 2
ODDC = [tile_case("oddC", mode, mma, cin, cout) for mma in ARITH for mode, cin, cout in (("3x3", 100, 12), ("3x3", 36, 36), ("s2", 20, 12))]
SPLITS = [tile_case("splits%d" % k, "3x3", mma, 64, 64) for mma in ARITH for k in SPLIT_TILES]
SPLITS += [tile_case("splits33", "s2", mma, 32, 32) for mma in ARITH]
BETA0 = [tile_case("beta0", mode, mma, cin, cout) for mma in ARITH for mode, cin, cout in (("3x3", 64, 64), ("up2", 32, 32), ("s2", 64, 64))]
TILE_CASES = EVERY_ROW + SMALL + ODDC + SPLITS + BETA0
PAIR_CASES = [tile_case("splits33", "3x3", mma, 64, 64) for mma in ARITH]
GROUP_CASES = [tile_case("splits%d" % k, "3x3", mma, 64, 32) for mma in ARITH for k in (9, 33)]


class Stub:
    """what _wgrad_desc reads of a View or a tensor: enough for the host-only class query, no memory behind it"""
    def __init__(self, N=0, H=0, W=0, C=0, ctot=0, coff=0, shape=None):
        self.N, self.H, self.W, self.C, self.ctot, self.coff, self.shape = N, H, W, C, ctot, coff, shape

    def c(self):
        from trainner_amd import hip
        return hip.CView(None, self.ctot, self.coff)

    def data_ptr(self):
        return None


def plan(ops, case, group_jobs=0, cin_begin=0):
    """the class query for a case's views (stubs of the same geometry): asserts the row, returns the plan"""
    cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
    H, W = in_size(mode, Ho, Wo)
    glo = g_offset(cin, cout)
    item = dict(x=Stub(N, H, W, cin, 4 + cin + M.hi_pad(4, cin), 4), g=Stub(N, Ho, Wo, cout, glo + cout + M.hi_pad(glo, cout), glo),
                dw=Stub(shape=(cout, cin + 9)), cin_begin=cin_begin, reflect=reflect)
    prev, ops.MMA = ops.MMA, mma
    try:
        return WC.lands_on(ops, item, mode, mma, row, group_jobs)
    finally:
        ops.MMA = prev


def check_plan(case, q):
    """the split arithmetic the class names"""
    cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
    T, e = row[2], 2 if mode == "up2" else 1
    per_image = cdiv(Wo, 16) * cdiv(Ho, T)
    total, splits, tps = per_image * N, q["splits"], q["tiles_per_split"]
    assert splits == cdiv(total, tps)
    last = total - (splits - 1) * tps
    if cls in ("px1", "one"):
        assert total == 1 and splits == 1
    if cls == "lineH":
        assert total == 2 and splits == 1 and Ho == e and Wo - 16 == e
    if cls == "lineW":
        assert total == 2 and splits == 1 and Ho - T == e and Wo == e
    if cls == "lone":
        assert (total, splits, tps, last) == (13, 4, 4, 1) and Ho - (cdiv(Ho, T) - 1) * T == e
    if cls in ("images", "oddC", "beta0"):
        assert N >= 3 and (total, splits, tps, last) == (18, 5, 4, 2) and per_image % tps != 0
        spans = [s for s in range(splits) if (s * tps) // per_image != (min((s + 1) * tps, total) - 1) // per_image]
        assert spans, "no split begins in one image and ends in the next"
        assert Wo % 16 == e and Ho % T == e
    if cls.startswith("splits"):
        k = int(cls[6:])
        assert splits == k and tps == 4 and last == 2, (splits, tps, last)
        assert (8 if splits <= 32 else 1) == (1 if k in (33, 40) else 8)     # the reduce form: eight rows per block up to 32 splits
    if cls == "oddC":
        assert cin % 4 == 0 and cout % 4 == 0 and cin % 32 != 0 and cout % 32 != 0


def trap_workspaces(ops, items, mode):
    """NaN into every workspace buffer the launch will use: each slab row of each split must be written by this launch"""
    from trainner_amd import hip
    for i, it in enumerate(items):
        d = ops.WgradDesc()
        ops._wgrad_desc(d, it["x"], it["g"], it["dw"], it.get("db"), WC.MODES[mode], it.get("cin_begin", 0), 1.0, 1.0, it.get("reflect", False), it.get("pair"))
        need = hip.load().tnr_wgrad_workspace_bytes(ctypes.byref(d))
        ops.WS.get("wgrad%d" % i, need, it["x"].buf.device).view(torch.float32).fill_(NAN)


def launch_twice(ops, mode, make, sources, once=False):
    """make() -> (items, outputs) on a fresh start.  Two launches, NaN in the workspaces before each: the same bits, and the source
    buffers keep theirs"""
    snaps = [v.buf.clone() for v in sources]
    runs = []
    for _ in range(1 if once else 2):
        items, outs = make()
        trap_workspaces(ops, items, mode)
        ops.wgrad_group(items, mode=WC.MODES[mode])
        runs.append(outs)
    for a, b in zip(runs[0], runs[-1]):
        assert same_bits(a, b), "two launches on the same inputs differ"
    for v, s in zip(sources, snaps):
        assert same_bits(v.buf, s), "a source buffer changed"
    return runs[0]


def compare(what, got, start, ref64, ref32, beta, count=None):
    """got against beta x start + ALPHA x ref; where the sum is empty the bits of beta x start"""
    base64, base32 = (start.double(), start) if beta != 0.0 else (torch.zeros_like(ref64), torch.zeros_like(ref32))
    assert bool(torch.isfinite(got).all()), what
    held(what, got, beta * base64 + ALPHA * ref64, beta * base32 + ALPHA * ref32)
    if count is not None and bool((count == 0).any()):
        empty = (count == 0).to(got.device)
        assert torch.equal(got[empty], (beta * base32).to(got.device)[empty]), "%s: an empty sum must leave beta x start" % what


@gpu
@pytest.mark.parametrize("case", TILE_CASES, ids=tile_id)
def test_tile(case, monkeypatch):
    from trainner_amd import ops
    cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
    monkeypatch.setattr(ops, "MMA", mma)
    beta = 0.0 if cls == "beta0" else 1.0
    x, g = tile_inputs(mode, cin, cout, N, Ho, Wo)
    dw64, db64, dw32, db32, count = tile_refs(mode, reflect, cin, cout, N, Ho, Wo, mma == BF16)
    k = dw64.shape[-1]
    xv, gv = views(x, g)
    for cb in (5, 0):                              # cin_begin > 0 (no db), then cin_begin == 0 with db
        dw0 = K.rnd(cout, cin + 9, k, k, seed=1300 + cb)
        db0 = K.rnd(cout, seed=1301)
        if beta == 0.0:                            # NaN in the part of dw the launch owns, and in db: not read
            dw0[:, cb:cb + cin] = NAN
            db0[:] = NAN

        def make():
            dw, db = dw0.to(K.DEV), db0.to(K.DEV) if cb == 0 else None
            return [dict(x=xv, g=gv, dw=dw, db=db, cin_begin=cb, alpha=ALPHA, beta=beta, reflect=reflect)], [dw] + ([db] if cb == 0 else [])
        check_plan(case, WC.lands_on(ops, make()[0][0], mode, mma, row))
        outs = launch_twice(ops, mode, make, (xv, gv))
        what = "%s cb%d" % (tile_id(case), cb)
        own = outs[0][:, cb:cb + cin]
        compare(what + " dw", own, dw0[:, cb:cb + cin], dw64, dw32, beta, count)
        keep = torch.ones(cin + 9, dtype=torch.bool)
        keep[cb:cb + cin] = False
        assert same_bits(outs[0][:, keep.to(K.DEV)], dw0[:, keep].to(K.DEV)), "dw entries of input channels outside the launch changed"
        if cb == 0:
            compare(what + " db", outs[1], db0, db64, db32, beta)
        if mma == X3:                              # the same launch on the fp32 matrix core
            monkeypatch.setattr(ops, "MMA", F32)
            ref_outs = launch_twice(ops, mode, make, (xv, gv), once=True)
            monkeypatch.setattr(ops, "MMA", X3)
            base = torch.zeros_like(dw64) if beta == 0.0 else dw0[:, cb:cb + cin].double()
            held_x3(what + " dw", own, ref_outs[0][:, cb:cb + cin], beta * base + ALPHA * dw64)
            if cb == 0:
                held_x3(what + " db", outs[1], ref_outs[1], (0.0 if beta == 0.0 else db0.double()) + ALPHA * db64)


@gpu
@pytest.mark.parametrize("case", PAIR_CASES, ids=tile_id)
def test_cout_pair_33_splits(case, monkeypatch):
    """[g4 | g3] with cout_split = 32 over one x: channels < 32 of g belong to (dw, db) with cin_total = 96, the others to (dw2, db2)
    with cin_total2 = 64; the reduce with one block per row"""
    from trainner_amd import ops
    cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
    monkeypatch.setattr(ops, "MMA", mma)
    x, g = tile_inputs(mode, cin, cout, N, Ho, Wo)
    dw64, db64, dw32, db32, count = tile_refs(mode, reflect, cin, cout, N, Ho, Wo, mma == BF16)
    xv, gv = views(x, g)
    a0, b0, a20, b20 = K.rnd(32, 96, 3, 3, seed=1310), K.rnd(32, seed=1311), K.rnd(32, 64, 3, 3, seed=1312), K.rnd(32, seed=1313)

    def make():
        a, b, a2, b2 = (t.to(K.DEV) for t in (a0, b0, a20, b20))
        return [dict(x=xv, g=gv, dw=a, db=b, alpha=ALPHA, beta=1.0, pair=(a2, b2, 32))], [a, b, a2, b2]
    q = WC.lands_on(ops, make()[0][0], mode, mma, row)
    check_plan(case, q)
    a, b, a2, b2 = launch_twice(ops, mode, make, (xv, gv))
    what = tile_id(case) + " pair"
    compare(what + " dw", a[:, :64], a0[:, :64], dw64[:32], dw32[:32], 1.0)
    assert same_bits(a[:, 64:], a0[:, 64:].to(K.DEV))
    compare(what + " dw2", a2, a20, dw64[32:], dw32[32:], 1.0)
    compare(what + " db", b, b0, db64[:32], db32[:32], 1.0)
    compare(what + " db2", b2, b20, db64[32:], db32[32:], 1.0)


@gpu
@pytest.mark.parametrize("case", GROUP_CASES, ids=tile_id)
def test_two_item_group_splits(case, monkeypatch):
    """the 64-channel windows at input channels 0 and 96 of a 160 -> 32 layer in ONE launch whose split count is planned for the group's
    two jobs; channels 64 .. 95 of x, outside both views, hold NaN like everything else outside"""
    from trainner_amd import ops
    cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
    monkeypatch.setattr(ops, "MMA", mma)
    x, g = tile_inputs(mode, 160, cout, N, Ho, Wo)
    dw64, db64, dw32, db32, count = tile_refs(mode, reflect, 160, cout, N, Ho, Wo, mma == BF16)
    xall, gv = views(x, g)
    xall.buf[..., xall.coff + 64:xall.coff + 96] = NAN
    dw0, db0 = K.rnd(32, 160, 3, 3, seed=1320), K.rnd(32, seed=1321)

    def make():
        dw, db = dw0.to(K.DEV), db0.to(K.DEV)
        return [dict(x=xall.sub(lo, 64), g=gv, dw=dw, db=db if lo == 0 else None, cin_begin=lo, alpha=ALPHA, beta=1.0) for lo in (0, 96)], [dw, db]
    for it in make()[0]:
        check_plan(case, WC.lands_on(ops, it, mode, mma, row, group_jobs=2))
    dw, db = launch_twice(ops, mode, make, (xall, gv))
    what = tile_id(case) + " group"
    for lo in (0, 96):
        compare("%s dw@%d" % (what, lo), dw[:, lo:lo + 64], dw0[:, lo:lo + 64], dw64[:, lo:lo + 64], dw32[:, lo:lo + 64], 1.0)
    assert same_bits(dw[:, 64:96], dw0[:, 64:96].to(K.DEV)), "the input channels no item covers changed"
    compare(what + " db", db, db0, db64, db32, 1.0)


# =====================================================================================================================
# 2. wgrad_thin, wgrad_thin7
# =====================================================================================================================
THIN_SHAPES = {"px1": (1, 1, 1), "lineH": (1, 1, 37), "lineW": (1, 9, 1), "pass511": (1, 3, 511), "pass512": (1, 3, 512), "pass513": (1, 3, 513),
               "rows": (5, 205, 3), "beta0": (2, 5, 7)}
# (N, H, W) of the wide buffer; the big grid is (H + 2 rpad) x (W + 2 rpad)
THIN7_SHAPES = {False: {"px1": (1, 1, 1), "lineH": (1, 1, 21), "lineW": (1, 9, 1), "pass319": (1, 3, 319), "pass320": (1, 3, 320), "pass321": (1, 3, 321),
                        "rows": (3, 171, 5), "beta0": (2, 5, 7)},
                True: {"min": (1, 4, 4), "lineH": (1, 4, 21), "lineW": (1, 9, 4), "pass319": (1, 4, 313), "pass320": (1, 4, 314), "pass321": (1, 4, 315),
                       "rows": (3, 165, 5), "beta0": (2, 5, 7)}}
THIN_CASES = [(cls, flip, cb, cs) for cls in THIN_SHAPES for flip in (False, True) for cb in (16, 32, 64) for cs in (1, 3)
              if cls != "beta0" or (cb, cs) == (32, 3)]
THIN7_CASES = [(cls, flip, cb, cs) for flip in (False, True) for cls in THIN7_SHAPES[flip] for cb in (16, 32, 64) for cs in (1, 3)
               if cls != "beta0" or (cb, cs) == (32, 3)]


def thin_id(c):
    return "%s-%s-C%d-c%d" % (c[0], "flip" if c[1] else "noflip", c[2], c[3])


def thin_statement(k, flip, big, small, w):
    """k = 3: a 3x3 layer with zero padding.  k = 7, flip = False: the 7x7 layer over its input as GIVEN ((H + 6) x (W + 6), already
    padded); flip = True: ReflectionPad2d(3) in front.  flip = False: small -> big channels (big = the output gradient)"""
    if k == 3:
        return F.conv2d(big if flip else small, w, None, padding=1)
    return F.conv2d(F.pad(big, (3, 3, 3, 3), mode="reflect"), w, None) if flip else F.conv2d(small, w, None)


@cache
def thin_case(k, cls, flip, cb, cs):
    """big, small, start of dw / db, and dw / db in fp64 and fp32 with the term count of every dw element"""
    N, H, W = (THIN_SHAPES if k == 3 else THIN7_SHAPES[flip])[cls]
    big = K.rnd(N, cb, H, W, seed=1400 + k)
    hs, ws = (H + 6, W + 6) if (k == 7 and not flip) else (H, W)
    small = K.rnd(N, cs, hs, ws, seed=1401 + k)
    shape = (cs, cb, k, k) if flip else (cb, cs, k, k)

    def grad(b, s, dtype):
        w = torch.zeros(shape, dtype=dtype, requires_grad=True)
        xin, gout = (b, s) if flip else (s, b)
        (dw,) = torch.autograd.grad(thin_statement(k, flip, b.to(dtype), s.to(dtype), w), w, gout.to(dtype))
        return dw
    gout = small if flip else big
    db64, db32 = gout.double().sum((0, 2, 3)), gout.sum((0, 2, 3))
    for draw in range(256):         # a db of one to three elements over a few pixels can round exactly in fp32: its start is drawn again
        db0 = K.rnd(shape[0], seed=1403 + 16 * draw, lo=-4.0, hi=4.0)      # until the fp32 statement differs from fp64 (the yardstick's denominator)
        if float(((db0 + ALPHA * db32).double() - (db0.double() + ALPHA * db64)).abs().max()) > 0.0:
            break
    return dict(big=big, small=small, dw0=K.rnd(*shape, seed=1402), db0=db0, dw64=grad(big, small, D), dw32=grad(big, small, torch.float32),
                db64=db64, db32=db32, count=grad(torch.ones_like(big), torch.ones_like(small), D))


def small4(small, fill):
    """NHWC4 buffer of the thin operand, `fill` in its pad channels"""
    N, cs, H, W = small.shape
    buf = torch.full((N, H, W, 4), fill, dtype=torch.float32)
    buf[..., :cs] = small.permute(0, 2, 3, 1)
    return buf.to(K.DEV)


def run_thin(ops, k, c, flip, bigv, sv, beta, with_db):
    """one launch on a fresh start with NaN in its workspace -> dw, db"""
    from trainner_amd import hip
    lib = hip.load()
    dw0, db0 = c["dw0"].clone(), c["db0"].clone()
    if beta == 0.0:
        dw0[:], db0[:] = NAN, NAN
    dw, db = dw0.to(K.DEV), db0.to(K.DEV) if with_db else None
    rpad = 3 if (k == 7 and flip) else 0
    if k == 3:
        name, need = "wgrad_thin@%x", lib.tnr_wgrad_thin_workspace_bytes(bigv.N, bigv.H, bigv.C)
    else:
        name, need = "wgrad_thin7@%x", lib.tnr_wgrad_thin7_workspace_bytes(bigv.N, bigv.H + 2 * rpad, bigv.C)
    ops.WS.get(name % hip.stream(), need, bigv.buf.device).view(torch.float32).fill_(NAN)
    if k == 3:
        ops.wgrad_thin(bigv, sv, dw, db, flip=flip, alpha=ALPHA, beta=beta)
    else:
        ops.wgrad_thin7(bigv, sv, dw, db, flip=flip, rpad=rpad, off=-6 if flip else 0, alpha=ALPHA, beta=beta)
    return dw, db


def check_thin(k, case):
    ops = K._ops()
    cls, flip, cb, cs = case
    c = thin_case(k, cls, flip, cb, cs)
    beta = 0.0 if cls == "beta0" else 1.0
    with_db = not (k == 7 and flip)                       # (that form has no bias output)
    bigv = nan_outside(M.win(c["big"], 8))
    s_sent, s_zero = ops.View(small4(c["small"], PAD_SENT)), ops.View(small4(c["small"], 0.0))
    snaps = [bigv.buf.clone(), s_sent.buf.clone()]
    dw, db = run_thin(ops, k, c, flip, bigv, s_sent, beta, with_db)
    for sv in (s_sent, s_zero):                           # the same bits again, and with zeros in the thin operand's pad channels
        dw2, db2 = run_thin(ops, k, c, flip, bigv, sv, beta, with_db)
        assert same_bits(dw, dw2) and (db is None or same_bits(db, db2)), "the result depends on %s" % ("the pad channels" if sv is s_zero else "the run")
    assert same_bits(bigv.buf, snaps[0]) and same_bits(s_sent.buf, snaps[1]), "a source buffer changed"
    what = "thin%d %s" % (k, thin_id(case))
    compare(what + " dw", dw, c["dw0"], c["dw64"], c["dw32"], beta, c["count"])
    if with_db:
        compare(what + " db", db, c["db0"], c["db64"], c["db32"], beta)


@gpu
@pytest.mark.parametrize("case", THIN_CASES, ids=thin_id)
def test_thin(case):
    check_thin(3, case)


@gpu
@pytest.mark.parametrize("case", THIN7_CASES, ids=thin_id)
def test_thin7(case):
    check_thin(7, case)


@gpu
@pytest.mark.parametrize("hw", [(3, 4), (4, 3)], ids=["H3", "W3"])
def test_thin7_refuses_a_reflection_wider_than_the_image(hw):
    """rpad = 3 needs H, W >= 4 (the smallest accepted size is the `min` class): one below, the entry returns its error before any
    launch and dw keeps its bits"""
    from trainner_amd import hip
    ops = K._ops()
    H, W = hw
    bigv = nan_outside(M.win(K.rnd(1, 16, H, W, seed=1410), 8))
    sv = ops.View(small4(K.rnd(1, 3, H, W, seed=1411), PAD_SENT))
    dw0 = K.rnd(3, 16, 7, 7, seed=1412)
    dw = dw0.to(K.DEV)
    with pytest.raises(hip.HipEngineError, match="wgrad_thin7"):
        ops.wgrad_thin7(bigv, sv, dw, None, flip=True, rpad=3, off=-6, alpha=ALPHA, beta=1.0)
    torch.cuda.synchronize()
    assert same_bits(dw, dw0.to(K.DEV))


# =====================================================================================================================
# 3. the device-free self-check
# =====================================================================================================================
def test_inputs_and_references():
    from trainner_amd import ops
    for name, f in list(globals().items()):
        if name.startswith("test_") and name != "test_inputs_and_references":
            assert any(m.name == "gpu" for m in getattr(f, "pytestmark", [])), "%s lacks @gpu" % name
    assert "pytestmark" not in globals()
    # coverage: every row test_gpu_wgrad_classes reaches gets one, lone and images
    assert len(EVERY_ROW) == 3 * len(WC.CASES) and len(set(TILE_CASES)) == len(TILE_CASES)
    for mma in ARITH:
        for cls in ("px1", "lineH", "lineW"):
            got = {(c[1], c[6][0]) for c in SMALL if c[0] == cls and c[2] == mma}
            assert {("3x3", 1), ("3x3", 2)} <= got and {m for m, _ in got} == {"3x3", "up2", "s2"}
        assert {int(c[0][6:]) for c in SPLITS if c[2] == mma and c[1] == "3x3"} == set(SPLIT_TILES)
    yard = {}

    def yard_of(what, start, r64, r32, beta=1.0):
        b64, b32 = (start.double(), start) if beta else (torch.zeros_like(r64), torch.zeros_like(r32))
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), what
        yard[what] = float(((beta * b32 + ALPHA * r32).double() - (beta * b64 + ALPHA * r64)).abs().max())

    for case in TILE_CASES + PAIR_CASES:
        cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
        for cb in (5, 0):
            check_plan(case, plan(ops, case, cin_begin=cb))
        assert (8 + cout + M.hi_pad(8, cout) != 4 + cin + M.hi_pad(4, cin)) or g_offset(cin, cout) == 12
        dw64, db64, dw32, db32, count = tile_refs(mode, reflect, cin, cout, N, Ho, Wo, mma == BF16)
        k = dw64.shape[-1]
        beta = 0.0 if cls == "beta0" else 1.0
        for cb in (5, 0):
            yard_of("%s cb%d dw" % (tile_id(case), cb), K.rnd(cout, cin + 9, k, k, seed=1300 + cb)[:, cb:cb + cin], dw64, dw32, beta)
        yard_of(tile_id(case) + " db", K.rnd(cout, seed=1301), db64, db32, beta)
        empty = count == 0
        assert bool((dw64[empty] == 0).all()) and bool((dw32[empty] == 0).all())
        per_pair = empty[0, 0]
        assert bool((empty == per_pair).all())                     # (the same taps for every channel pair)
        if cls == "px1" and not reflect:                            # the planted empty sums: the taps that never meet the image
            assert int(per_pair.sum()) == {"3x3": 8, "up2": 0, "s2": 12}[mode]
        elif cls == "lineH" and mode == "3x3":
            assert bool(per_pair[0].all()) and bool(per_pair[2].all()) and not bool(per_pair[1].any())      # a 1-row image: the top and bottom taps
        elif cls == "lineW" and mode == "3x3":
            assert bool(per_pair[:, 0].all()) and bool(per_pair[:, 2].all()) and not bool(per_pair[:, 1].any())
        elif cls not in ("px1", "lineH", "lineW"):
            assert not bool(empty.any())
    for case in GROUP_CASES:
        cls, mode, mma, cin, cout, reflect, row, N, Ho, Wo = case
        check_plan(case, plan(ops, case, group_jobs=2))
        dw64, db64, dw32, db32, count = tile_refs(mode, reflect, 160, cout, N, Ho, Wo, mma == BF16)
        for lo in (0, 96):
            yard_of("%s group dw@%d" % (tile_id(case), lo), K.rnd(32, 160, 3, 3, seed=1320)[:, lo:lo + 64], dw64[:, lo:lo + 64], dw32[:, lo:lo + 64])
        yard_of(tile_id(case) + " group db", K.rnd(32, seed=1321), db64, db32)
    for k, cases, grid in ((3, THIN_CASES, 1024), (7, THIN7_CASES, 512)):
        for case in cases:
            cls, flip, cb, cs = case
            c = thin_case(k, cls, flip, cb, cs)
            beta = 0.0 if cls == "beta0" else 1.0
            yard_of("thin%d %s dw" % (k, thin_id(case)), c["dw0"], c["dw64"], c["dw32"], beta)
            if not (k == 7 and flip):
                yard_of("thin%d %s db" % (k, thin_id(case)), c["db0"], c["db64"], c["db32"], beta)
            empty = c["count"] == 0
            assert bool((c["dw64"][empty] == 0).all())
            N, H, W = c["big"].shape[0], c["big"].shape[2], c["big"].shape[3]
            if k == 3 and cls == "px1":
                assert int(empty[0, 0].sum()) == 8
            if k == 3 and cls == "lineH":
                assert bool(empty[0, 0, 0].all()) and bool(empty[0, 0, 2].all())
            if cls == "rows":                                       # two rows per workgroup, the last one short, a workgroup across two images
                rows, Hg = N * (H + (6 if (k == 7 and flip) else 0)), H + (6 if (k == 7 and flip) else 0)
                assert rows > grid and cdiv(rows, grid) == 2 and rows % 2 == 1 and Hg % 2 == 1
    zero = [what for what, v in yard.items() if not v > 0.0]
    assert not zero, zero
