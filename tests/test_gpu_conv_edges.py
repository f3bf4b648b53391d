"""Edge-shape parity of the forward and data-gradient convolution kernels behind tnr_conv_forward (csrc/conv_tile.hip, conv_x3w8.h,
conv_sweep.hip: conv3x3_d4 / conv_s2_d4, conv_wino.hip) and of the pooled / shuffled stores, the image-layer forms (TNR_CONV_3x3_C4 /
TNR_CONV_7x7_C4, conv_thin, conv_thin7) and the patch-matrix forms (conv_small, conv_col), against the plain F.conv2d /
F.conv_transpose2d statement of the layer and its epilogue in FLOAT64 on the CPU.  test_gpu_kernels.py runs every geometry at a few
friendly shapes under 2e-5 x (scale + 1); here the kernels run at the shapes at which such kernels go wrong, and the class is part of
the test id.  Before it launches, every case asserts through tnr_conv_launch_class (ops.conv_launch_class: the launcher's own
decision code, host only) the kernel, tile, grid and split-K factor it names.

Modes: 3x3 (forward packing), dg3 (TNR_PACK_DGRAD_3x3), s2 (4x4 stride 2), dgs2 (its data gradient; the tile space is the GRADIENT's
grid), up2 (nearest x2 + 3x3).  Forms: ops.conv(wino=False) gives conv_tile / conv3x3_x3w8 under f32, conv3x3_d4 / conv_s2_d4 where they
qualify under bf16x3 and bf16; wino=True gives conv3x3_wino (bf16x3).  e = the smallest ragged edge: 1 pixel, 2 for s2 / dgs2 / up2.
  px1      one output pixel (reflection and up2: 2 x 2; dgs2: a 1 x 1 gradient)
  lineH/W  H = e with W = tw + e, and H = th + e at the narrowest W that still picks the tile, for tw = 8, 16, 32 and the 32 x 16
           tile of the 32-cout layers (big_m: from 16 rows)
  one      one ragged tile: 3 x 5 (s2 / dgs2 / up2: 2 x 4)
  images   N = 3, two tile columns x three tile rows, the last column and row e wide / tall (the 32-wide tiles of conv_tile and
           x3w8: three columns -- at 33 columns conv_pick_tw takes a narrower tile); 32, 64 and 160 output channels
  oddC     the `images` shape at 100 -> 12, 36 -> 36, 20 -> 100 (s2: 20 -> 12): multiples of 4, not of 16 / 32
  sill     one below, at and one above every acceptance threshold (d4: W 32, H 8; wino: H, W 8; s2 / dgs2: 32 x 8 tile space;
           x3w8 and big_m: 16 rows at W = 32; split-K: 32 chunks, 192 tiles): the query shows the kernel change where the code says
  oddW     Winograd with odd H, W (the 2 x 2 output patch straddles the edge) at 9 x 9, 17 x 33, 33 x 17, zero and reflection padding
  wrap     more tiles than the persistent grid (cap x CUs workgroups; sized for 256 CUs) and not a multiple of it: the second trip
           of conv3x3_wino, conv3x3_d4 and conv_s2_d4 (forward and data gradient), ragged last tile row and column
  splitk   KinP = 512, 528 (33 chunks: uneven splits), 640, 1024 at 4 x 4, 8 x 8, 16 x 16; 191 and 192 tiles; Cout = 100; s2 at 128 / 132
  epi      bias + LeakyReLU + alpha, r1 over r1_ch < Cout channels with beta1 != 1, r2 with alpha2 != 1, a mask over [m_lo, m_hi) inside
           [0, Cout): three views at three offsets of three buffers of three widths; the noise multiplier with pix0 != 0; y += conv(x)

Traps in every case.  x and y are views at two different non-zero channel offsets of two buffers of different width; the other
channels hold NaN in the sources and a sentinel in the destination, which holds it bit for bit afterwards; the sources hold the same
bits afterwards.  y starts as NaN wherever the launch has no r1 on y.  The packed weights come from a fresh packer, every weight image
derived from them and the split-K workspace start as NaN.  Every launch runs twice and returns the same bits.  No comparison leaves
out an element (the mask is fp32 test data read with the same `> 0` on both sides).  A forward or data-gradient output is never an
empty sum at these shapes (counted with all-ones inputs: every output meets at least one tap; the stride-2 forms at one pixel meet
4 of 16 / 1 of 4), so test_inputs_and_references asserts the counts instead of a bit pattern.

Bounds, all the project's own.  err(device) against fp64 <= 2 x err(the same statement in fp32 on the CPU, epilogue included) + 2e-7 x
max|ref| (test_gpu_membound_kernels.yardstick) for f32, the direct bf16x3 forms and bf16 (there from the bf16-ROUNDED x and w; bias and
residuals un-rounded).  bf16x3 also: err <= 1.5 x err(the f32-matrix-core launch on the same inputs) + 2e-7 x scale; the Winograd form
3 x, and 2e-5 x (scale + 1) (test_gpu_conv_plan.py); its ratio to the CPU's fp32 statement is printed, not asserted.
For the tnr_conv_forward cases of section 1 (test_conv, test_inplace_accumulate, test_conv_shuffle2) the fp32 statement of the
yardstick is ONE fp32 chain per output in the order of the kernels' K loop (chain_sum): against torch's own fp32 convolution, which
sums in blocks, 25 of the first 185 device results missed the bound by up to 1.6 x (f32 and bf16x3 alike: images-dg3-160to32 5.41e-06
against 1.20e-06 at scale 4.9; the unsplit 512-channel layer 2.20e-05 against 2.27e-06 at scale 7.8), and the CPU chain has the device's
error (5.51e-06; 1.69e-05): the matrix-core accumulator IS one chain over K = taps x Cin, a legitimate order.  Split-K shortens the
chain to K / ksplit >= 1152 terms and still misses torch's bound (up to 1.42 x: splitk-3x3-528to64-8x8 f32), so those cases keep the
chain too.  Every test_conv case prints its ratio to torch's statement on a YARDSTICK-TORCH line; DESIGN.md 25 has the worst per class
and what breaking the chain in the kernels would take.  The forms of section 4 (C4 image layers, conv_thin / conv_thin7, conv_small /
conv_col) are held to torch's own fp32 statement, which they meet (worst 0.99: conv_thin 64 -> 3 at 17 x 17); they print the chain's
ratio on a YARDSTICK-CHAIN line.

Sections 3 and 4: ops.conv_pool2 (with and without the route map) at 8 x 8, 10 x 18 and the even wino `wrap` shape, against the fp64
max-pool of the fp64 convolution and bit for bit against ops.conv(wino=True) + maxpool2_fwd; ops.conv_shuffle2 at 8 x 32, 9 x 33 and the
d4 `wrap` shape with 256 couts; TNR_CONV_3x3_C4 / TNR_CONV_7x7_C4 (px1, lineH, lineW, images); ops.conv_thin / conv_thin7 forward and
dgrad (Cbig 16 / 32 / 64, Csmall 1 / 3; px1 or the smallest size the reflection accepts -- one below is refused --, lines, a 16 x 16 tile
plus one, 159 / 160 / 161 columns of conv_thin7c_kernel's segments at odd H; the destination's pad channels hold a finite sentinel, keep
it, and the stored bits equal those of a launch over zeros); ops.conv_small / ops.conv_col for the 4x4 stride-1 layers at 8, 16, 24,
4096 and 4104 output pixels, Cin 4 and 36.

test_inputs_and_references (no device) builds every case's inputs and references, asserts the class of every case in every arithmetic
through the query with the CU-dependent arithmetic at 256, that no yardstick denominator is zero, the tap counts, and the size of the
largest case.  The module has no module-level `pytestmark`: every other test carries the gpu mark itself.
"""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K
import test_gpu_membound_kernels as M

gpu = pytest.mark.gpu
NAN = float("nan")
D = torch.double
S32 = M.S32
ALPHA, BETA1, ALPHA2 = 0.75, 0.5, 0.25                      # (exact in fp32)
F32, BF16, X3 = 0, 1, 2                                     # hip.MMA_*
ARITH = {"f32": F32, "bf16": BF16, "bf16x3": X3}
CUS = 256                                                   # the CU count the `wrap` class is sized for
cache = functools.lru_cache(maxsize=None)


def cdiv(a, b):
    return -(-a // b)


def same_bits(a, b):
    """torch.equal on the bit patterns (the buffers hold NaN on purpose)"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def nan_outside(v):
    v.buf[..., :v.coff] = NAN
    v.buf[..., v.coff + v.C:] = NAN
    return v


# =====================================================================================================================
# 1. the cases of tnr_conv_forward
# =====================================================================================================================
class Case:
    """mode, launch channels cin -> cout (x.C -> y.C), N and the OUTPUT size Ho x Wo, the form asked for, the epilogue"""
    def __init__(self, cls, mode, cin, cout, N, Ho, Wo, wino=False, reflect=False, epi="lrelu", bf16=False, aim=None, note="", abi_splitk=False, **want):
        self.cls, self.mode, self.cin, self.cout, self.N, self.Ho, self.Wo = cls, mode, cin, cout, N, Ho, Wo
        self.wino, self.reflect, self.epi, self.bf16, self.note, self.abi_splitk = wino, reflect, epi, bf16, note, abi_splitk
        self.aim = aim                  # the arithmetic whose kernel the class is about (None: every one)
        self.want = want                # what the class names of the query's answer in that arithmetic, beyond expected()
        self.e = 2 if mode in ("s2", "up2") else 1          # in the tile space (dgs2: one gradient pixel = two output pixels)

    @property
    def id(self):
        return "%s-%s-%dto%d-N%d-%dx%d%s%s%s%s" % (self.cls, self.mode, self.cin, self.cout, self.N, self.Ho, self.Wo, "-wino" if self.wino else "",
                                                  "-reflect" if self.reflect else "", "" if self.epi == "lrelu" else "-" + self.epi, self.note)

    def in_size(self):
        return {"s2": (2 * self.Ho, 2 * self.Wo), "dgs2": (self.Ho // 2, self.Wo // 2), "up2": (self.Ho // 2, self.Wo // 2)}.get(self.mode, (self.Ho, self.Wo))

    def space(self):
        """the tile space: the output grid, for dgs2 the gradient's"""
        return self.in_size() if self.mode == "dgs2" else (self.Ho, self.Wo)

    def wshape(self):
        k = 4 if self.mode in ("s2", "dgs2") else 3
        return (self.cin, self.cout, k, k) if self.mode in ("dg3", "dgs2") else (self.cout, self.cin, k, k)

    def geom(self):
        return (self.mode, self.cin, self.cout, self.N, self.Ho, self.Wo, self.reflect)

    def arithmetics(self, mma_mode):
        return [mma_mode] + (["bf16"] if (mma_mode == "bf16x3" and self.bf16) else [])


def conv_mode(ops, c):
    return {"3x3": (ops.CONV_3x3, ops.PACK_FWD), "dg3": (ops.CONV_3x3, ops.PACK_DGRAD_3x3), "s2": (ops.CONV_4x4_S2, ops.PACK_FWD_S2D),
            "dgs2": (ops.DGRAD_4x4_S2, ops.PACK_DGRAD_S2), "up2": (ops.CONV_3x3_UP2, ops.PACK_FWD)}[c.mode]


def pick_tw(sw, sh):
    """the tile width of conv_tile as DESIGN.md states it: the 256-pixel shape with the fewest padded pixels, the widest on ties;
    16 and 32 only from that width on"""
    cands = [(cdiv(sw, tw) * tw * cdiv(sh, 256 // tw) * (256 // tw), -tw) for tw in (32, 16, 8) if tw == 8 or sw >= tw]
    return -min(cands)[1]


def want_ksplit(c, KinP, tiles):
    """the split-K factor as conv_tile.hip's comment states it (plain epilogues, < 192 tiles, >= 32 chunks, >= 8 chunks per split,
    512 workgroup slots, every split non-empty)"""
    nchunks = KinP // 16 * (4 if c.mode == "s2" else 1)
    if c.epi not in ("lrelu", "bias") or c.cout % 4 or c.mode == "dgs2" or tiles >= 192 or nchunks < 32:
        return 1
    want = min(cdiv(512, tiles), nchunks // 8)
    return 1 if want < 2 else cdiv(nchunks, cdiv(nchunks, want))


def expected(c, arith, KinP, KoutP):
    """what the documented thresholds say tnr_conv_forward launches for the case through ops.conv / conv_launch_desc"""
    sh, sw = c.space()
    H, W = c.in_size()
    x3, stream_arith = arith == "bf16x3", arith in ("bf16x3", "bf16")
    three = c.mode in ("3x3", "dg3")
    tw = pick_tw(sw, sh)
    nt = 2 if c.cout > 32 else 1
    big_m = three and nt == 1 and tw == 32 and sh >= 16
    th = (512 if big_m else 256) // tw
    par = 4 if c.mode == "dgs2" else 1
    tile = dict(kernel="tile", tw=tw, th=th, nt=nt, mt=4 if big_m else 2, tiles_x=cdiv(sw, tw), tiles_y=cdiv(sh, th), ncb=cdiv(c.cout, 32 * nt), cap=0)
    tile["tiles"] = tile["tiles_x"] * tile["tiles_y"] * tile["ncb"] * c.N * par
    ks = want_ksplit(c, KinP, tile["tiles"]) if (c.abi_splitk or (KinP >= 512 and c.N * c.Ho * c.Wo <= 16384)) else 1
    tile["ksplit"] = ks
    if ks > 1:
        tile["tiles"] *= ks
        return tile
    chans = c.cout % 64 == 0 and KoutP == c.cout and c.cin == KinP and c.cin % 16 == 0 and c.cin >= 32
    grid = lambda t, h: dict(tw=t, th=h, tiles_x=cdiv(sw, t), tiles_y=cdiv(sh, h), ncb=c.cout // 64, ksplit=1, tiles=cdiv(sw, t) * cdiv(sh, h) * (c.cout // 64) * c.N * par)
    if c.wino is not False and x3 and three and chans and H >= 8 and W >= 8:
        return dict(kernel="wino", nt=2, mt=0, cap=1, **grid(16, 16))
    if stream_arith and three and chans and W >= 32 and H >= 8:
        return dict(kernel="d4", nt=2, mt=2, cap=2, **grid(32, 8))
    if stream_arith and c.mode in ("s2", "dgs2") and chans and sw >= 32 and sh >= 8 and c.epi != "noise":
        return dict(kernel="s2_d4", nt=2, mt=2, cap=2, **grid(32, 8))
    if x3 and three and nt == 2 and tw == 32 and sh >= 16 and not c.reflect and c.cin == KinP and c.cin % 16 == 0:
        return dict(kernel="x3w8", tw=32, th=16, nt=2, mt=2, tiles_x=cdiv(sw, 32), tiles_y=cdiv(sh, 16), ncb=cdiv(c.cout, 64), ksplit=1, cap=0,
                    tiles=cdiv(sw, 32) * cdiv(sh, 16) * cdiv(c.cout, 64) * c.N)
    return tile


def out_of(mode, sh, sw):
    """output size of a tile space"""
    return (2 * sh, 2 * sw) if mode == "dgs2" else (sh, sw)


def lines(mode, cin, cout, tw, th, wmin, wline=None, **kw):
    """in the tile space: lineH: H = e, W = tw + e.  lineW: H = th + e at W = e (tw = 8) or the narrowest width that picks the tile.
    The 32 x 16 tile of the 32-cout layers exists from 16 rows on, and 32 columns win the pick over 16 only from 49 columns on
    (wline): its lineH is one tile row of 16 x 49"""
    e = 2 if mode in ("s2", "up2") else 1
    hmin = 16 if th == 16 and tw == 32 else e
    return [Case("lineH", mode, cin, cout, 1, *out_of(mode, hmin, wline or tw + e), note="-tw%d" % tw, tw=tw, th=th, tiles_x=2, tiles_y=1, **kw),
            Case("lineW", mode, cin, cout, 1, *out_of(mode, th + e, wmin), note="-tw%d" % tw, tw=tw, th=th, tiles_x=1, tiles_y=2, **kw)]


CASES = []
# px1
CASES += [Case("px1", "3x3", 32, 64, 1, 1, 1, bf16=True), Case("px1", "3x3", 32, 64, 1, 2, 2, reflect=True), Case("px1", "dg3", 64, 32, 1, 1, 1),
          Case("px1", "s2", 32, 64, 1, 1, 1, bf16=True), Case("px1", "dgs2", 64, 32, 1, 2, 2, bf16=True), Case("px1", "up2", 32, 64, 1, 2, 2)]
# lines: conv_tile at every width (96 couts: no weight-stream kernel takes them), the 32-cout tile, the stride-2 and x2 modes
for tw, th, wmin in ((8, 32, 1), (16, 16, 16), (32, 8, 32)):
    CASES += lines("3x3", 32, 96, tw, th, wmin, kernel="tile", bf16=(tw == 8))
CASES += lines("3x3", 64, 32, 32, 16, 32, wline=49, kernel="tile", mt=4, bf16=True)
CASES += lines("dg3", 96, 32, 32, 16, 32, wline=49, kernel="tile", mt=4)
for mode in ("s2", "dgs2", "up2"):
    CASES += lines(mode, 32, 96, 8, 32, 2 if mode != "dgs2" else 1, kernel="tile")
CASES += [Case("lineH", "s2", 64, 64, 1, 8, 34, aim="bf16x3", note="-s2d4", bf16=True, kernel="s2_d4", tiles_x=2, tiles_y=1),
          Case("lineW", "dgs2", 64, 64, 1, 18, 64, aim="bf16x3", note="-s2d4", kernel="s2_d4", tiles_x=1, tiles_y=2),
          Case("lineH", "3x3", 64, 64, 1, 8, 33, aim="bf16x3", note="-d4", bf16=True, kernel="d4", tiles_x=2, tiles_y=1),
          Case("lineW", "3x3", 64, 64, 1, 9, 32, aim="bf16x3", note="-d4", kernel="d4", tiles_x=1, tiles_y=2),
          Case("lineH", "3x3", 64, 64, 1, 8, 17, wino=True, aim="bf16x3", kernel="wino", tiles_x=2, tiles_y=1),
          Case("lineW", "3x3", 64, 64, 1, 17, 8, wino=True, aim="bf16x3", kernel="wino", tiles_x=1, tiles_y=2)]
# one ragged tile
CASES += [Case("one", "3x3", 32, 64, 1, 3, 5, bf16=True), Case("one", "3x3", 32, 64, 1, 3, 5, reflect=True), Case("one", "dg3", 64, 32, 1, 3, 5),
          Case("one", "s2", 32, 64, 1, 2, 4, bf16=True), Case("one", "dgs2", 64, 32, 1, 4, 8), Case("one", "up2", 32, 64, 1, 4, 8)]
# images: N = 3, 2 x 3 tiles, the last column and row e wide / tall.  The 32-wide tiles of conv_tile and x3w8 get 3 x 3 at 65 columns:
# at 33 columns and three tile rows conv_pick_tw covers fewer padded pixels with a narrower tile
IMG, IMG3 = dict(tiles_x=2, tiles_y=3), dict(tiles_x=3, tiles_y=3)
CASES += [Case("images", "3x3", 64, 64, 3, 17, 65, aim="f32", kernel="tile", tw=32, th=8, nt=2, **IMG3),
          Case("images", "3x3", 64, 64, 3, 17, 33, aim="bf16x3", bf16=True, note="-d4", kernel="d4", **IMG),
          Case("images", "3x3", 64, 64, 3, 17, 33, aim="bf16x3", reflect=True, note="-d4", kernel="d4", **IMG),
          Case("images", "3x3", 64, 32, 3, 33, 65, kernel="tile", mt=4, nt=1, bf16=True, **IMG3),
          Case("images", "3x3", 64, 32, 3, 33, 17, kernel="tile", tw=16, th=16, nt=1, mt=2, **IMG),
          Case("images", "3x3", 32, 160, 3, 17, 65, aim="f32", kernel="tile", tw=32, nt=2, ncb=3, **IMG3),
          Case("images", "3x3", 32, 160, 3, 33, 65, aim="bf16x3", note="-x3w8", kernel="x3w8", ncb=3, **IMG3),
          Case("images", "3x3", 64, 64, 3, 33, 17, wino=True, aim="bf16x3", kernel="wino", **IMG),
          Case("images", "3x3", 64, 64, 3, 33, 17, wino=True, reflect=True, aim="bf16x3", kernel="wino", **IMG),
          Case("images", "dg3", 64, 64, 3, 17, 33, aim="bf16x3", bf16=True, kernel="d4", **IMG),
          Case("images", "dg3", 160, 32, 3, 33, 65, kernel="tile", mt=4, **IMG3),
          Case("images", "s2", 64, 64, 3, 18, 34, aim="bf16x3", bf16=True, kernel="s2_d4", **IMG),
          Case("images", "s2", 32, 160, 3, 18, 66, kernel="tile", tw=32, ncb=3, **IMG3),
          Case("images", "dgs2", 64, 64, 3, 34, 66, aim="bf16x3", bf16=True, kernel="s2_d4", **IMG),
          Case("images", "dgs2", 160, 32, 3, 34, 130, kernel="tile", tw=32, nt=1, **IMG3),
          Case("images", "up2", 64, 64, 3, 18, 66, kernel="tile", tw=32, **IMG3), Case("images", "up2", 32, 160, 3, 18, 66, kernel="tile", tw=32, ncb=3, **IMG3)]
# oddC
CASES += [Case("oddC", "3x3", 100, 12, 3, 33, 65, kernel="tile", tw=32, mt=4, bf16=True, **IMG3), Case("oddC", "3x3", 36, 36, 3, 17, 65, kernel="tile", tw=32, **IMG3),
          Case("oddC", "3x3", 20, 100, 3, 17, 65, aim="f32", kernel="tile", tw=32, ncb=2, **IMG3), Case("oddC", "dg3", 36, 36, 3, 17, 65, kernel="tile", tw=32, **IMG3),
          Case("oddC", "s2", 20, 12, 3, 18, 66, kernel="tile", tw=32, bf16=True, **IMG3), Case("oddC", "dgs2", 36, 20, 3, 34, 130, kernel="tile", tw=32, **IMG3),
          Case("oddC", "3x3", 36, 36, 3, 17, 65, reflect=True, kernel="tile", tw=32, **IMG3), Case("oddC", "3x3", 36, 36, 3, 33, 17, kernel="tile", tw=16, **IMG)]
# sills (aim: the arithmetic in which the threshold decides)
for W in (31, 32, 33):
    CASES.append(Case("sill", "3x3", 32, 64, 1, 8, W, aim="bf16x3", bf16=True, note="-d4W", kernel="d4" if W >= 32 else "tile"))
for H in (7, 8, 9):
    CASES.append(Case("sill", "3x3", 32, 64, 1, H, 32, aim="bf16x3", note="-d4H", kernel="d4" if H >= 8 else "tile"))
for H, W in ((7, 7), (7, 9), (9, 7), (8, 8), (9, 9)):       # (asked through the process policy: wino=True refuses a launch the library declines)
    CASES.append(Case("sill", "3x3", 32, 64, 1, H, W, wino=None, aim="bf16x3", note="-wino", kernel="wino" if min(H, W) >= 8 else "tile"))
for mode in ("s2", "dgs2"):
    for Ws in (30, 32, 34):
        k = 2 if mode == "dgs2" else 1
        CASES.append(Case("sill", mode, 64, 64, 1, 8 * k, Ws * k, aim="bf16x3", bf16=True, note="-space%d" % Ws, kernel="s2_d4" if Ws >= 32 else "tile"))
    CASES.append(Case("sill", mode, 64, 64, 1, 6 * (2 if mode == "dgs2" else 1), 32 * (2 if mode == "dgs2" else 1), aim="bf16x3", note="-spaceH6", kernel="tile"))
for H in (15, 16, 17):
    CASES.append(Case("sill", "3x3", 16, 64, 1, H, 32, aim="bf16x3", note="-x3w8", kernel="x3w8" if H >= 16 else "tile"))
    CASES.append(Case("sill", "3x3", 64, 32, 1, H, 32, note="-bigm", kernel="tile", mt=4 if H >= 16 else 2, th=16 if H >= 16 else 8))
# oddW
for H, W in ((9, 9), (17, 33), (33, 17)):
    for refl in (False, True):
        for cin, cout in ((32, 64), (48, 128)):
            CASES.append(Case("oddW", "3x3", cin, cout, 2, H, W, wino=True, reflect=refl, aim="bf16x3", kernel="wino"))
# wrap: the second trip of the persistent grids at 256 CUs
CASES += [Case("wrap", "3x3", 32, 256, 1, 65, 193, wino=True, aim="bf16x3", kernel="wino", tiles=260, cap=1),
          Case("wrap", "3x3", 32, 256, 1, 65, 193, wino=True, epi="full", aim="bf16x3", kernel="wino", tiles=260, cap=1),
          Case("wrap", "3x3", 32, 256, 1, 65, 193, wino=True, epi="noise", aim="bf16x3", kernel="wino", tiles=260, cap=1),
          Case("wrap", "3x3", 32, 256, 3, 49, 113, wino=True, aim="bf16x3", kernel="wino", tiles=384, cap=1),       # (the second trip lies in another image)
          Case("wrap", "3x3", 32, 256, 2, 257, 33, aim="bf16x3", bf16=True, kernel="d4", tiles=528, cap=2),
          Case("wrap", "3x3", 32, 256, 2, 257, 33, epi="full", aim="bf16x3", kernel="d4", tiles=528, cap=2),
          Case("wrap", "3x3", 32, 256, 2, 257, 33, epi="noise", aim="bf16x3", kernel="d4", tiles=528, cap=2),
          Case("wrap", "dg3", 32, 256, 2, 257, 33, reflect=False, aim="bf16x3", kernel="d4", tiles=528, cap=2),
          Case("wrap", "s2", 64, 256, 2, 258, 34, aim="bf16x3", bf16=True, kernel="s2_d4", tiles=528, cap=2),
          Case("wrap", "s2", 64, 256, 2, 258, 34, epi="full", aim="bf16x3", kernel="s2_d4", tiles=528, cap=2),
          Case("wrap", "dgs2", 64, 256, 2, 132, 68, aim="bf16x3", bf16=True, kernel="s2_d4", tiles=576, cap=2),
          Case("wrap", "dgs2", 64, 256, 2, 132, 68, epi="full", aim="bf16x3", kernel="s2_d4", tiles=576, cap=2)]
# split-K (ksplit, and the chunks of the last split against the others: `even`)
SPLITS = {512: (4, True), 528: (4, False), 640: (5, True), 1024: (8, True)}
for cin, (ks, even) in SPLITS.items():
    for side in (4, 8, 16):
        CASES.append(Case("splitk", "3x3", cin, 64, 2, side, side, kernel="tile", ksplit=ks, even=even, bf16=(side == 8)))
CASES += [Case("splitk", "3x3", 512, 64, 191, 4, 4, note="-tiles191", kernel="tile", ksplit=3, even=False),
          Case("splitk", "3x3", 512, 64, 192, 4, 4, note="-tiles192", kernel="tile", ksplit=1),
          Case("splitk", "3x3", 496, 64, 2, 8, 8, note="-chunks31", kernel="tile", ksplit=1),
          Case("splitk", "3x3", 528, 100, 2, 8, 8, note="-padC", kernel="tile", ksplit=4, even=False, ncb=2),
          Case("splitk", "dg3", 528, 64, 2, 8, 8, kernel="tile", ksplit=4, even=False),
          Case("splitk", "s2", 128, 64, 2, 8, 8, abi_splitk=True, kernel="tile", ksplit=4, even=True),
          Case("splitk", "s2", 132, 64, 2, 8, 8, abi_splitk=True, kernel="tile", ksplit=4, even=True, note="-KinP144"),
          Case("splitk", "s2", 164, 64, 2, 8, 8, abi_splitk=True, kernel="tile", ksplit=5, even=False, note="-KinP176")]
# epilogue operands at ragged tile edges, in every form that has an epilogue
CASES += [Case("epi", "3x3", 64, 32, 3, 33, 17, epi="full", kernel="tile", nt=1, mt=2, **IMG),
          Case("epi", "3x3", 64, 32, 3, 33, 65, epi="full", kernel="tile", nt=1, mt=4, bf16=True, **IMG3),
          Case("epi", "3x3", 32, 96, 3, 17, 65, epi="full", aim="f32", kernel="tile", tw=32, nt=2, **IMG3),
          Case("epi", "3x3", 16, 64, 3, 33, 65, epi="full", aim="bf16x3", kernel="x3w8", **IMG3),
          Case("epi", "3x3", 64, 64, 3, 17, 33, epi="full", aim="bf16x3", bf16=True, kernel="d4", **IMG),
          Case("epi", "3x3", 64, 64, 3, 17, 33, epi="noise", aim="bf16x3", kernel="d4", **IMG),
          Case("epi", "3x3", 64, 64, 3, 33, 17, epi="full", wino=True, aim="bf16x3", kernel="wino", **IMG),
          Case("epi", "3x3", 64, 64, 3, 33, 17, epi="full", wino=True, reflect=True, aim="bf16x3", kernel="wino", **IMG),
          Case("epi", "s2", 64, 64, 3, 18, 34, epi="full", aim="bf16x3", bf16=True, kernel="s2_d4", **IMG),
          Case("epi", "dgs2", 64, 64, 3, 34, 66, epi="full", aim="bf16x3", kernel="s2_d4", **IMG),
          Case("epi", "up2", 32, 96, 3, 18, 66, epi="full", kernel="tile", tw=32, **IMG3)]
assert len({c.id for c in CASES}) == len(CASES)


def rnd_nonzero_yard(make, seeds=256):
    """oracle.detrand draws from a 2^-23 grid, so a tiny sum can round exactly in fp32: redraw the start value (the bias) until the
    fp32 statement differs from fp64 (the yardstick's denominator)"""
    for draw in range(seeds):
        out = make(draw)
        if float((out[1].double() - out[0]).abs().max()) > 0.0:
            return out
    raise AssertionError("no draw with a non-zero fp32 error")


def conv_sum(c, x, w):
    """the plain statement of the layer without bias, in the dtype of x"""
    if c.mode == "3x3":
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w) if c.reflect else F.conv2d(x, w, padding=1)
    if c.mode == "dg3":
        return F.conv_transpose2d(x, w, padding=1)
    if c.mode == "s2":
        return F.conv2d(x, w, stride=2, padding=1)
    if c.mode == "dgs2":
        return F.conv_transpose2d(x, w, stride=2, padding=1)
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)


def chain_sum(c, x, w):
    """The same sum in fp32 on the CPU as ONE chain per output, in the order of the kernels' K loop (csrc/conv_body.h: input chunks of
    16 channels outermost, the taps of a chunk, its channels): acc = fp32(acc + x * w), term after term.  torch's own fp32 convolution
    sums in blocks, and a chain of K = taps x Cin terms drifts further: this is the fp32 statement the yardstick holds
    the direct kernels to, torch's is printed beside it."""
    N, Ho, Wo = c.N, c.Ho, c.Wo
    acc = torch.zeros(N, c.cout, Ho, Wo)
    if c.mode == "dgs2":            # per output parity the two taps per axis that meet it: oy = 2 iy - 1 + ky
        gp = F.pad(x, (1, 1, 1, 1))
        H, W = x.shape[2:]
        taps = {0: ((1, 0), (3, -1)), 1: ((0, 1), (2, 0))}          # parity -> (k, offset of the gradient pixel)
        for c0 in range(0, c.cin, 16):
            for py in (0, 1):
                for px in (0, 1):
                    sub = acc[:, :, py::2, px::2]
                    for ky, dy in taps[py]:
                        for kx, dx in taps[px]:
                            for ci in range(c0, min(c0 + 16, c.cin)):
                                sub.addcmul_(gp[:, ci:ci + 1, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W], w[ci, :, ky, kx].view(1, -1, 1, 1))
        return acc
    if c.mode == "dg3":             # the data gradient as the forward convolution it is: taps flipped, channels transposed
        w = w.flip(2, 3).transpose(0, 1)
    if c.mode == "up2":
        x = F.interpolate(x, scale_factor=2, mode="nearest")
    k, s_, = w.shape[2], 2 if c.mode == "s2" else 1
    xp = F.pad(x, (1, 1, 1, 1), mode="reflect") if c.reflect else F.pad(x, (1, 1, 1, 1))
    for c0 in range(0, c.cin, 16):
        for ky in range(k):
            for kx in range(k):
                for ci in range(c0, min(c0 + 16, c.cin)):
                    acc.addcmul_(xp[:, ci:ci + 1, ky:ky + s_ * Ho:s_, kx:kx + s_ * Wo:s_], w[:, ci, ky, kx].view(1, -1, 1, 1))
    return acc


def chain_taps(xp, w, Ho, Wo, acc=None):
    """one fp32 chain per output over an already padded input, taps outermost, then channels: the order of the patch-matrix GEMM
    (K = (tap, channel)) and of the vector-ALU kernels"""
    acc = torch.zeros(xp.shape[0], w.shape[0], Ho, Wo) if acc is None else acc
    for ky in range(w.shape[2]):
        for kx in range(w.shape[3]):
            for ci in range(w.shape[1]):
                acc.addcmul_(xp[:, ci:ci + 1, ky:ky + Ho, kx:kx + Wo], w[:, ci, ky, kx].view(1, -1, 1, 1))
    return acc


def mask_range(cout):
    lo = 4 if cout <= 32 else 16
    return lo, cout - (4 if cout <= 32 else 16)


def r1_channels(cout):
    return cout // 2 if (cout // 2) % 4 == 0 else cout // 2 + 2


def epilogue(c, s, t, dtype, field=None):
    """act(sum + bias) x alpha; + beta1 x r1 over r1_ch channels; x noise (pos 1); x alpha2 + r2; the mask gate over [m_lo, m_hi)"""
    v = F.leaky_relu(s + t["bias"].to(dtype).view(1, -1, 1, 1), S32) * ALPHA
    if c.epi in ("full", "noise"):
        ch = r1_channels(c.cout)
        v[:, :ch] = v[:, :ch] + BETA1 * t["r1"].to(dtype)[:, :ch]
    if c.epi == "noise":
        v = v * field.to(dtype)
    if c.epi == "full":
        v = v * ALPHA2 + t["r2"].to(dtype)
        lo, hi = mask_range(c.cout)
        gate = torch.where(t["mask"][:, lo:hi] > 0, torch.ones((), dtype=dtype), torch.full((), S32, dtype=dtype))
        v[:, lo:hi] = v[:, lo:hi] * gate
    return v


def inputs(c):
    return dict(_inputs(c.geom()))


def sums(c, rounded):
    return _sums(c.geom(), rounded)


@cache
def _inputs(geom):
    c = Case("", *geom[:6], reflect=geom[6], epi="full")
    H, W = c.in_size()
    sd = 2000 + 7 * c.cin + 3 * c.cout + c.Ho
    t = dict(x=K.rnd(c.N, c.cin, H, W, seed=sd), w=K.rnd(*c.wshape(), seed=sd + 1, lo=-0.1, hi=0.1))
    # (every epilogue's operands: the inputs are shared between the epilogue variants of a shape)
    t.update(r1=K.rnd(c.N, c.cout, c.Ho, c.Wo, seed=sd + 3), r2=K.rnd(c.N, c.cout, c.Ho, c.Wo, seed=sd + 4), mask=K.rnd(c.N, c.cout, c.Ho, c.Wo, seed=sd + 5))
    return t


@cache
def _sums(geom, rounded):
    """the convolution sums in fp64, in fp32 as one chain, in fp32 as torch sums them (rounded: from the bf16-rounded x and w), and the
    number of taps every output meets"""
    c = Case("", *geom[:6], reflect=geom[6])
    t = _inputs(geom)
    x, w = (K._bf(t["x"]), K._bf(t["w"])) if rounded else (t["x"], t["w"])
    count = conv_sum(c, torch.ones(1, 1, *x.shape[2:], dtype=D), torch.ones(1, 1, *w.shape[2:], dtype=D))
    return conv_sum(c, x.double(), w.double()), chain_sum(c, x, w), conv_sum(c, x, w), count


def refs(c, rounded, field=None):
    """-> inputs with the bias, ref64, ref32 (one chain; epilogue included), err(torch's fp32 statement).  The noise field is test
    data: drawn by tnr_gauss_mult, a kernel of its own, it enters the statements as the fp32 tensor it is (so those references are
    not kept)"""
    assert (field is not None) == (c.epi == "noise")
    if (c, rounded) in _REFS:
        return _REFS[(c, rounded)]
    t = inputs(c)
    s64, s32, storch, _ = sums(c, rounded)

    def make(draw):
        t["bias"] = K.rnd(c.cout, seed=2900 + c.cout + 16 * draw)
        return epilogue(c, s64, t, D, field), epilogue(c, s32, t, torch.float32, field)
    r64, r32 = rnd_nonzero_yard(make)
    out = (t, r64, r32, float((epilogue(c, storch, t, torch.float32, field).double() - r64).abs().max()))
    if field is None:
        _REFS[(c, rounded)] = out
    return out


_REFS = {}


class Stub:
    """what _conv_desc and conv_plan read of a View, a packed weight or a tensor: enough for the host-only query, no memory behind it"""
    def __init__(self, N=0, H=0, W=0, C=0, ctot=0, coff=0):
        self.N, self.H, self.W, self.C, self.ctot, self.coff, self.pixels = N, H, W, C, ctot, coff, N * H * W

    def c(self):
        from trainner_amd import hip
        return hip.CView(64, self.ctot, self.coff)          # (a non-null placeholder: the query dereferences nothing)

    def data_ptr(self):
        return 64


def y_offset(c):
    """8, or 12 where the two buffers would otherwise be equally wide"""
    return 8 if 8 + c.cout + M.hi_pad(8, c.cout) != 4 + c.cin + M.hi_pad(4, c.cin) else 12


def epi_kwargs(ops, c, bias, r1=None, r2=None, mask=None, noise=None):
    kw = dict(bias=bias, act=ops.ACT_LRELU, slope=0.2, alpha=ALPHA, reflect=c.reflect)
    if c.epi in ("full", "noise"):
        kw.update(r1=r1, r1_ch=r1_channels(c.cout), beta1=BETA1)
    if c.epi == "full":
        lo, hi = mask_range(c.cout)
        kw.update(r2=r2, alpha2=ALPHA2, mask=mask, m_lo=lo, m_hi=hi, m_slope=0.2)
    if c.epi == "noise":
        kw.update(noise=noise)
    return kw


NOISE_PIX0 = 1234


def the_noise(ops):
    return ops.Noise(0.1, ops.noise_key(25, 2, 3), pos=1, pix0=NOISE_PIX0)


def describe(ops, c, arith, xv, wp, yv, kw):
    """the descriptor ops.conv hands tnr_conv_forward for the case, without touching memory, and the query's answer for it.
    abi_splitk: the C entry splits any launch its conv_ksplit accepts; ops.conv offers a workspace from KinP = 512 on, so the
    stride-2 cases attach one themselves"""
    from trainner_amd import hip
    lib = hip.load()
    mode, _ = conv_mode(ops, c)
    prev = ops.MMA, ops.WINO_MIN_CIN, ops.WINO_MIN_PIXELS
    ops.MMA = ARITH[arith]
    if c.wino is None:
        ops.WINO_MIN_CIN, ops.WINO_MIN_PIXELS = 0, 0
    try:
        form, d = ops.conv_launch_desc(xv, wp, yv, mode, c.wino, 0, kw, dry=True)
        if c.abi_splitk:
            need = lib.tnr_conv_workspace_bytes(ctypes.byref(d))
            assert need > 0 and not d.ws
            d.wq, d.wq_bytes, d.ws, d.ws_bytes = None, 0, 64, need
        return d, ops.conv_launch_class(d)
    finally:
        ops.MMA, ops.WINO_MIN_CIN, ops.WINO_MIN_PIXELS = prev


def check_class(c, arith, q, KinP, KoutP, cus=CUS):
    """the query's answer against the documented thresholds, and what the class names on top of them"""
    exp = expected(c, arith, KinP, KoutP)
    assert q == exp, (c.id, arith, q, exp)
    if c.aim not in (None, arith):
        return
    for k, v in c.want.items():
        if k != "even":
            assert q[k] == v, (c.id, arith, k, q[k], v)
    sh, sw = c.space()
    if c.cls in ("images", "oddC") or (c.cls == "epi" and "tiles_x" in c.want):
        assert c.N == 3 and sw - (q["tiles_x"] - 1) * q["tw"] == c.e and sh - (q["tiles_y"] - 1) * q["th"] == c.e, (c.id, q)
    if c.cls == "oddC":
        assert c.cin % 4 == 0 and c.cout % 4 == 0 and (c.cin % 16 or c.cout % 32)
    if c.cls == "wrap":
        grid = q["cap"] * cus
        assert q["cap"] > 0 and q["tiles"] > grid and q["tiles"] % grid != 0, "%s: %d tiles do not wrap a grid of %d workgroups unevenly" % (c.id, q["tiles"], grid)
        assert sw % q["tw"] != 0 and sh % q["th"] != 0
    if c.cls == "splitk" and "even" in c.want:
        nchunks = KinP // 16 * (4 if c.mode == "s2" else 1)
        per = cdiv(nchunks, q["ksplit"])
        assert (nchunks - (q["ksplit"] - 1) * per == per) == c.want["even"] and nchunks - (q["ksplit"] - 1) * per > 0, (c.id, nchunks, per)


def trap_images(monkeypatch, ops):
    """every weight image derived from packed weights (the pre-split stream, the Winograd transform) starts as NaN: the entry is
    planted before ops._stream_image looks, which then packs into it because its generation is not the packer's"""
    orig = ops._stream_image

    def planted(owner, attr, key, need, dev, pack):
        assert owner is not None, "the cases pack through a fresh WeightPacker"
        images = owner.__dict__.setdefault(attr, {})
        if key not in images:
            images[key] = [torch.full((need // 4,), NAN, dtype=torch.float32, device=dev), None]
        return orig(owner, attr, key, need, dev, pack)
    monkeypatch.setattr(ops, "_stream_image", planted)


class ws_trap:
    """NaN into the ops.WS buffers a launch will ask for; on the way out: every buffer in `must` WAS asked for, and whatever was asked
    for under a trapped name was the very buffer that had been filled (not a new or renamed one)"""
    def __init__(self, ops, sizes, dev, must=()):
        self.ops, self.must, self.asked, self.ptr = ops, must, {}, {}
        for name, nbytes in sizes.items():
            buf = ops.WS.get(name, nbytes, dev)
            buf.view(torch.float32).fill_(NAN)
            self.ptr[name] = buf.data_ptr()

    def __enter__(self):
        orig = type(self.ops.WS).get

        def get(name, nbytes, device):
            buf = orig(self.ops.WS, name, nbytes, device)
            self.asked[name] = buf.data_ptr()
            return buf
        self.ops.WS.get = get
        return self

    def __exit__(self, *exc):
        del self.ops.WS.get
        if exc[0] is None:
            assert set(self.must) <= set(self.asked), "the launch did not ask for %s" % (set(self.must) - set(self.asked))
            for name, ptr in self.asked.items():
                assert name not in self.ptr or ptr == self.ptr[name], "%s: the launch used another buffer than the one filled with NaN" % name
        return False


def run_case(ops, c, arith, t, once=False, check=True):
    """two launches from a fresh start each -> the y view as NCHW (on the device); every trap of the module's docstring"""
    from trainner_amd import hip
    mode, kind = conv_mode(ops, c)
    ops.MMA = ARITH[arith]
    if c.wino is None:
        ops.WINO_MIN_CIN, ops.WINO_MIN_PIXELS = 0, 0
    xv = nan_outside(M.win(t["x"], 4))
    srcs = [xv]
    r1 = r2 = mk = None
    if c.epi in ("full", "noise"):
        r1, r2, mk = (nan_outside(M.win(t[n], lo)) for n, lo in (("r1", 12), ("r2", 16), ("mask", 20)))
        assert len({v.ctot for v in (r1, r2, mk)}) == 3
        srcs += [r1, r2, mk]
    bias = t["bias"].to(K.DEV)
    kw = epi_kwargs(ops, c, bias, r1, r2, mk, the_noise(ops) if c.epi == "noise" else None)
    snaps = [v.buf.clone() for v in srcs]
    yo = y_offset(c)
    outs = []
    for rep in range(1 if once else 2):
        yv = M.blank(c.N, c.Ho, c.Wo, c.cout, yo, inner=NAN)
        assert yv.ctot != xv.ctot and yv.coff != xv.coff
        wp, _keep = K.pack(ops, t["w"].to(K.DEV), kind)
        d, q = describe(ops, c, arith, xv, wp, yv, kw)
        if check:
            check_class(c, arith, q, wp.KinP, wp.KoutP, torch.cuda.get_device_properties(0).multi_processor_count if c.cls == "wrap" else CUS)
        name = "splitk@%x" % hip.stream()
        with ws_trap(ops, {name: d.ws_bytes} if d.ws_bytes > 0 else {}, xv.buf.device, must=[name] if d.ws_bytes > 0 else []):
            if c.abi_splitk:            # the descriptor of describe() with the real addresses
                ws = ops.WS.get(name, d.ws_bytes, xv.buf.device)
                ops._conv_desc(d, xv, wp, yv, mode, **kw)
                d.ws, d.ws_bytes = ws.data_ptr(), ws.numel() * 8
                hip.check(hip.load().tnr_conv_forward(ctypes.byref(d), hip.stream()), "conv_forward")
            else:
                ops.conv(xv, wp, yv, mode=mode, wino=c.wino, **kw)
            torch.cuda.synchronize()
        outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
        outside[yo:yo + c.cout] = False
        assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT)), "%s: channels outside the y view changed" % c.id
        outs.append(M.got(yv))
    assert same_bits(outs[0], outs[-1]), "%s: two launches on the same inputs differ" % c.id
    for v, s in zip(srcs, snaps):
        assert same_bits(v.buf, s), "%s: a source buffer changed" % c.id
    return outs[0], q


def held_x3(what, got_x3, got_f32, ref64, factor):
    """the project's own bf16x3 criterion: err <= factor x err(fp32-matrix-core launch on the same inputs) + 2e-7 x scale"""
    e64 = ref64.to(got_x3.device)
    scale = float(ref64.abs().max())
    e_x3, e_f32 = float((got_x3.double() - e64).abs().max()), float((got_f32.double() - e64).abs().max())
    bound = factor * e_f32 + 2e-7 * scale
    print("YARDSTICK-X3 %-60s x3 %.3e  f32-mma %.3e  scale %.3e  x3/bound %.3f" % (what, e_x3, e_f32, scale, e_x3 / bound if bound else float("inf")))
    assert e_x3 <= bound, (what, e_x3, e_f32, scale)


def device_field(ops, c):
    """the noise multiplier of the case's launch as tnr_gauss_mult draws it, NCHW on the CPU"""
    m = torch.empty((c.N, c.Ho, c.Wo, c.cout), device=K.DEV)
    ops.gauss_mult(ops.View(m), None, the_noise(ops))
    torch.cuda.synchronize()
    return m.permute(0, 3, 1, 2).contiguous().cpu()


def check_case(c, mma_mode, monkeypatch):
    from trainner_amd import ops
    for name in ("MMA", "WINO_MIN_CIN", "WINO_MIN_PIXELS"):
        monkeypatch.setattr(ops, name, getattr(ops, name))          # (run_case sets them: restored after the test)
    trap_images(monkeypatch, ops)
    field = device_field(ops, c) if c.epi == "noise" else None
    for arith in c.arithmetics(mma_mode):
        t, r64, r32, e_torch = refs(c, arith == "bf16", field)
        got, q = run_case(ops, c, arith, t)
        what = "%s %s %s" % (c.id, arith, q["kernel"])
        assert bool(torch.isfinite(got).all()), what
        if q["kernel"] == "wino":
            scale = float(r64.abs().max())
            e_dev = float((got.double() - r64.to(got.device)).abs().max())
            print("YARDSTICK-TORCH %-60s dev %.3e  torch-fp32 %.3e  dev/(2 torch + 2e-7 scale) %.3f (not asserted)" % (what, e_dev, e_torch, e_dev / (2 * e_torch + 2e-7 * scale)))
            assert e_dev <= 2e-5 * (scale + 1.0), (what, e_dev, scale)
        else:
            e_dev, e_32 = M.yardstick(what, got, r64, r32)
            print("YARDSTICK-TORCH %-60s dev %.3e  torch-fp32 %.3e  dev/(2 torch + 2e-7 scale) %.3f (not asserted)"
                  % (what, e_dev, e_torch, e_dev / (2 * e_torch + 2e-7 * float(r64.abs().max()))))
        if arith == "bf16x3":
            got_f32, _ = run_case(ops, c, "f32", t, once=True, check=False)
            held_x3(what, got, got_f32, r64, 3.0 if q["kernel"] == "wino" else 1.5)


@gpu
@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_conv(c, mma_mode, monkeypatch):
    check_case(c, mma_mode, monkeypatch)


@gpu
@pytest.mark.parametrize("shape", [(3, 17, 33, 32, 96), (2, 33, 33, 32, 32), (2, 17, 33, 64, 64)], ids=lambda s: "N%d-%dx%d-%dto%d" % s)
def test_inplace_accumulate(shape, mma_mode, monkeypatch):
    """y += conv(x) where x and y are disjoint channel windows of ONE buffer (the dense-block gradient layout) at a ragged shape: r1 is
    y itself, so y starts as data; the channels of the buffer outside both windows hold NaN and keep their bits"""
    from trainner_amd import ops
    trap_images(monkeypatch, ops)
    N, H, W, cin, cout = shape
    x, y0, w = K.rnd(N, cin, H, W, seed=2500 + cin), K.rnd(N, cout, H, W, seed=2501), K.rnd(cout, cin, 3, 3, seed=2502, lo=-0.1, hi=0.1)
    r64 = y0.double() + F.conv2d(x.double(), w.double(), padding=1)
    r32 = y0 + chain_sum(Case("", "3x3", cin, cout, N, H, W), x, w)
    runs = []
    for rep in range(2):
        buf = torch.full((N, H, W, 4 + cout + 8 + cin + 4), NAN)
        buf[..., 4:4 + cout] = y0.permute(0, 2, 3, 1)
        buf[..., 12 + cout:12 + cout + cin] = x.permute(0, 2, 3, 1)
        buf = buf.to(K.DEV)
        start = buf.clone()
        yv, xv = ops.View(buf, 4, cout), ops.View(buf, 12 + cout, cin)
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_FWD)
        ops.conv(xv, wp, yv, wino=False, r1=yv, beta1=1.0)
        torch.cuda.synchronize()
        keep = torch.ones(buf.shape[3], dtype=torch.bool, device=K.DEV)
        keep[4:4 + cout] = False
        assert same_bits(buf[..., keep], start[..., keep]), "channels outside the y window changed"
        runs.append(M.got(yv))
    assert same_bits(runs[0], runs[1])
    M.yardstick("inplace N%d-%dx%d-%dto%d %s" % (shape + (mma_mode,)), runs[0], r64, r32)


# =====================================================================================================================
# 2. the device-free self-check
# =====================================================================================================================
def stub_launch(ops, c, arith):
    """the query for stubs of the case's views: the geometry run_case builds, no memory"""
    H, W = c.in_size()
    _, kind = conv_mode(ops, c)
    co, ci, kh, kw_ = c.wshape()
    KoutP, KinP, _n = ops.pack_dims(co, ci, kh, kw_, kind)
    xv = Stub(c.N, H, W, c.cin, 4 + c.cin + M.hi_pad(4, c.cin), 4)
    yo = y_offset(c)
    yv = Stub(c.N, c.Ho, c.Wo, c.cout, yo + c.cout + M.hi_pad(yo, c.cout), yo)
    views = [Stub(c.N, c.Ho, c.Wo, c.cout, lo + c.cout + M.hi_pad(lo, c.cout), lo) for lo in (12, 16, 20)]
    kw = epi_kwargs(ops, c, Stub(), *views, the_noise(ops) if c.epi == "noise" else None)
    wp = ops.Packed(Stub(), KoutP, KinP, kind, None)
    return describe(ops, c, arith, xv, wp, yv, kw)[1], KinP, KoutP


def test_inputs_and_references():
    from trainner_amd import ops
    for name, f in list(globals().items()):
        if name.startswith("test_") and name != "test_inputs_and_references":
            assert any(m.name == "gpu" for m in getattr(f, "pytestmark", [])), "%s lacks @gpu" % name
    assert "pytestmark" not in globals()
    kernels = {a: set() for a in ARITH}
    widths = set()
    for c in CASES:
        for arith in ARITH:
            q, KinP, KoutP = stub_launch(ops, c, arith)
            check_class(c, arith, q, KinP, KoutP)
            kernels[arith].add(q["kernel"])
            if q["kernel"] == "tile":
                widths.add((q["tw"], q["th"]))
            if c.aim in (None, arith) and c.cls == "wrap":
                assert q["kernel"] == c.want["kernel"]
    assert kernels["f32"] == {"tile"} and kernels["bf16x3"] == {"tile", "x3w8", "d4", "s2_d4", "wino"} and kernels["bf16"] == {"tile", "d4", "s2_d4"}
    assert widths == {(8, 32), (16, 16), (32, 8), (32, 16)}
    # a sill is a place where the kernel changes: each group of sill cases holds both sides
    family = lambda c: (c.mode, c.note.rstrip("0123456789"))
    for fam in {family(c) for c in CASES if c.cls == "sill"}:
        group = [c for c in CASES if c.cls == "sill" and family(c) == fam]
        assert len(group) == 1 or len({(c.want["kernel"], c.want.get("mt")) for c in group}) == 2, fam
    assert {c.want["ksplit"] for c in CASES if c.cls == "splitk"} >= {1, 3, 4, 5, 8}
    yard, biggest = {}, 0
    for c in CASES:
        for rounded in ((False, True) if c.bf16 else (False,)):
            s64, s32, storch, count = sums(c, rounded)
            assert bool((count >= 1).all()), c.id                  # no output is an empty sum ...
            if c.cls == "px1":                                      # ... and at one pixel the stride-2 forms meet 4 of 16 / 1 of 4 taps
                assert int(count.max()) == {"3x3": 9 if c.reflect else 1, "dg3": 1, "s2": 4, "dgs2": 1, "up2": 4}[c.mode], (c.id, count)
            field = torch.ones(c.N, c.cout, c.Ho, c.Wo) if c.epi == "noise" else None      # (the device's draw is not known here)
            t, r64, r32, e_torch = refs(c, rounded, field)
            assert float((s32.double() - s64).abs().max()) <= 4e-3 * float(s64.abs().max()) + 1e-6, c.id      # (the chain is the same sum)
            assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()) and r64.shape == (c.N, c.cout, c.Ho, c.Wo), c.id
            yard[(c.id, rounded)] = float((r32.double() - r64).abs().max())
        H, W = c.in_size()
        wide = 4 * c.N * max(H * W * (c.cin + 12), c.Ho * c.Wo * (c.cout + 28))
        biggest = max(biggest, wide)
    for shape in POOL_SHAPES:
        x, w, b, r64, r32, rt = plain_case(*shape, "relu")
        yard[("pool2", shape)] = float((rt.double() - r64).abs().max())
        assert shape[3] % 2 == 0 and shape[4] % 2 == 0
    for k in C4_SHAPES:
        for cls in C4_SHAPES[k]:
            x, w, b, r64, r32, rchain = c4_case(k, cls)
            yard[("c4", k, cls)] = float((r32.double() - r64).abs().max())
    for case in THIN_CASES:
        x, w, b, r64, r32, rchain = thin_case(*case)
        yard[("thin",) + case] = float((r32.double() - r64).abs().max())
    for cls in COL_SHAPES:
        for cin in (4, 36):
            x, w, b, r64, r32, rchain = col_case(cls, cin)
            yard[("col", cls, cin)] = float((r32.double() - r64).abs().max())
    zero = [k for k, v in yard.items() if not v > 0.0]
    assert not zero, zero
    assert biggest < 64 << 20, biggest


# =====================================================================================================================
# 3. pooled and shuffled stores
# =====================================================================================================================
def lrelu_bias(s, b, dtype, act):
    v = s + b.to(dtype).view(1, -1, 1, 1)
    return {"relu": F.relu(v), "lrelu": F.leaky_relu(v, S32), "none": v}[act] * ALPHA


@cache
def plain_case(N, cin, cout, H, W, act):
    """a zero-padded 3x3 layer with bias, activation and alpha: inputs, fp64, one fp32 chain, torch's fp32"""
    c = Case("", "3x3", cin, cout, N, H, W)
    t = inputs(c)
    s64, s32, storch, _ = sums(c, False)
    b = K.rnd(cout, seed=3100 + cout)
    return t["x"], t["w"], b, lrelu_bias(s64, b, D, act), lrelu_bias(s32, b, torch.float32, act), lrelu_bias(storch, b, torch.float32, act)


POOL_SHAPES = [(1, 32, 64, 8, 8), (2, 32, 64, 10, 18), (1, 32, 256, 66, 194)]          # the minimum, a 16 x 16 tile plus one patch, the wino `wrap` shape made even


@gpu
@pytest.mark.parametrize("with_route", [False, True], ids=["noroute", "route"])
@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "N%d-%dto%d-%dx%d" % s)
def test_conv_pool2(shape, with_route, mma_mode, monkeypatch):
    """ops.conv_pool2 (the Winograd form's pooled store) against the fp64 max-pool of the fp64 convolution (max and ReLU are continuous:
    no element is left out) under the Winograd bounds, and bit for bit -- values and route bytes -- against ops.conv(wino=True) +
    maxpool2_fwd on the same inputs, which include/trainner_hip.h promises equal.  The fp32 matrix core has no such store: the entry
    says so and launches nothing."""
    from trainner_amd import ops
    trap_images(monkeypatch, ops)
    N, cin, cout, H, W = shape
    x, w, b, r64, r32, rt = plain_case(N, cin, cout, H, W, "relu")
    p64 = F.max_pool2d(r64, 2)
    xv = nan_outside(M.win(x, 4))
    snap = xv.buf.clone()
    bias = b.to(K.DEV)
    kw = dict(bias=bias, act=ops.ACT_RELU, alpha=ALPHA)

    def pooled():
        yv = M.blank(N, H // 2, W // 2, cout, 8, inner=NAN)
        route = torch.full((N, H // 2, W // 2, cout), 0xEE, dtype=torch.uint8, device=K.DEV) if with_route else None
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_FWD)
        done = ops.conv_pool2(xv, wp, yv, route=route, wino=True, **kw)
        torch.cuda.synchronize()
        return done, yv, route
    done, yv, route = pooled()
    if mma_mode == "f32":
        assert done is False and bool(torch.isnan(M.got(yv)).all())
        return
    assert done is True
    done2, yv2, route2 = pooled()
    assert same_bits(yv.buf, yv2.buf) and (route is None or torch.equal(route, route2)), "two launches differ"
    assert same_bits(xv.buf, snap)
    outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
    outside[8:8 + cout] = False
    assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT))
    full = M.blank(N, H, W, cout, 8, inner=NAN)
    wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_FWD)
    q = describe(ops, Case("", "3x3", cin, cout, N, H, W, wino=True), "bf16x3", xv, wp, full, kw)[1]
    assert q["kernel"] == "wino" and q["cap"] == 1
    if (H, W) == (66, 194):
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        assert q["tiles"] == 260 and q["tiles"] > cus and q["tiles"] % cus != 0, (q, cus)
    ops.conv(xv, wp, full, wino=True, **kw)
    two = M.blank(N, H // 2, W // 2, cout, 8, inner=NAN)
    ops.maxpool2_fwd(full, two)
    torch.cuda.synchronize()
    assert same_bits(M.got(yv), M.got(two)), "the pooled store differs from conv + maxpool2_fwd"
    got = M.got(yv)
    scale = float(p64.abs().max())
    e_dev = float((got.double() - p64.to(got.device)).abs().max())
    print("YARDSTICK-TORCH pool2 %s dev %.3e torch-fp32 %.3e (not asserted)" % (shape, e_dev, float((F.max_pool2d(rt, 2).double() - p64).abs().max())))
    assert e_dev <= 2e-5 * (scale + 1.0)
    monkeypatch.setattr(ops, "MMA", F32)
    f32 = M.blank(N, H, W, cout, 8, inner=NAN)
    ops.conv(xv, wp, f32, wino=False, **kw)
    torch.cuda.synchronize()
    held_x3("pool2 %s" % (shape,), got, F.max_pool2d(M.got(f32), 2), p64, 3.0)
    if with_route:      # bits 0-1: the first maximum in the scan order (0,0), (0,1), (1,0), (1,1); bit 2: pooled value > 0
        m = M.got(full)
        win = torch.stack([m[:, :, 0::2, 0::2], m[:, :, 0::2, 1::2], m[:, :, 1::2, 0::2], m[:, :, 1::2, 1::2]])
        best, arg = win[0].clone(), torch.zeros_like(win[0], dtype=torch.uint8)
        for i in (1, 2, 3):
            better = win[i] > best
            best, arg = torch.where(better, win[i], best), torch.where(better, torch.full_like(arg, i), arg)
        want = arg + 4 * (best > 0).to(torch.uint8)
        assert torch.equal(route.permute(0, 3, 1, 2), want), "route bytes"


SHUFFLE_SHAPES = [(1, 8, 32, 64), (1, 9, 33, 64), (2, 257, 33, 64)]          # the minimum of the d4 kernel, ragged, the d4 `wrap` shape (Cout = 4 nf = 256)


@gpu
@pytest.mark.parametrize("shape", SHUFFLE_SHAPES, ids=lambda s: "N%d-%dx%d-nf%d" % s)
def test_conv_shuffle2(shape, mma_mode, monkeypatch):
    """ops.conv_shuffle2 (conv nf -> 4 nf + nn.PixelShuffle(2) + LeakyReLU in the d4 kernel's store) against the fp64 statement; y is a
    view at a non-zero offset of a wider buffer.  bf16x3 and bf16; the fp32 matrix core has no such kernel and the entry says so."""
    from trainner_amd import ops
    trap_images(monkeypatch, ops)
    N, H, W, nf = shape
    for arith in [mma_mode] + (["bf16"] if mma_mode == "bf16x3" else []):
        monkeypatch.setattr(ops, "MMA", ARITH[arith])
        c = Case("", "3x3", nf, 4 * nf, N, H, W)
        t = inputs(c)
        s64, s32, storch, _ = sums(c, arith == "bf16")
        b = K.rnd(4 * nf, seed=3200)
        r64, r32 = (F.pixel_shuffle(lrelu_bias(s_, b, dt, "lrelu"), 2) for s_, dt in ((s64, D), (s32, torch.float32)))
        xv = nan_outside(M.win(t["x"], 4))
        snap = xv.buf.clone()
        kw = dict(bias=b.to(K.DEV), act=ops.ACT_LRELU, slope=0.2, alpha=ALPHA)
        runs = []
        for rep_ in range(2):
            yv = M.blank(N, 2 * H, 2 * W, nf, 8, inner=NAN)
            wp, _keep = K.pack(ops, t["w"].to(K.DEV), ops.PACK_FWD)
            done = ops.conv_shuffle2(xv, wp, yv, **kw)
            torch.cuda.synchronize()
            if arith == "f32":
                assert done is False and bool(torch.isnan(M.got(yv)).all())
                return
            assert done is True
            form, d = ops.conv_launch_desc(xv, wp, yv, ops.CONV_3x3, None, 2, kw, dry=True)
            q = ops.conv_launch_class(d)
            assert q["kernel"] == "d4" and q["cap"] == 2 and q["ncb"] == 4 * nf // 64
            if H == 257:
                cus = torch.cuda.get_device_properties(0).multi_processor_count
                assert q["tiles"] == 528 and q["tiles"] > 2 * cus and q["tiles"] % (2 * cus) != 0, (q, cus)
            outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
            outside[8:8 + nf] = False
            assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT))
            runs.append(M.got(yv))
        assert same_bits(runs[0], runs[1]) and same_bits(xv.buf, snap)
        M.yardstick("shuffle2 %s %s" % (shape, arith), runs[0], r64, r32)
        if arith == "bf16x3":
            monkeypatch.setattr(ops, "MMA", F32)
            mid, two = M.blank(N, H, W, 4 * nf, 8, inner=NAN), M.blank(N, 2 * H, 2 * W, nf, 8, inner=NAN)
            ops.conv(xv, wp, mid, wino=False, **kw)
            ops.depth_to_space(mid, two)
            torch.cuda.synchronize()
            held_x3("shuffle2 %s" % (shape,), runs[0], M.got(two), r64, 1.5)


# =====================================================================================================================
# 4. the image layers (3 -> 64 over NHWC4: taps folded into K), the thin forms and the patch-matrix forms
# =====================================================================================================================
def beside_chain(what, got, r64, r32, rchain):
    """the yardstick against torch's own fp32 statement, which these forms are held to; beside it the ratio to one fp32 chain"""
    e_chain = float((rchain.double() - r64).abs().max())
    e_dev = float((got.double() - r64.to(got.device)).abs().max())
    print("YARDSTICK-CHAIN %-50s dev %.3e  chain-fp32 %.3e  dev/(2 chain + 2e-7 scale) %.3f (not asserted)"
          % (what, e_dev, e_chain, e_dev / (2 * e_chain + 2e-7 * float(r64.abs().max()))))
    M.yardstick(what, got, r64, r32)


C4_SHAPES = {3: {"px1": (1, 1, 1), "lineH": (1, 1, 9), "lineW": (1, 33, 1), "images": (3, 17, 65)},
             7: {"px1": (1, 4, 4), "lineH": (1, 4, 9), "lineW": (1, 33, 4), "images": (3, 17, 65)}}      # 7x7 with ReflectionPad2d(3) needs 4 x 4


@cache
def c4_case(k, cls):
    N, H, W = C4_SHAPES[k][cls]
    x, w, b = K.rnd(N, 3, H, W, seed=3300 + k), K.rnd(64, 3, k, k, seed=3301 + k, lo=-0.2, hi=0.2), K.rnd(64, seed=3302)
    p = k // 2
    pad = (lambda t: F.pad(t, (p, p, p, p), mode="reflect")) if k == 7 else (lambda t: F.pad(t, (p, p, p, p)))
    r64 = lrelu_bias(F.conv2d(pad(x.double()), w.double()), b, D, "lrelu")
    r32 = lrelu_bias(F.conv2d(pad(x), w), b, torch.float32, "lrelu")
    return x, w, b, r64, r32, lrelu_bias(chain_taps(pad(x), w, H, W), b, torch.float32, "lrelu")


@gpu
@pytest.mark.parametrize("cls", ["px1", "lineH", "lineW", "images"])
@pytest.mark.parametrize("k", [3, 7])
def test_image_layer_c4(k, cls, mma_mode, monkeypatch):
    """TNR_CONV_3x3_C4 and TNR_CONV_7x7_C4 (ReflectionPad2d(3) in the kernel): 3 -> 64 over an NHWC4 image, y a view of a wider buffer"""
    from trainner_amd import ops
    x, w, b, r64, r32, rchain = c4_case(k, cls)
    N, H, W = C4_SHAPES[k][cls]
    x4 = K.nhwc_buf(F.pad(x, (0, 0, 0, 0, 0, 1)), fill=0.0)
    snap = x4.clone()
    runs = []
    for rep_ in range(2):
        yv = M.blank(N, H, W, 64, 8, inner=NAN)
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_C4_FWD)
        kw = dict(bias=b.to(K.DEV), act=ops.ACT_LRELU, slope=0.2, alpha=ALPHA, reflect=(k == 7))
        mode = ops.CONV_3x3_C4 if k == 3 else ops.CONV_7x7_C4
        form, d = ops.conv_launch_desc(ops.View(x4), wp, yv, mode, None, 0, kw, dry=True)
        q = ops.conv_launch_class(d)
        assert (q["kernel"], q["nt"], q["ksplit"]) == ("tile", 2, 1) and q["tw"] == pick_tw(W, H), q
        ops.conv(ops.View(x4), wp, yv, mode=mode, **kw)
        torch.cuda.synchronize()
        outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
        outside[8:72] = False
        assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT))
        runs.append(M.got(yv))
    assert same_bits(runs[0], runs[1]) and same_bits(x4, snap)
    beside_chain("c4 %dx%d %s %s" % (k, k, cls, mma_mode), runs[0], r64, r32, rchain)


THIN_SHAPES = {"px1": (1, 1, 1), "lineH": (1, 1, 37), "lineW": (1, 9, 1), "tile+1": (2, 17, 17)}
THIN7_SHAPES = {"min": (1, 4, 4), "lineH": (1, 4, 21), "lineW": (1, 9, 4), "tile+1": (2, 17, 17), "seg159": (1, 5, 159), "seg160": (1, 5, 160), "seg161": (1, 5, 161)}
THIN_CASES = [(k, cls, dg, cb, cs) for k, shapes in ((3, THIN_SHAPES), (7, THIN7_SHAPES)) for cls in shapes for dg in (False, True)
              for cb in (16, 32, 64) for cs in (1, 3) if not cls.startswith("seg") or (cb, cs) in ((16, 1), (64, 3))]
PAD_SENT = 7.5


@cache
def thin_case(k, cls, dg, cb, cs):
    """forward: Cbig -> Csmall with bias and alpha (k = 7: ReflectionPad2d(3)).  dgrad: the gradient of a Csmall -> Cbig layer with respect
    to its input (k = 7: its reflection-padded input, (H + 6) x (W + 6), zero borders)"""
    N, H, W = (THIN_SHAPES if k == 3 else THIN7_SHAPES)[cls]
    x = K.rnd(N, cb, H, W, seed=3400 + k + cb)
    p = k // 2
    if not dg:
        w, b = K.rnd(cs, cb, k, k, seed=3401 + k, lo=-0.1, hi=0.1), K.rnd(cs, seed=3402)
        pad = (lambda t: F.pad(t, (p, p, p, p), mode="reflect")) if k == 7 else (lambda t: F.pad(t, (p, p, p, p)))
        r64 = ALPHA * (F.conv2d(pad(x.double()), w.double()) + b.double().view(1, -1, 1, 1))
        r32 = ALPHA * (F.conv2d(pad(x), w) + b.view(1, -1, 1, 1))
        return x, w, b, r64, r32, ALPHA * (chain_taps(pad(x), w, H, W) + b.view(1, -1, 1, 1))
    w = K.rnd(cb, cs, k, k, seed=3403 + k, lo=-0.1, hi=0.1)
    q = p if k == 3 else 0                                          # conv_transpose2d's padding: the 7x7 gradient lives on the padded grid
    r64 = F.conv_transpose2d(x.double(), w.double(), padding=q)
    weq = w.flip(2, 3).transpose(0, 1).contiguous()
    e = k - 1 - q
    return x, w, None, r64, F.conv_transpose2d(x, w, padding=q), chain_taps(F.pad(x, (e, e, e, e)), weq, r64.shape[2], r64.shape[3])


@gpu
@pytest.mark.parametrize("case", THIN_CASES, ids=lambda c: "thin%d-%s-%s-C%d-c%d" % (c[0], c[1], "dgrad" if c[2] else "fwd", c[3], c[4]))
def test_thin(case, mma_mode):
    """ops.conv_thin / ops.conv_thin7, forward and dgrad=True: x a view at offset 8 with NaN outside; the 4-channel side is the
    destination, whose pad channels hold a finite sentinel and keep it, and the stored bits equal those of a launch over zeros there"""
    from trainner_amd import ops
    k, cls, dg, cb, cs = case
    x, w, b, r64, r32, rchain = thin_case(*case)
    N, Ho, Wo = r64.shape[0], r64.shape[2], r64.shape[3]
    xv = nan_outside(M.win(x, 8))
    snap = xv.buf.clone()
    wd, bd = w.to(K.DEV), None if b is None else b.to(K.DEV)
    runs = []
    for fill in (PAD_SENT, PAD_SENT, 0.0):
        y = torch.full((N, Ho, Wo, 4), fill, device=K.DEV)
        y[..., :cs] = NAN
        if k == 3:
            ops.conv_thin(xv, wd, ops.View(y, 0, cs), bias=bd, alpha=1.0 if dg else ALPHA, dgrad=dg)
        else:
            ops.conv_thin7(xv, wd, ops.View(y, 0, cs), pad=6 if dg else 3, reflect=not dg, bias=bd, alpha=1.0 if dg else ALPHA, dgrad=dg)
        torch.cuda.synchronize()
        assert bool((y[..., cs:] == fill).all()), "the pad channels of the destination changed"
        runs.append(y[..., :cs].permute(0, 3, 1, 2))
    assert same_bits(runs[0], runs[1]), "two launches differ"
    assert same_bits(runs[0], runs[2]), "the result depends on the destination's pad channels"
    assert same_bits(xv.buf, snap)
    if k == 7 and not dg and cls.startswith("seg"):
        assert cdiv(Wo, 160) == (2 if Wo > 160 else 1) and Ho % 2 == 1          # T7C_SEG columns per wave, cdiv(Ho, 2) row pairs
    beside_chain("thin%d %s %s C%d c%d" % (k, cls, "dgrad" if dg else "fwd", cb, cs), runs[0], r64, r32, rchain)


@gpu
@pytest.mark.parametrize("hw", [(3, 4), (4, 3)], ids=["H3", "W3"])
def test_thin7_refuses_a_reflection_wider_than_the_image(hw, mma_mode):
    from trainner_amd import hip, ops
    H, W = hw
    xv = nan_outside(M.win(K.rnd(1, 16, H, W, seed=3410), 8))
    y = torch.full((1, H, W, 4), PAD_SENT, device=K.DEV)
    with pytest.raises(hip.HipEngineError, match="conv_thin7"):
        ops.conv_thin7(xv, K.rnd(3, 16, 7, 7, seed=3411).to(K.DEV), ops.View(y, 0, 3), pad=3, reflect=True)
    torch.cuda.synchronize()
    assert bool((y == PAD_SENT).all())


COL_SHAPES = {"pix8": (1, 3, 5), "pix16": (1, 5, 5), "pix24": (1, 4, 9), "pix4096": (1, 65, 65), "pix4104": (1, 73, 58)}      # N, H, W of the input: (H - 1) x (W - 1) outputs


@cache
def col_case(cls, cin):
    N, H, W = COL_SHAPES[cls]
    x, w, b = K.rnd(N, cin, H, W, seed=3500 + cin), K.rnd(64, cin, 4, 4, seed=3501, lo=-0.1, hi=0.1), K.rnd(64, seed=3502)
    r64 = lrelu_bias(F.conv2d(x.double(), w.double(), padding=1), b, D, "lrelu")
    r32 = lrelu_bias(F.conv2d(x, w, padding=1), b, torch.float32, "lrelu")
    return x, w, b, r64, r32, lrelu_bias(chain_taps(F.pad(x, (1, 1, 1, 1)), w, H - 1, W - 1), b, torch.float32, "lrelu")


@gpu
@pytest.mark.parametrize("entry", ["conv_small", "conv_col"])
@pytest.mark.parametrize("cin", [4, 36])
@pytest.mark.parametrize("cls", list(COL_SHAPES))
def test_patch_matrix_4x4_s1(cls, cin, entry, mma_mode):
    """the PatchGAN's 4x4 stride-1 pad-1 layers through tnr_im2col + the 1x1 kernel: 8, 16 and 24 output pixels (conv_small's image
    widths 8 and 16), 4096 (32) and 4104 (8); Cin = 4 and 36 (K = 64 and 576: the second runs split-K where the tiles are few)"""
    from trainner_amd import hip, ops
    x, w, b, r64, r32, rchain = col_case(cls, cin)
    N, H, W = COL_SHAPES[cls]
    assert (N * (H - 1) * (W - 1)) == int(cls[3:])
    xv = nan_outside(M.win(x, 4))
    snap = xv.buf.clone()
    runs = []
    for rep_ in range(2):
        yv = M.blank(N, H - 1, W - 1, 64, 8, inner=NAN)
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_COL_FWD)
        names = ["im2col@%x" % hip.stream(), "splitk@%x" % hip.stream()]
        with ws_trap(ops, {n: 4 * 16 * cin * 4104 + (1 << 16) for n in names}, xv.buf.device, must=names[:1]):
            getattr(ops, entry)(xv, wp, yv, 4, 1, 1, bias=b.to(K.DEV), act=ops.ACT_LRELU, slope=0.2, alpha=ALPHA)
            torch.cuda.synchronize()
        outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
        outside[8:72] = False
        assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT))
        runs.append(M.got(yv))
    assert same_bits(runs[0], runs[1]) and same_bits(xv.buf, snap)
    beside_chain("%s %s Cin%d %s" % (entry, cls, cin, mma_mode), runs[0], r64, r32, rchain)
