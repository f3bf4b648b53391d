"""Edge-shape parity of the tile-staged image-space kernels -- csrc/image_losses.hip (filter_kernel<0/1>, fd_fwd / fd_bwd, point_*,
overflow_*), csrc/freqsep.hip (low pass, high pass forward and backward), csrc/spl_loss.hip (statistics, finalize, gradient) and
csrc/ssim_loss.hip (ssim_fwd / ssim_bwd, pool_fwd / pool_bwd, combine) -- through the ops wrappers, against the fp64 restatements of
tools/make_golden_image_losses.py (hfen_response, fd_responses, rho, adjoint), make_golden_freqsep.py (low), make_golden_spl.py
(spl_trace, differences, rgb_to_yuv, denorm) and make_golden_ssim.py (maps, level_table, restate; `maps` takes any window).  The
golden-shape modules run these kernels at 72 x 72, 99 x 117, 136 x 136 (and 192 x 192); here they run at the shapes at which tiled
stencils go wrong, and the class is part of the test id.  A K-tap HFEN filter with K < 15 is stated here from F.conv2d /
F.conv_transpose2d (hfen_stmt / hfen_adj) and pinned to the tool's statement at K = 15 in test_inputs_and_references.

Constants read from the kernels (they agree with what the classes were written for): tile TW x TH = 64 x 16 for every stencil kernel,
halos 7 (HFEN), 4 (freqsep), 1 (fd backward, spl gradient), 0 (fd forward, spl statistics); SSIM forward tile FT = 32 x 32 map
positions, backward tile BH x BW = 16 x 32 pixels of the FULL image; SPL band RT x TH = 4 x 16 = 64 rows; second-stage sums stride over
256 threads.

  px1      1 x 1 (SSIM: K x K after the shave, shave 0 and 4, one map position; avgpool2_pad: 2 x 2); one below is refused
  thin     1 x 65, 17 x 1, 3 x 5, and 2 x 4, 5 x 8 (W % 4 == 0: the 16-byte path on an image narrower than the halo); SSIM K x 50, 45 x K
  sill     W in {63, 64, 65, 128} x H in {15, 16, 17, 32} (each value twice); SPL H = 63, 64, 65; SSIM maps of 31 / 32 / 33 both ways
           (K = 11, shave 4 and 0) and full images of 15 x 31, 16 x 32, 17 x 33 for the backward tile (K = 11 shave 0, K = 3 shave 4)
  vecsill  NCHW, W = 4, 8, 60, 64, 68, 72: every operand in turn 1, 2 or 3 floats off a 16-byte boundary (vec_rows declines), all
           operands 4 floats off (still the 16-byte path): the same bits as the aligned launch, which meets the bounds
  planes   N = 3 with C = 1, 2, 3, 4, every plane different; N x C x tiles = 288 (stencils) / 300 (SSIM) > 256; C = 5 refused (spl, ssim)
  taps     HFEN K = 1, 3, 7, 15 with a seeded asymmetric table; freqsep with asymmetric 9 taps; SSIM K = 1, 3, 5, 7, 11 asymmetric;
           MS-SSIM over level_table(23, 27) (windows 11, 11, 5, 3, 1; odd sizes on both axes at the pooled levels)
  epi      every backward with accumulate / gscale (filter_loss_bwd, fd_loss_bwd, freqsep_low, freqsep_high_bwd, spl_loss_bwd,
           ssim_bwd, pointwise_loss_bwd, overflow_loss_bwd): a null gscale, a gscale tensor != 1 (SPL: four different ones, one per
           family, all families on), accumulate onto a pre-filled gx (== fill + fresh, one fp32 addition).  Shapes: N3 C3 17 x 65
           (scalar epilogues, both layouts), 17 x 64 (the last group exactly full) and 17 x 72 (a group across the second tile column)
           for the 16-byte epilogues, whose accumulated bits must equal the scalar epilogue's; the flat kernels at every n of the
           flat sweep, 16-byte body and scalar tail.  Every launch uses a scale that is no power of two

The flat kernels (point_*, overflow_*) sweep n = 1 (px1), 3 / 4 / 5 (thin), 255 / 1023 / 1024 / 1025 (sill), 70001 (planes: 274
partials, the second-stage sum strides), aligned and one float off.

Traps in every case.  Every device operand (images, losses, SSIM sums, coefficient buffers, gscale, the pooled MS-SSIM levels; the
workspaces are the wrappers' own) is a slice of a larger flat buffer (PAD floats on either side, enough for the 7-row halo of
the widest single-plane case): NaN around the sources, a sentinel around the destinations that must survive bit for bit; destinations
start as NaN unless the launch accumulates; the sources hold the same bits afterwards; every launch runs twice and returns the same bits.

Bounds, measured on the restatement, never on the device.  Values: |v - v64| <= 4 x |v32 - v64| + 4 fp32 ulps of v64.  Gradients and
maps: max err <= 4 x max|r32 - r64| (over the compared elements) + 2e-7 x max|r64|, r32 the same restatement evaluated in fp32 on the CPU (the factor 4 is that of
test_gpu_image_losses.py / test_gpu_ssim_loss.py).  Every ratio is printed on a RATIO line before it is asserted; DESIGN.md sections 11-13 and 18
has the worst per class.  Pure movement and single correctly rounded operations (accumulate, pool backward, the SSIM-mode coefficient)
compare with torch.equal; identical images give exactly 0.

Kinks.  Every class runs kink-free criteria with no exclusion at all: l2 (HFEN value and map), tv-l2 / dtv-l2 / grad-l2, the HFEN adjoint
on a given random map, freqsep on inputs whose pre-clamp value stays inside [0.01, 0.99] and, for the backward, on a GIVEN saved output
with planted exact 0 / 1 entries (the mask is then the same predicate on both sides).  Kinked criteria run under
make_golden_image_losses.near_zero_mask (fd l1 / cb: the 3 x 3 reach of a response with 0 < |e64| <= 4 e32_resp; HFEN l1 map: the
responses within that band): the left-out share is 0 for cases under 1000 elements and <= 1e-3 otherwise, from seeds chosen on the
fp64 restatement alone (first_seed).  SSIM cases have no clamped variance in fp32 or fp64 and every per-level cs / ssim above 0.5,
except one planted clamp at a sill shape whose value alone is checked.

test_inputs_and_references (no device) builds every case, asserts the class conditions, the shares, that the fp32 restatement's own error (the
yardstick without its additive term, over the compared elements) is non-zero except in the cases listed in CARRIED, the refusals (the TNR_REQUIRE returns of these entry points all precede their first HIP call, so they
are reached through the loaded library with host pointers) and the size of the largest case.  No module-level `pytestmark`.
"""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import detrand
from tools import make_golden_freqsep as TF
from tools import make_golden_image_losses as T
from tools import make_golden_spl as TS
from tools import make_golden_ssim as TG

gpu = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = -123.0
D = torch.double
PAD = 2048                                                  # floats around every slice (multiple of 4; > 7 rows of 128 + 7)
SCALE = float(torch.tensor(0.37, dtype=torch.float32))      # no power of two; the same number as a double and as a float
GS = float(torch.tensor(0.6, dtype=torch.float32))
C1 = float(torch.tensor(0.01 ** 2, dtype=torch.float32))    # the constants as the C ABI receives them (fp32)
C2 = float(torch.tensor(0.03 ** 2, dtype=torch.float32))
CRIT = {"l1": 0, "l2": 1, "cb": 2, "elastic": 3, "clipl1": 4}
LAYOUTS = [0, 1]
LAYOUT_IDS = ["nchw", "cl"]
cache = functools.lru_cache(maxsize=None)


def _ops():
    from trainner_amd import ops
    return ops


def U(shape, seed, lo=0.0, hi=1.0):
    return detrand.uniform(shape, seed, lo, hi)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def ulp32(v):
    return float(torch.finfo(torch.float32).eps) * 2.0 ** math.floor(math.log2(max(abs(v), 1e-30)))


def value_bound(v64, v32):
    return 4.0 * abs(v32 - v64) + 4.0 * ulp32(v64)


def e32_term(r64, r32, keep=None):
    """4 x the fp32 restatement's own error, over the compared elements only"""
    d = (r32.double() - r64).abs()
    d = d if keep is None else d[keep]
    return 4.0 * float(d.max()) if d.numel() else 0.0


def map_bound(r64, r32, keep=None):
    return e32_term(r64, r32, keep) + 2e-7 * float(r64.abs().max())


def report(cid, what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    print("\nRATIO %-34s %-22s err %.3e bound %.3e ratio %.3f" % (cid, what, err, bound, ratio), end="")
    return ratio


def check_value(cid, what, got, v64, v32):
    b = value_bound(v64, v32)
    assert report(cid, what, abs(got - v64), b) <= 1.0, (cid, what, got, v64, v32)


def check_map(cid, what, got, r64, r32, keep=None):
    assert got.shape == r64.shape and bool(torch.isfinite(got).all()), (cid, what)
    err = (got.double() - r64).abs()
    if keep is not None:
        err = err[keep]
    e = float(err.max()) if err.numel() else 0.0
    assert report(cid, what, e, map_bound(r64, r32, keep)) <= 1.0, (cid, what, e)


# =====================================================================================================================
# operands: slices of larger flat buffers
# =====================================================================================================================
class Op:
    """An N x C x H x W operand in `layout` at float offset PAD + off of a flat device buffer; `outer` around it."""
    def __init__(self, shape, layout, off=0, data=None, inner=NAN, outer=NAN):
        N, C, H, W = shape
        self.shape, self.layout, self.n, self.lo = shape, layout, N * C * H * W, PAD + off
        host = torch.full((self.lo + self.n + PAD,), outer, dtype=torch.float32)
        if data is not None:
            d = data.float()
            assert tuple(d.shape) == tuple(shape)
            host[self.lo:self.lo + self.n] = (d.permute(0, 2, 3, 1) if layout else d).contiguous().flatten()
        else:
            host[self.lo:self.lo + self.n] = inner
        self.host = host
        self.buf = host.to(DEV)
        assert self.buf.data_ptr() % 16 == 0
        flat = self.buf[self.lo:self.lo + self.n]
        self.t = flat.view(N, H, W, C).permute(0, 3, 1, 2) if layout else flat.view(N, C, H, W)
        assert self.t.data_ptr() % 16 == (4 * off) % 16

    def reset(self):
        self.buf.copy_(self.host)

    def result(self):
        N, C, H, W = self.shape
        f = self.buf[self.lo:self.lo + self.n].cpu()
        return (f.view(N, H, W, C).permute(0, 3, 1, 2) if self.layout else f.view(N, C, H, W)).contiguous()

    def outside_ok(self):
        b = self.buf.cpu()
        return same_bits(b[:self.lo], self.host[:self.lo]) and same_bits(b[self.lo + self.n:], self.host[self.lo + self.n:])

    def unchanged(self):
        return same_bits(self.buf.cpu(), self.host)


class Small:
    """k scalars (a loss, the SSIM sums) between two sentinels"""
    def __init__(self, k=1, dtype=torch.float32, inner=NAN, data=None):
        self.k = k = k if data is None else len(data)
        self.host = torch.full((k + 2,), SENT, dtype=dtype)
        self.host[1:1 + k] = inner if data is None else torch.as_tensor(data, dtype=dtype)
        self.buf = self.host.to(DEV)
        self.t = self.buf[1:1 + k]

    def reset(self):
        self.buf.copy_(self.host)

    def result(self):
        return self.buf[1:1 + self.k].cpu()

    def outside_ok(self):
        b = self.buf.cpu()
        return float(b[0]) == SENT and float(b[-1]) == SENT


def run_twice(call, srcs, outs):
    """the launch twice from the same start: the same bits, the sentinels intact, the sources untouched; leaves the second result"""
    before = [s.buf.clone() for s in srcs]
    call()
    first = [o.buf.clone() for o in outs]
    for o in outs:
        o.reset()
    call()
    for o, f in zip(outs, first):
        assert torch.equal(o.buf.view(torch.uint8), f.view(torch.uint8)), "two runs differ"
        assert o.outside_ok(), "wrote outside the slice"
    for s, b in zip(srcs, before):
        assert torch.equal(s.buf.view(torch.uint8), b.view(torch.uint8)), "a source changed"


def gst(gs):
    """a gscale operand (a Small, or None for the null pointer) as the wrappers take it"""
    return None if gs is None else gs.t


def gsrc(gs):
    return [] if gs is None else [gs]


def autograd(fn, x, dtype):
    x = x.detach().to(dtype).contiguous().requires_grad_(True)
    v = fn(x)
    v.backward()
    return v.detach(), x.grad.detach()


def first_seed(base, ok):
    """the first of 32 seeds from `base` whose fp64 restatement meets `ok` (the kinked cases' left-out share)"""
    for s in range(base, base + 32):
        if ok(s):
            return s
    raise AssertionError("no seed from %d meets the share" % base)


def share_cap(numel):
    return 0.0 if numel < 1000 else 1e-3


# =====================================================================================================================
# the case tables
# =====================================================================================================================
SILL_HW = [(15, 63), (16, 64), (17, 65), (32, 128), (17, 63), (32, 64), (15, 65), (16, 128)]
THIN_HW = [(1, 65), (17, 1), (3, 5), (2, 4), (5, 8)]
VEC_W = [4, 8, 60, 64, 68, 72]


def _img_cases():
    c = {"px1-1x1": (1, 1, 1, 1)}
    for h, w in THIN_HW:
        c["thin-%dx%d" % (h, w)] = (1, 1, h, w)
    for h, w in SILL_HW:
        c["sill-%dx%d" % (h, w)] = (1, 1, h, w)
    for ch in (1, 2, 3, 4):
        c["planes-N3C%d-17x65" % ch] = (3, ch, 17, 65)
    c["planes-N3C4-49x321"] = (3, 4, 49, 321)               # 3 x 4 x (4 x 6) = 288 tiles: the second-stage sum strides
    return c


IMG = _img_cases()
SPL = dict(IMG)
SPL.update({"sill-%dx9" % h: (1, 2, h, 9) for h in (63, 64, 65)})
SPL["sill-129x68"] = (1, 3, 129, 68)                         # three bands, two tile columns, W % 4 == 0
VEC = {"vecsill-17x%d" % w: (1, 1, 17, w) for w in VEC_W}     # NCHW only (test_vecsill)
# epi: the scalar epilogues (W = 65, and channels-last) and the 16-byte ones at an exactly full last group (64) and across a tile column (72)
EPI = {"epi-N3C3-17x65": (3, 3, 17, 65), "epi-N1C3-17x64": (1, 3, 17, 64), "epi-N1C3-17x72": (1, 3, 17, 72)}
SHAPES = {**IMG, **VEC, **EPI}                              # what the reference builders look a name up in
SPL_SHAPES = {**SPL, **VEC, **EPI}
HFEN_TAPS = {"taps-K%d" % k: k for k in (1, 3, 7, 15)}
# name -> (N, C, H, W, shave, K, asymmetric taps)
SSIM = {"px1-K11-11x11-shave0": (1, 1, 11, 11, 0, 11, False), "px1-K11-19x19-shave4": (1, 1, 19, 19, 4, 11, False),
        "px1-K3-3x3-shave0": (1, 1, 3, 3, 0, 3, False),
        "thin-11x50": (1, 1, 11, 50, 0, 11, False), "thin-45x11": (1, 1, 45, 11, 0, 11, False),
        "sill-map31x33-shave4": (1, 1, 49, 51, 4, 11, False), "sill-map32x32-shave4": (1, 1, 50, 50, 4, 11, False),
        "sill-map33x31-shave4": (1, 1, 51, 49, 4, 11, False), "sill-map32x32-shave0": (1, 1, 42, 42, 0, 11, False),
        "sill-bwd15x31-K11": (1, 1, 15, 31, 0, 11, False), "sill-bwd16x32-K11": (1, 1, 16, 32, 0, 11, False),
        "sill-bwd17x33-K11": (1, 1, 17, 33, 0, 11, False), "sill-bwd15x31-K3-shave4": (1, 1, 15, 31, 4, 3, False),
        "sill-bwd16x32-K3-shave4": (1, 1, 16, 32, 4, 3, False), "sill-bwd17x33-K3-shave4": (1, 1, 17, 33, 4, 3, False),
        "planes-N3C1-20x37": (3, 1, 20, 37, 2, 11, False), "planes-N3C2-20x37": (3, 2, 20, 37, 2, 11, False),
        "planes-N3C3-20x37": (3, 3, 20, 37, 2, 11, False), "planes-N3C4-20x37": (3, 4, 20, 37, 2, 11, False),
        "planes-N3C4-139x139": (3, 4, 139, 139, 0, 11, False)}                      # 3 x 4 x 25 = 300 forward blocks
SSIM.update({"taps-K%d" % k: (1, 2, 21, 40, 1, k, True) for k in (1, 3, 5, 7, 11)})
CLAMP_CASE = "sill-map32x32-shave4"
POOL = {"px1-2x2": (1, 1, 2, 2, 0), "thin-3x5": (1, 1, 3, 5, 0), "thin-2x9": (1, 1, 2, 9, 0), "sill-shave2-9x12": (2, 3, 9, 12, 2),
        "planes-N3C4-23x27": (3, 4, 23, 27, 0)}
FLAT_N = [1, 3, 4, 5, 255, 1023, 1024, 1025, 70001]         # 70001 scalar: 274 blocks > 256 partials
FLAT_IDS = ["px1-n1", "thin-n3", "thin-n4", "thin-n5", "sill-n255", "sill-n1023", "sill-n1024", "sill-n1025", "planes-n70001"]


def case_seed(name):
    return 1000 + sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100000


# =====================================================================================================================
# 1. HFEN (filter_kernel<0/1>)
# =====================================================================================================================
def hfen_stmt(d, taps):
    """e = L * d: the zero-padded K x K correlation of every plane, in d's dtype"""
    K = taps.shape[0]
    return F.conv2d(d, taps.to(d.dtype).expand(d.shape[1], 1, K, K), padding=K // 2, groups=d.shape[1])


def hfen_adj(m, taps):
    K = taps.shape[0]
    return F.conv_transpose2d(m, taps.to(m.dtype).expand(m.shape[1], 1, K, K), padding=K // 2, groups=m.shape[1])


@cache
def asym_taps(K):
    return U((K, K), 900 + K, -1.0, 1.0)


class Ref:
    pass


@cache
def filter_ref(name):
    r = Ref()
    if name in HFEN_TAPS:
        r.shape, r.taps = (1, 2, 19, 70), asym_taps(HFEN_TAPS[name])
    else:
        r.shape, r.taps = SHAPES[name], T.log_taps()
    r.K = r.taps.shape[0]
    numel = r.shape[0] * r.shape[1] * r.shape[2] * r.shape[3]

    def build(seed):
        x, y = U(r.shape, seed), U(r.shape, seed + 50000)
        e64, e32 = hfen_stmt(x.double() - y.double(), r.taps), hfen_stmt(x - y, r.taps)
        band = 4 * float((e32.double() - e64).abs().max())
        far = (e64.abs() > band) | (e64 == 0)
        return x, y, e64, e32, far

    r.seed = first_seed(case_seed(name), lambda s: 1.0 - float(build(s)[4].double().mean()) <= share_cap(numel))
    r.x, r.y, r.e64, r.e32, r.far = build(r.seed)
    r.near_share = 1.0 - float(r.far.double().mean())
    r.v = {c: (float(SCALE * T.rho(r.e64, c).sum()), float((SCALE * T.rho(r.e32, c).sum()))) for c in ("l2", "l1")}
    r.map = {c: (T.drho(r.e64, c), T.drho(r.e32, c)) for c in ("l2", "l1")}
    r.m = U(r.shape, r.seed + 7, -1.0, 1.0)
    r.adj = (SCALE * hfen_adj(r.m.double(), r.taps), torch.tensor(SCALE, dtype=torch.float32) * hfen_adj(r.m, r.taps))
    return r


def run_filter(r, layout, offs=(0, 0, 0, 0, 0), gs=None, fill=None):
    ops = _ops()
    tp = [float(v) for v in r.taps.flatten()]
    x, y = Op(r.shape, layout, offs[0], r.x), Op(r.shape, layout, offs[1], r.y)
    dmap, loss = Op(r.shape, layout, offs[2], outer=SENT), Small()
    out = {}
    for c in ("l2", "l1"):
        dmap.reset()
        loss.reset()
        run_twice(lambda: ops.filter_loss_fwd(x.t, y.t, layout, tp, r.K, CRIT[c], SCALE, loss.t, dmap.t), [x, y], [loss, dmap])
        out["v_" + c], out["map_" + c] = float(loss.result()[0]), dmap.result()
    m = Op(r.shape, layout, offs[3], r.m)
    gx = Op(r.shape, layout, offs[4], data=fill, outer=SENT)
    run_twice(lambda: ops.filter_loss_bwd(m.t, layout, tp, r.K, SCALE, gst(gs), gx.t, accumulate=fill is not None), [m] + gsrc(gs), [gx])
    out["gx"] = gx.result()
    return out


def check_filter(cid, r, out):
    for c in ("l2", "l1"):
        check_value(cid, "hfen-%s value" % c, out["v_" + c], *r.v[c])
    check_map(cid, "hfen-l2 map", out["map_l2"], *r.map["l2"])
    check_map(cid, "hfen-l1 map", out["map_l1"], *r.map["l1"], keep=r.far)
    assert float(out["map_l1"].abs().max()) <= 1.0
    check_map(cid, "hfen adjoint", out["gx"], *r.adj)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(IMG) + list(HFEN_TAPS))
def test_hfen(name, layout):
    r = filter_ref(name)
    check_filter("%s-%s" % (name, LAYOUT_IDS[layout]), r, run_filter(r, layout))


# =====================================================================================================================
# 2. finite differences (fd_fwd_kernel / fd_bwd_kernel)
# =====================================================================================================================
FD_NAMES = {"grad-2d-l2": (2, "l2", True), "grad-4d-l2": (4, "l2", True), "tv-l2": (2, "l2", False), "dtv-l2": (4, "l2", False),
            "grad-4d-l1": (4, "l1", True), "grad-4d-cb": (4, "cb", True)}
FD_KINKED = ("grad-4d-l1", "grad-4d-cb")


def fd_stmt(x, y, dirs, crit):
    ex = T.fd_responses(x, dirs == 4)
    ey = T.fd_responses(y, dirs == 4) if y is not None else [0.0] * dirs
    return SCALE * sum(T.rho(a - b, crit).sum() for a, b in zip(ex, ey))


@cache
def fd_ref(name):
    r = Ref()
    r.shape = SHAPES[name]
    numel = r.shape[0] * r.shape[1] * r.shape[2] * r.shape[3]

    def build(seed):
        x, y = U(r.shape, seed), U(r.shape, seed + 50000)
        e64 = [a - b for a, b in zip(T.fd_responses(x.double(), True), T.fd_responses(y.double(), True))]
        e32 = [a - b for a, b in zip(T.fd_responses(x, True), T.fd_responses(y, True))]
        e32_resp = max(float((a.double() - b).abs().max()) for a, b in zip(e32, e64))
        return x, y, T.near_zero_mask(x, y, "grad-4d-l1", e32_resp)

    r.seed = first_seed(case_seed(name) + 1, lambda s: float(build(s)[2].double().mean()) <= share_cap(numel))
    r.x, r.y, r.left_out = build(r.seed)
    r.v, r.g = {}, {}
    for n, (dirs, crit, with_y) in FD_NAMES.items():
        v64, g64 = autograd(lambda t: fd_stmt(t, r.y.to(t.dtype) if with_y else None, dirs, crit), r.x, D)
        v32, g32 = autograd(lambda t: fd_stmt(t, r.y.to(t.dtype) if with_y else None, dirs, crit), r.x, torch.float32)
        r.v[n], r.g[n] = (float(v64), float(v32)), (g64, g32)
    return r


def run_fd(r, layout, offs=(0, 0, 0), names=tuple(FD_NAMES), gs=None, fill=None):
    ops = _ops()
    x, y = Op(r.shape, layout, offs[0], r.x), Op(r.shape, layout, offs[1], r.y)
    gx, loss = Op(r.shape, layout, offs[2], data=fill, outer=SENT), Small()
    out = {}
    for n in names:
        dirs, crit, with_y = FD_NAMES[n]
        yt = y.t if with_y else None
        gx.reset()
        loss.reset()
        run_twice(lambda: ops.fd_loss_fwd(x.t, yt, layout, dirs, CRIT[crit], SCALE, loss.t), [x, y], [loss])
        run_twice(lambda: ops.fd_loss_bwd(x.t, yt, layout, dirs, CRIT[crit], SCALE, gst(gs), gx.t, accumulate=fill is not None), [x, y] + gsrc(gs), [gx])
        out[n] = (float(loss.result()[0]), gx.result())
    return out


def check_fd(cid, r, out):
    for n, (v, g) in out.items():
        check_value(cid, n + " value", v, *r.v[n])
        check_map(cid, n + " grad", g, *r.g[n], keep=~r.left_out if n in FD_KINKED else None)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(IMG))
def test_fd(name, layout):
    r = fd_ref(name)
    check_fd("%s-%s" % (name, LAYOUT_IDS[layout]), r, run_fd(r, layout))


# =====================================================================================================================
# 3. flat criteria (point_*, overflow_*)
# =====================================================================================================================
@cache
def flat_ref(n):
    r = Ref()
    r.shape = (1, 1, 1, n)
    r.a, r.b = U(r.shape, 300 + n, -0.5, 1.5), U(r.shape, 50300 + n)      # a leaves [0, 1] on both sides: the overflow criterion acts
    r.v, r.g = {}, {}
    for c in ("l2", "elastic", "cb"):
        f = lambda t, c=c: SCALE * T.rho(t - r.b.to(t.dtype), c).sum()
        (v64, g64), (v32, g32) = autograd(f, r.a, D), autograd(f, r.a, torch.float32)
        r.v[c], r.g[c] = (float(v64), float(v32)), (g64, g32)
    f = lambda t: SCALE * torch.log((t - t.clamp(0, 1)).abs() + 1).sum()
    (v64, g64), (v32, g32) = autograd(f, r.a, D), autograd(f, r.a, torch.float32)
    r.v["overflow"], r.g["overflow"] = (float(v64), float(v32)), (g64, g32)
    d = (r.a.double() - r.b.double()).abs()
    r.kink_free = bool((d > 1e-6).all()) and bool(((r.a - 0.0).abs() > 1e-6).all()) and bool(((r.a - 1.0).abs() > 1e-6).all())
    return r


def run_flat(r, off):
    ops = _ops()
    a, b = Op(r.shape, 0, off, r.a), Op(r.shape, 0, off, r.b)
    ga, loss = Op(r.shape, 0, off, outer=SENT), Small()
    out = {}
    for c in ("l2", "elastic", "cb", "overflow"):
        ga.reset()
        loss.reset()
        if c == "overflow":
            run_twice(lambda: ops.overflow_loss_fwd(a.t, SCALE, loss.t), [a], [loss])
            run_twice(lambda: ops.overflow_loss_bwd(a.t, SCALE, None, ga.t), [a], [ga])
        else:
            run_twice(lambda: ops.pointwise_loss_fwd(a.t, b.t, CRIT[c], SCALE, loss.t), [a, b], [loss])
            run_twice(lambda: ops.pointwise_loss_bwd(a.t, b.t, CRIT[c], SCALE, None, ga.t), [a, b], [ga])
        out[c] = (float(loss.result()[0]), ga.result())
    return out


@gpu
@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_flat_criteria(n):
    """px1 / thin / sill of the flat kernels: n around the group of four and the 256-thread block, the 16-byte path and (one float
    off) the scalar path; the gradients of the two paths are the same bits"""
    r = flat_ref(n)
    outs = [run_flat(r, off) for off in (0, 1, 4)]
    for off, out in zip((0, 1, 4), outs):
        for c, (v, g) in out.items():
            check_value("%s-flat-off%d" % (FLAT_IDS[FLAT_N.index(n)], off), c + " value", v, *r.v[c])
            check_map("%s-flat-off%d" % (FLAT_IDS[FLAT_N.index(n)], off), c + " grad", g, *r.g[c])
            assert same_bits(g, outs[0][c][1])


# =====================================================================================================================
# 4. frequency separation
# =====================================================================================================================
@cache
def fs_taps(kind):
    if kind == "asym":
        t = U((9,), 77, 0.02, 1.0)
        return t / t.sum()
    return TF.taps1d("gaussian")


def fs_low(x, taps):
    """L x as a 9 x 9 zero-padded correlation with the outer product of the taps (make_golden_freqsep.low with k2 given)"""
    k = taps.to(x.dtype)
    return TF.low(x, None, k2=torch.outer(k, k))


@cache
def fs_ref(name):
    r = Ref()
    r.taps = fs_taps("asym" if name == "taps-asym9" else "gaussian")
    r.shape = (1, 2, 19, 70) if name == "taps-asym9" else SHAPES[name]
    s = case_seed(name) + 2
    r.x, r.g = U(r.shape, s), U(r.shape, s + 1, -1.0, 1.0)
    o = U(r.shape, s + 2, 0.001, 0.999)                      # a GIVEN saved output with planted exact edges
    pick = U(r.shape, s + 3)
    r.o = torch.where(pick < 0.1, torch.zeros_like(o), torch.where(pick > 0.9, torch.ones_like(o), o))
    r.low = (fs_low(r.x.double(), r.taps), fs_low(r.x, r.taps))
    pre = [(t - fs_low(t, r.taps) + 1.0) / 2.0 for t in (r.x.double(), r.x)]
    r.pre_margin = float(torch.minimum(pre[0], 1 - pre[0]).min())
    r.high = (pre[0].clamp(0, 1), pre[1].clamp(0, 1))
    inside = (r.o > 0) & (r.o < 1)
    gp = [torch.where(inside, 0.5 * t, torch.zeros_like(t)) for t in (r.g.double(), r.g)]
    r.hb = tuple(t - fs_low(t, r.taps) for t in gp)
    return r


def run_fs(r, layout, offs=(0, 0, 0, 0, 0, 0), gs=None, fill=None):
    ops = _ops()
    tp = [float(v) for v in r.taps]
    x, g, o = Op(r.shape, layout, offs[0], r.x), Op(r.shape, layout, offs[1], r.g), Op(r.shape, layout, offs[2], r.o)
    lo, hi = Op(r.shape, layout, offs[3], data=fill, outer=SENT), Op(r.shape, layout, offs[4], outer=SENT)
    gx = Op(r.shape, layout, offs[5], data=fill, outer=SENT)
    acc = fill is not None
    run_twice(lambda: ops.freqsep_low(x.t, layout, tp, lo.t, gst(gs), accumulate=acc), [x] + gsrc(gs), [lo])
    run_twice(lambda: ops.freqsep_high_fwd(x.t, layout, tp, hi.t), [x], [hi])
    run_twice(lambda: ops.freqsep_high_bwd(g.t, o.t, layout, tp, gx.t, gst(gs), accumulate=acc), [g, o] + gsrc(gs), [gx])
    return {"low": lo.result(), "high": hi.result(), "hb": gx.result()}


def check_fs(cid, r, out):
    check_map(cid, "freqsep low", out["low"], *r.low)
    check_map(cid, "freqsep high", out["high"], *r.high)
    check_map(cid, "freqsep high bwd", out["hb"], *r.hb)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(IMG) + ["taps-asym9"])
def test_freqsep(name, layout):
    r = fs_ref(name)
    check_fs("%s-%s" % (name, LAYOUT_IDS[layout]), r, run_fs(r, layout))


# =====================================================================================================================
# 5. spatial profile losses
# =====================================================================================================================
SPL_GS = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in (0.6, 1.3, 0.45, 0.85))      # one per family, all different


def spl_stmt(x, y, mask, gs=(1.0, 1.0, 1.0, 1.0)):
    """the sum over the selected families (RGB 1, YUV 2, DIMG 4, DYUV 8) of gs[family] x its SPLoss traces"""
    v = 0.0
    if mask & 1:
        v = v + gs[0] * TS.spl_trace(x, y)
    if mask & 2:
        v = v + gs[1] * TS.spl_trace(TS.rgb_to_yuv(x), TS.rgb_to_yuv(y))
    for bit, f, g in ((4, lambda t: t, gs[2]), (8, TS.rgb_to_yuv, gs[3])):
        if mask & bit:
            (xh, xv), (yh, yv) = TS.differences(f(x)), TS.differences(f(y))
            v = v + g * (TS.spl_trace(xv, yv) + TS.spl_trace(xh, yh))
    return v


@cache
def spl_ref(name):
    r = Ref()
    r.shape = SPL_SHAPES[name]
    r.mask = 15 if r.shape[1] == 3 else 5
    s = case_seed(name) + 3
    r.x, r.y = U(r.shape, s, 0.05, 1.0), U(r.shape, s + 50000, 0.05, 1.0)
    y = r.y
    (v64, g64) = autograd(lambda t: spl_stmt(t, y.double(), r.mask), r.x, D)
    (v32, g32) = autograd(lambda t: spl_stmt(t, y, r.mask), r.x, torch.float32)
    r.v, r.g = (float(v64), float(v32)), (g64, g32)
    return r


@cache
def spl_ref_gs(name):
    """the gradient with one gscale per family (the value launch takes none)"""
    r = spl_ref(name)
    return tuple(autograd(lambda t: spl_stmt(t, r.y.to(t.dtype), r.mask, SPL_GS), r.x, dt)[1] for dt in (D, torch.float32))


def run_spl(r, layout, offs=(0, 0, 0), gs=None, fill=None):
    ops = _ops()
    x, y = Op(r.shape, layout, offs[0], r.x), Op(r.shape, layout, offs[1], r.y)
    gx, loss = Op(r.shape, layout, offs[2], data=fill, outer=SENT), Small(5)
    coef = Small(ops.spl_coef(x.t, r.mask).numel())
    run_twice(lambda: ops.spl_loss_fwd(x.t, y.t, layout, r.mask, False, loss.t, coef.t), [x, y], [loss, coef])
    run_twice(lambda: ops.spl_loss_bwd(x.t, y.t, layout, r.mask, False, coef.t, gst(gs), gx.t, accumulate=fill is not None),
              [x, y, coef] + gsrc(gs), [gx])
    assert bool(torch.isfinite(coef.result()).all())
    return {"loss": loss.result(), "gx": gx.result()}


def check_spl(cid, r, out):
    assert bool(torch.isfinite(out["loss"]).all())
    check_value(cid, "spl value", float(out["loss"][4]), *r.v)
    check_map(cid, "spl grad", out["gx"], *r.g)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(SPL))
def test_spl(name, layout):
    r = spl_ref(name)
    check_spl("%s-%s" % (name, LAYOUT_IDS[layout]), r, run_spl(r, layout))


# =====================================================================================================================
# 6. vecsill: the 16-byte path against the scalar path, operand by operand
# =====================================================================================================================
def offset_sets(nops, W):
    """aligned; every operand in turn 1, 2 or 3 floats off; all operands 4 floats off"""
    sets = [(0,) * nops]
    for i in range(nops):
        sets.append(tuple(1 + (i + W // 4) % 3 if j == i else 0 for j in range(nops)))
    sets.append((4,) * nops)
    return sets


def equal_outputs(a, b):
    if isinstance(a, dict):
        return all(equal_outputs(a[k], b[k]) for k in a)
    if isinstance(a, tuple):
        return all(equal_outputs(p, q) for p, q in zip(a, b))
    return a == b if isinstance(a, float) else same_bits(a, b)


@gpu
@pytest.mark.parametrize("family", ["hfen", "fd", "freqsep", "spl"])
@pytest.mark.parametrize("W", VEC_W)
def test_vecsill(W, family):
    name = "vecsill-17x%d" % W
    ref, run, check, nops = {"hfen": (filter_ref, run_filter, check_filter, 5), "fd": (fd_ref, run_fd, check_fd, 3),
                             "freqsep": (fs_ref, run_fs, check_fs, 6), "spl": (spl_ref, run_spl, check_spl, 3)}[family]
    r = ref(name)
    base = None
    for offs in offset_sets(nops, W):
        out = run(r, 0, offs=offs)
        if base is None:
            base = out
            check("%s-%s" % (name, family), r, out)
        assert equal_outputs(base, out), (family, W, offs)


# =====================================================================================================================
# 7. epi: accumulate, gscale, identical images
# =====================================================================================================================
EPI_FAMILIES = {"hfen": (lambda n: filter_ref(n), lambda *a, **k: run_filter(*a, **k), ["gx"], 5),
                "fd": (lambda n: fd_ref(n), lambda *a, **k: run_fd(*a, names=("dtv-l2", "grad-4d-l2"), **k), ["dtv-l2", "grad-4d-l2"], 3),
                "freqsep": (lambda n: fs_ref(n), lambda *a, **k: run_fs(*a, **k), ["low", "hb"], 6),
                "spl": (lambda n: spl_ref(n), lambda *a, **k: run_spl(*a, **k), ["gx"], 3)}


def epi_refs(family, name):
    """-> {key: ((r64, r32) with a null gscale, (r64, r32) with the gscale tensor)}"""
    r = EPI_FAMILIES[family][0](name)
    g32 = torch.tensor(GS, dtype=torch.float32)
    scaled = lambda p: (GS * p[0], g32 * p[1])
    if family == "spl":
        return {"gx": (r.g, spl_ref_gs(name))}
    plain = {"hfen": lambda: {"gx": r.adj}, "fd": lambda: {k: r.g[k] for k in ("dtv-l2", "grad-4d-l2")},
             "freqsep": lambda: {"low": r.low, "hb": r.hb}}[family]()
    return {k: (v, scaled(v)) for k, v in plain.items()}


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("family", list(EPI_FAMILIES))
@pytest.mark.parametrize("name", list(EPI))
def test_epi_accumulate_and_gscale(name, family, layout):
    """null gscale, a gscale tensor (SPL: four different ones, one per family), accumulate onto a pre-filled gx.  17 x 65 and
    channels-last take the scalar epilogues; NCHW at 17 x 64 / 17 x 72 the 16-byte ones, whose accumulated result must also be the
    bits of the scalar epilogue (first operand one float off)"""
    ref, run, keys, nops = EPI_FAMILIES[family]
    r = ref(name)
    cid = "%s-%s-%s" % (name, family, LAYOUT_IDS[layout])
    fill = U(r.shape, 4711, -2.0, 2.0)
    gs = lambda: Small(data=SPL_GS if family == "spl" else [GS])
    unit, fresh, acc = run(r, layout), run(r, layout, gs=gs()), run(r, layout, gs=gs(), fill=fill)
    pick = (lambda o, k: o[k][1]) if family == "fd" else (lambda o, k: o[k])
    for k, (null, scaled) in epi_refs(family, name).items():
        check_map(cid, k + " null gscale", pick(unit, k), *null)
        check_map(cid, k + " gscale", pick(fresh, k), *scaled)
        assert torch.equal(pick(acc, k), fill + pick(fresh, k)), (cid, k)          # one fp32 addition
    if layout == 0 and r.shape[3] % 4 == 0:
        scalar = run(r, 0, offs=(1,) + (0,) * (nops - 1), gs=gs(), fill=fill)
        for k in keys:
            assert same_bits(pick(scalar, k), pick(acc, k)), (cid, k)


@gpu
@pytest.mark.parametrize("off", [0, 1], ids=["vec", "scalar"])
@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_epi_flat_accumulate_and_gscale(n, off):
    """point_bwd / overflow_bwd with a gscale tensor and onto a pre-filled ga: the 16-byte body and the scalar tail both accumulate"""
    ops = _ops()
    r = flat_ref(n)
    cid = "epi-flat-%s-%s" % (FLAT_IDS[FLAT_N.index(n)], "scalar" if off else "vec")
    fill = U(r.shape, 4713, -2.0, 2.0)
    g32 = torch.tensor(GS, dtype=torch.float32)
    a, b = Op(r.shape, 0, off, r.a), Op(r.shape, 0, off, r.b)
    for c in ("elastic", "overflow"):
        res = []
        for f in (None, fill):
            ga, gs = Op(r.shape, 0, off, data=f, outer=SENT), Small(data=[GS])
            if c == "overflow":
                run_twice(lambda: ops.overflow_loss_bwd(a.t, SCALE, gs.t, ga.t, accumulate=f is not None), [a, gs], [ga])
            else:
                run_twice(lambda: ops.pointwise_loss_bwd(a.t, b.t, CRIT[c], SCALE, gs.t, ga.t, accumulate=f is not None), [a, b, gs], [ga])
            res.append(ga.result())
        check_map(cid, c + " grad gscale", res[0], GS * r.g[c][0], g32 * r.g[c][1])
        assert torch.equal(res[1], fill + res[0]), (cid, c)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", ["px1-1x1", "thin-2x4", "thin-17x1", "sill-16x64"])
def test_identical_images_give_exactly_zero(name, layout):
    ops = _ops()
    shape = IMG[name]
    xs = U(shape, 99)
    x, y, loss = Op(shape, layout, 0, xs), Op(shape, layout, 0, xs), Small()
    gx = Op(shape, layout, 0, outer=SENT)
    tp = [float(v) for v in T.log_taps().flatten()]
    for c in ("l1", "l2", "elastic", "clipl1"):
        for call in (lambda: ops.filter_loss_fwd(x.t, y.t, layout, tp, 15, CRIT[c], SCALE, loss.t, gx.t),
                     lambda: ops.fd_loss_fwd(x.t, y.t, layout, 4, CRIT[c], SCALE, loss.t),
                     lambda: ops.pointwise_loss_fwd(x.t, y.t, CRIT[c], SCALE, loss.t)):
            loss.reset()
            call()
            assert float(loss.result()[0]) == 0.0, (name, c)
        gx.reset()
        ops.fd_loss_bwd(x.t, y.t, layout, 4, CRIT[c], SCALE, None, gx.t)
        assert float(gx.result().abs().max()) == 0.0 and gx.outside_ok()


# =====================================================================================================================
# 8. SSIM, the pooling between MS-SSIM levels, the combine kernel
# =====================================================================================================================
@cache
def ssim_taps(K, asym):
    if asym:
        t = U((K,), 640 + K, 0.05, 1.0)
        return t / t.sum() if K > 1 else torch.tensor([0.75])
    return TG.window(K, 1.5 * K / 11)


def ssim_pair(shape, seed):
    """hr: uniform noise in [0.1, 0.9]; sr = hr + 0.02 U(-1, 1): every window has variance, cs and ssim stay near 1"""
    hr = U(shape, seed, 0.1, 0.9)
    return (hr.double() + 0.02 * U(shape, seed + 50000, -1.0, 1.0).double()).float(), hr


def ssim_obj(x, y, shave, taps, coef):
    H, W = x.shape[-2:]
    m, cs, clamped = TG.maps(x[..., shave:H - shave, shave:W - shave], y[..., shave:H - shave, shave:W - shave], taps, C1, C2)
    c = coef.to(x.dtype)
    obj = (c[:, 0].view(-1, 1, 1, 1) * m).sum() + (c[:, 1].view(-1, 1, 1, 1) * cs).sum()
    return obj, m, cs, clamped


@cache
def ssim_ref(name, planted=False):
    r = Ref()
    N, C, H, W, r.shave, r.K, asym = SSIM[name]
    r.shape, r.taps = (N, C, H, W), ssim_taps(r.K, asym)
    r.x, r.y = ssim_pair(r.shape, case_seed(name) + 4)
    if planted:
        r.x = r.x.clone()
        r.x[..., 12:36, 14:38] = 0.3                        # a constant patch: sigma1_sq rounds around 0
    oh, ow = H - 2 * r.shave - r.K + 1, W - 2 * r.shave - r.K + 1
    r.count = C * oh * ow
    r.coef = torch.tensor([[(1.0 + 0.25 * n) / r.count, (0.37 - 0.1 * n) / r.count] for n in range(N)], dtype=torch.float32)
    _, m64, cs64, r.clamped64 = ssim_obj(r.x.double(), r.y.double(), r.shave, r.taps, r.coef)
    _, m32, cs32, r.clamped32 = ssim_obj(r.x, r.y, r.shave, r.taps, r.coef)
    r.sums = (torch.stack((m64.sum((1, 2, 3)), cs64.sum((1, 2, 3))), 1), torch.stack((m32.double().sum((1, 2, 3)), cs32.double().sum((1, 2, 3))), 1))
    r.means = (float(m64.mean((1, 2, 3)).min()), float(cs64.mean((1, 2, 3)).min()))
    if not planted:
        r.g = tuple(autograd(lambda t: ssim_obj(t, r.y.to(t.dtype), r.shave, r.taps, r.coef)[0], r.x, dt)[1] for dt in (D, torch.float32))
    return r


def run_ssim(r, layout, gs=None, fill=None, bwd=True):
    ops = _ops()
    tp = [float(v) for v in r.taps]
    N = r.shape[0]
    x, y = Op(r.shape, layout, 0, r.x), Op(r.shape, layout, 0, r.y)
    sums = Small(2 * N, torch.float64)
    run_twice(lambda: ops.ssim_fwd(x.t, y.t, layout, r.shave, tp, C1, C2, sums.t), [x, y], [sums])
    out = {"sums": sums.result().view(N, 2)}
    value, coef = Small(), Small(2 * N)
    run_twice(lambda: ops.msssim_combine(sums.t, 1, N, [r.count], None, 0, value.t, coef.t), [sums], [value, coef])
    out["value"], out["coef"] = float(value.result()[0]), coef.result().view(N, 2)
    if bwd:
        gx = Op(r.shape, layout, 0, data=fill, outer=SENT)
        cf = Small(data=r.coef.flatten())
        run_twice(lambda: ops.ssim_bwd(x.t, y.t, layout, r.shave, tp, C1, C2, cf.t, gst(gs), gx.t, accumulate=fill is not None),
                  [x, y, cf] + gsrc(gs), [gx])
        out["gx"] = gx.result()
    return out


def check_ssim_value(cid, r, out):
    N = r.shape[0]
    for n in range(N):
        for j, what in enumerate(("sum ssim", "sum cs")):
            check_value(cid, "%s[%d]" % (what, n), float(out["sums"][n, j]), float(r.sums[0][n, j]), float(r.sums[1][n, j]))
    v64, v32 = float(r.sums[0][:, 0].sum()) / (r.count * N), float(r.sums[1][:, 0].sum()) / (r.count * N)
    check_value(cid, "ssim mean", out["value"], v64, v32)
    want = torch.tensor([[1.0 / (float(r.count) * N), 0.0]] * N, dtype=torch.float64).float()
    assert torch.equal(out["coef"], want), cid                 # one correctly rounded division


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(SSIM))
def test_ssim(name, layout):
    r = ssim_ref(name)
    cid = "%s-%s" % (name, LAYOUT_IDS[layout])
    out = run_ssim(r, layout)
    check_ssim_value(cid, r, out)
    check_map(cid, "ssim grad", out["gx"], *r.g)
    s, (H, W) = r.shave, r.shape[2:]
    if s:
        border = torch.ones(r.shape, dtype=torch.bool)
        border[..., s:H - s, s:W - s] = False
        assert float(out["gx"][border].abs().max()) == 0.0     # the shaved border carries no gradient


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_ssim_planted_clamp_value(layout):
    r = ssim_ref(CLAMP_CASE, planted=True)
    check_ssim_value("sill-planted-clamp-%s" % LAYOUT_IDS[layout], r, run_ssim(r, layout, bwd=False))


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_epi_ssim_accumulate_and_gscale(layout):
    r = ssim_ref("planes-N3C2-20x37")
    cid = "epi-ssim-%s" % LAYOUT_IDS[layout]
    fill = U(r.shape, 4712, -2.0, 2.0)
    fresh, acc = run_ssim(r, layout, gs=Small(data=[GS]))["gx"], run_ssim(r, layout, gs=Small(data=[GS]), fill=fill)["gx"]
    check_map(cid, "ssim grad gscale", fresh, GS * r.g[0], torch.tensor(GS, dtype=torch.float32) * r.g[1])
    assert torch.equal(acc, fill + fresh)                      # also: the shaved border keeps the fill (fresh is 0 there)


@cache
def pool_ref(name):
    r = Ref()
    N, C, H, W, r.shave = POOL[name]
    r.shape = (N, C, H, W)
    s = case_seed(name) + 5
    r.x, r.y = U(r.shape, s), U(r.shape, s + 1)
    h, w = H - 2 * r.shave, W - 2 * r.shave
    r.oshape = (N, C, (h + 2 * (h & 1) - 2) // 2 + 1, (w + 2 * (w & 1) - 2) // 2 + 1)
    cut = lambda t: t[..., r.shave:H - r.shave, r.shave:W - r.shave]
    pool = lambda t: F.avg_pool2d(cut(t), 2, padding=(h % 2, w % 2))
    r.px, r.py = (pool(r.x.double()), pool(r.x)), (pool(r.y.double()), pool(r.y))
    r.gc, r.gf = U(r.oshape, s + 2, -1.0, 1.0), U(r.shape, s + 3, -1.0, 1.0)
    up = autograd(lambda t: (pool(t) * r.gc).sum(), r.x, torch.float32)[1]      # 0.25 gc at the pixels of the region: exact
    r.bwd = r.gf + up                                                           # one fp32 addition
    return r


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("name", list(POOL))
def test_avgpool2_pad(name, layout):
    ops = _ops()
    r = pool_ref(name)
    cid = "%s-pool-%s" % (name, LAYOUT_IDS[layout])
    x, y = Op(r.shape, layout, 0, r.x), Op(r.shape, layout, 0, r.y)
    xo, yo = Op(r.oshape, 0, 0, outer=SENT), Op(r.oshape, 0, 0, outer=SENT)
    assert ops.avgpool2_pad_dims(r.shape[2], r.shape[3], r.shave) == tuple(r.oshape[2:])
    run_twice(lambda: ops.avgpool2_pad_fwd(x.t, y.t, layout, r.shave, xo.t, yo.t), [x, y], [xo, yo])
    check_map(cid, "pool fwd x", xo.result(), *r.px)
    check_map(cid, "pool fwd y", yo.result(), *r.py)
    gc, gf = Op(r.oshape, 0, 0, r.gc), Op(r.shape, layout, 0, data=r.gf, outer=SENT)
    run_twice(lambda: ops.avgpool2_pad_bwd(gc.t, gf.t, layout, r.shave), [gc], [gf])
    assert torch.equal(gf.result(), r.bwd), cid


MS_SHAVE, MS_SHAPE = 4, (2, 3, 31, 35)                      # 23 x 27 after the shave


@cache
def ms_ref():
    r = Ref()
    r.x, r.y = ssim_pair(MS_SHAPE, 8080)
    r.table = TG.level_table(MS_SHAPE[2] - 2 * MS_SHAVE, MS_SHAPE[3] - 2 * MS_SHAVE)
    d64, d32 = {}, {}
    f = lambda t, d: TG.restate(t, r.y.to(t.dtype), "ms-ssim", MS_SHAVE, detail=d)
    (v64, g64), (v32, g32) = autograd(lambda t: f(t, d64), r.x, D), autograd(lambda t: f(t, d32), r.x, torch.float32)
    r.v, r.g, r.detail = (float(v64), float(v32)), (g64, g32), (d64, d32)
    return r


@gpu
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_msssim_levels(layout):
    """the shrinking windows of level_table(23, 27): ssim_fwd, avgpool2_pad_fwd, msssim_combine, then ssim_bwd / avgpool2_pad_bwd back"""
    ops = _ops()
    r = ms_ref()
    cid = "taps-msssim-23x27-%s" % LAYOUT_IDS[layout]
    N, C = MS_SHAPE[:2]
    L = len(r.table)
    x, y = Op(MS_SHAPE, layout, 0, r.x), Op(MS_SHAPE, layout, 0, r.y)
    weights = [float(torch.tensor(w, dtype=torch.float32)) for w in TG.MS_WEIGHTS]

    def pipeline():
        """every intermediate (the level sums, the pooled images, the coefficients, the coarse gradients) is a guarded slice too"""
        sums, guarded = Small(L * N * 2, torch.float64), []
        sv = sums.t.view(L, N, 2)
        cx, cy, clay, cshave, pyramid, counts = x.t, y.t, layout, MS_SHAVE, [], []
        for i, (h, w, k, sigma) in enumerate(r.table):
            taps = [float(v) for v in TG.window(k, sigma)]
            ops.ssim_fwd(cx, cy, clay, cshave, taps, C1, C2, sv[i])
            counts.append(C * (h - k + 1) * (w - k + 1))
            pyramid.append((cx, cy, clay, cshave, taps))
            if i < L - 1:
                nx, ny = (Op((N, C) + tuple(r.table[i + 1][:2]), 0, outer=SENT) for _ in range(2))
                ops.avgpool2_pad_fwd(cx, cy, clay, cshave, nx.t, ny.t)
                guarded += [nx, ny]
                cx, cy, clay, cshave = nx.t, ny.t, 0, 0
        value, coef = Small(), Small(L * N * 2)
        ops.msssim_combine(sums.t, L, N, counts, weights, 1, value.t, coef.t)
        cv = coef.t.view(L, N, 2)
        coarse = None
        for i in range(L - 1, -1, -1):
            cx, cy, clay, cshave, taps = pyramid[i]
            g = Op(tuple(cx.shape), clay, 0, outer=SENT)
            ops.ssim_bwd(cx, cy, clay, cshave, taps, C1, C2, cv[i], None, g.t)
            if coarse is not None:
                ops.avgpool2_pad_bwd(coarse.t, g.t, clay, cshave)
            guarded.append(g)
            coarse = g
        for o in guarded + [sums, value, coef]:
            assert o.outside_ok(), "wrote outside a slice"
        return float(value.result()[0]), coarse.result()

    (v1, g1), (v2, g2) = pipeline(), pipeline()
    assert v1 == v2 and same_bits(g1, g2)
    assert x.unchanged() and y.unchanged()
    check_value(cid, "ms-ssim value", v1, *r.v)
    check_map(cid, "ms-ssim grad", g1, *r.g)


# =====================================================================================================================
# 9. the device-free test
# =====================================================================================================================
def _refusals():
    from trainner_amd import hip
    lib = hip.load()
    buf = torch.zeros(4096, dtype=torch.float32)
    dbl = torch.zeros(64, dtype=torch.float64)
    p, q = buf.data_ptr(), buf.data_ptr() + 4096
    w11 = (ctypes.c_float * 11)(*[1.0 / 11] * 11)
    w9 = (ctypes.c_float * 9)(*[1.0 / 9] * 9)
    w225 = (ctypes.c_float * 225)(*[0.0] * 225)
    ws, wsb = dbl.data_ptr(), 64 * 8
    return lib, [
        ("ssim_fwd 10x10 K11", "does not fit", lambda: lib.tnr_ssim_fwd(p, q, 1, 1, 10, 10, 0, 0, w11, 11, C1, C2, ws, ws, wsb, None)),
        ("ssim_fwd 18x18 K11 shave4", "does not fit", lambda: lib.tnr_ssim_fwd(p, q, 1, 1, 18, 18, 0, 4, w11, 11, C1, C2, ws, ws, wsb, None)),
        ("ssim_bwd 10x10 K11", "does not fit", lambda: lib.tnr_ssim_bwd(p, q, 1, 1, 10, 10, 0, 0, w11, 11, C1, C2, p, None, q, 0, None)),
        ("ssim_fwd even window", "odd number of taps", lambda: lib.tnr_ssim_fwd(p, q, 1, 1, 12, 12, 0, 0, w11, 10, C1, C2, ws, ws, wsb, None)),
        ("ssim_fwd C5", "1..4 channels", lambda: lib.tnr_ssim_fwd(p, q, 1, 5, 11, 11, 0, 0, w11, 11, C1, C2, ws, ws, wsb, None)),
        ("ssim_bwd C5", "1..4 channels", lambda: lib.tnr_ssim_bwd(p, q, 1, 5, 11, 11, 0, 0, w11, 11, C1, C2, p, None, q, 0, None)),
        ("ssim_fwd shave eats all", "nothing left", lambda: lib.tnr_ssim_fwd(p, q, 1, 1, 8, 8, 0, 4, w11, 1, C1, C2, ws, ws, wsb, None)),
        ("avgpool2_pad_fwd 1x1", "cannot be pooled", lambda: lib.tnr_avgpool2_pad_fwd(p, q, 1, 1, 1, 1, 0, 0, p, q, None)),
        ("avgpool2_pad_bwd 1x1", "cannot be pooled", lambda: lib.tnr_avgpool2_pad_bwd(p, q, 1, 1, 1, 1, 0, 0, None)),
        ("avgpool2_pad_fwd C5", "1..4 channels", lambda: lib.tnr_avgpool2_pad_fwd(p, q, 1, 5, 2, 2, 0, 0, p, q, None)),
        ("spl_loss_fwd C5", "at most 4 channels", lambda: lib.tnr_spl_loss_fwd(p, q, 1, 5, 4, 4, 0, 1, 0, p, q, ws, wsb, None)),
        ("spl_loss_bwd C5", "at most 4 channels", lambda: lib.tnr_spl_loss_bwd(p, q, 1, 5, 4, 4, 0, 1, 0, p, None, p + 64, 0, None)),
        ("spl_loss_fwd yuv C1", "need 3 channels", lambda: lib.tnr_spl_loss_fwd(p, q, 1, 1, 4, 4, 0, 2, 0, p, q, ws, wsb, None)),
        ("filter_loss_fwd K17", "odd number of taps", lambda: lib.tnr_filter_loss_fwd(p, q, 1, 1, 1, 1, 0, w225, 17, 1, 1.0, p, None, ws, wsb, None)),
        ("filter_loss_bwd K2", "odd number of taps", lambda: lib.tnr_filter_loss_bwd(p, 1, 1, 1, 1, 0, w225, 2, 1.0, None, q, 0, None)),
        ("fd_loss_fwd 0x1", "bad shape", lambda: lib.tnr_fd_loss_fwd(p, q, 1, 1, 0, 1, 0, 4, 1, 1.0, p, ws, wsb, None)),
        ("fd_loss_bwd dirs3", "dirs not 2 / 4", lambda: lib.tnr_fd_loss_bwd(p, q, 1, 1, 1, 1, 0, 3, 1, 1.0, None, p + 64, 0, None)),
        ("freqsep_low W0", "bad shape", lambda: lib.tnr_freqsep_low(p, 1, 1, 1, 0, 0, w9, None, q, 0, None)),
        ("freqsep_high_bwd aliased", "aliases", lambda: lib.tnr_freqsep_high_bwd(p, q, 1, 1, 1, 1, 0, w9, None, q, 0, None)),
        ("pointwise_loss_fwd n0", "bad arguments", lambda: lib.tnr_pointwise_loss_fwd(p, q, 0, 1, 1.0, p, ws, None)),
        ("overflow_loss_bwd aliased", "bad arguments", lambda: lib.tnr_overflow_loss_bwd(p, 4, 1.0, None, p, 0, None)),
    ]


def case_bytes():
    shapes = [filter_ref(n).shape for n in list(SHAPES) + list(HFEN_TAPS)] + list(SPL_SHAPES.values()) + [v[:4] for v in SSIM.values()]
    shapes += [v[:4] for v in POOL.values()] + [MS_SHAPE, (1, 1, 1, max(FLAT_N))]
    return max(4 * s[0] * s[1] * s[2] * s[3] for s in shapes)


# The cases whose fp32 restatement is exact although the reference is not zero, so that the additive term alone is the bound: one
# pixel, and the l1 gradients of the thinnest images (a few signs times SCALE).  The HFEN l1 map is sign(e): away from the left-out
# band it is exact in every case, by construction.
CARRIED = {("px1-1x1", "grad-4d-l1"), ("px1-1x1", "spl value"), ("thin-17x1", "grad-4d-l1"), ("thin-1x65", "grad-4d-l1"), ("thin-2x4", "grad-4d-l1")}


def test_inputs_and_references():
    # the classes are all there, and sit where the kernels' constants put them
    TW, TH, FT, BH, BW, RT = 64, 16, 32, 16, 32, 4
    for table in (IMG, SPL, SSIM):
        assert {n.split("-")[0] for n in table} >= {"px1", "thin", "sill", "planes"}
    assert {h for h, _ in SILL_HW} == {TH - 1, TH, TH + 1, 2 * TH} and {w for _, w in SILL_HW} == {TW - 1, TW, TW + 1, 2 * TW}
    assert {SPL[n][2] for n in SPL if n.startswith("sill-6")} == {RT * TH - 1, RT * TH, RT * TH + 1}
    maps = {(v[2] - 2 * v[4] - v[5] + 1, v[3] - 2 * v[4] - v[5] + 1) for n, v in SSIM.items() if n.startswith("sill-map")}
    assert maps >= {(FT - 1, FT + 1), (FT, FT), (FT + 1, FT - 1)}
    assert {SSIM[n][2:4] for n in SSIM if n.startswith("sill-bwd")} == {(BH - 1, BW - 1), (BH, BW), (BH + 1, BW + 1)}
    assert all(v[2] - 2 * v[4] == v[5] and v[3] - 2 * v[4] == v[5] for n, v in SSIM.items() if n.startswith("px1"))
    assert all(w % 4 == 0 for w in VEC_W) and (2, 4) in THIN_HW and (5, 8) in THIN_HW
    n_, c_, h_, w_ = IMG["planes-N3C4-49x321"]
    assert n_ * c_ * -(-h_ // TH) * -(-w_ // TW) > 256
    n_, c_, h_, w_, s_, k_, _ = SSIM["planes-N3C4-139x139"]
    assert n_ * c_ * (-(-(h_ - 2 * s_ - k_ + 1) // FT)) * (-(-(w_ - 2 * s_ - k_ + 1) // FT)) > 256
    assert max(FLAT_N) // 256 > 256
    for nops in (3, 5, 6):
        for W in VEC_W:
            sets = offset_sets(nops, W)
            assert sets[0] == (0,) * nops and sets[-1] == (4,) * nops and len(sets) == nops + 2
            assert all(sum(1 for o in s if o) == 1 and max(s) in (1, 2, 3) for s in sets[1:-1])
    # the widest single-plane case's halo rows fit the NaN margin
    assert PAD % 4 == 0 and PAD >= 7 * max(s[3] for s in IMG.values() if s[0] * s[1] == 1) + 7

    carried = set()     # (case, what) whose fp32 restatement is exact although the reference is not zero: the additive term carries them

    def nonzero(cid, what, r64, r32, keep=None):
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), (cid, what)
        if e32_term(r64, r32, keep) == 0.0 and float(r64.abs().max()) > 0.0:
            carried.add((cid, what))

    def nonzero_value(cid, what, v64, v32):
        assert math.isfinite(v64) and math.isfinite(v32), (cid, what)
        if v32 == v64 and v64 != 0.0:
            carried.add((cid, what))

    # HFEN: the K-tap statement pinned to the tool's at K = 15, and to the centred 15 x 15 table below it
    x, y = U((1, 2, 19, 70), 1), U((1, 2, 19, 70), 2)
    t15 = asym_taps(15)
    assert float((hfen_stmt(x.double() - y.double(), t15) - T.hfen_response(x.double(), y.double(), t15)).abs().max()) <= 1e-12
    m = U((1, 2, 19, 70), 3, -1.0, 1.0).double()
    assert float((hfen_adj(m, t15) - T.adjoint(m, t15)).abs().max()) <= 1e-12
    for K in (1, 3, 7):
        big = torch.zeros(15, 15)
        o = (15 - K) // 2
        big[o:o + K, o:o + K] = asym_taps(K)
        assert float((hfen_stmt(x.double() - y.double(), asym_taps(K)) - T.hfen_response(x.double(), y.double(), big)).abs().max()) <= 1e-12
        assert float((hfen_adj(m, asym_taps(K)) - T.adjoint(m, big)).abs().max()) <= 1e-12
        assert not torch.equal(asym_taps(K), asym_taps(K).flip(0, 1)) or K == 1
        assert K == 1 or not torch.equal(asym_taps(K), asym_taps(K).t())
    for name in list(SHAPES) + list(HFEN_TAPS):
        r = filter_ref(name)
        numel = r.x.numel()
        assert r.near_share <= share_cap(numel), (name, r.near_share)
        for c in ("l2", "l1"):
            nonzero_value(name, "hfen value " + c, *r.v[c])
            nonzero(name, "hfen map " + c, *r.map[c], keep=r.far if c == "l1" else None)
        nonzero(name, "hfen adjoint", *r.adj)
        assert float(r.adj[0].abs().max()) > 0 and float(r.e64.abs().max()) > 0
    for name in SHAPES:
        r = fd_ref(name)
        assert float(r.left_out.double().mean()) <= share_cap(r.x.numel()), name
        for n in FD_NAMES:
            nonzero(name, n, *r.g[n], keep=~r.left_out if n in FD_KINKED else None)
            nonzero_value(name, n + " value", *r.v[n])
        N, C, H, W = r.shape
        if H > 1 or W > 1:
            assert float(r.g["grad-4d-l2"][0].abs().max()) > 0
    for n in FLAT_N:
        r = flat_ref(n)
        assert r.kink_free or n > 1000, n                    # |a - b| and the clamp edges stay clear of the kinks
        d = (r.a.double() - r.b.double()).abs()
        assert float((d <= 1e-6).double().mean()) <= share_cap(n) and float(((r.a.abs() <= 1e-6) | ((r.a - 1).abs() <= 1e-6)).double().mean()) <= share_cap(n)
        for c in r.g:
            nonzero(FLAT_IDS[FLAT_N.index(n)], "flat " + c, *r.g[c])
            nonzero_value(FLAT_IDS[FLAT_N.index(n)], "flat %s value" % c, *r.v[c])
    # freqsep: no clamp acts on the forward cases; the symmetric table is the tool's; the asymmetric one is neither flipped nor even
    k = fs_taps("gaussian")
    xx = U((1, 2, 19, 70), 5).double()
    assert float((fs_low(xx, k) - TF.low_separable(xx, "gaussian")).abs().max()) <= 1e-12
    assert not torch.equal(fs_taps("asym"), fs_taps("asym").flip(0))
    for name in list(SHAPES) + ["taps-asym9"]:
        r = fs_ref(name)
        assert r.pre_margin >= 0.01, (name, r.pre_margin)
        for what in ("low", "high", "hb"):
            nonzero(name, "freqsep " + what, *getattr(r, what))
        if r.o.numel() >= 64:
            assert bool((r.o == 0).any()) and bool((r.o == 1).any())
    for name in SPL_SHAPES:
        r = spl_ref(name)
        nonzero_value(name, "spl value", *r.v)
        nonzero(name, "spl grad", *r.g)
    for name in EPI:
        nonzero(name, "spl grad, four gscales", *spl_ref_gs(name))
        assert len(set(SPL_GS)) == 4 and SPL_SHAPES[name][1] == 3      # every family is on and has its own scale
    # SSIM: no clamped variance in either precision, every mean above 0.5; the planted case does clamp
    for name in SSIM:
        r = ssim_ref(name)
        assert r.clamped64 == 0 and r.clamped32 == 0, (name, r.clamped64, r.clamped32)
        assert min(r.means) > 0.5, (name, r.means)
        nonzero(name, "ssim grad", *r.g)
        K, asym = SSIM[name][5], SSIM[name][6]
        if asym and K > 1:
            assert not torch.equal(r.taps, r.taps.flip(0))
    p = ssim_ref(CLAMP_CASE, planted=True)
    assert p.clamped32 + p.clamped64 > 0
    ms = ms_ref()
    assert [t[2] for t in ms.table] == [11, 11, 5, 3, 1] and all(t[0] % 2 or t[1] % 2 for t in ms.table[:1])
    assert [t[:2] for t in ms.table] == [(23, 27), (12, 14), (6, 7), (3, 4), (2, 2)]
    for d in ms.detail:
        assert d["clamped"] == 0
        assert all(float(cs.min()) > 0.5 for _, cs in d["levels"][:-1]) and float(d["levels"][-1][0].min()) > 0.5
    nonzero("msssim", "grad", *ms.g)
    for name in POOL:
        r = pool_ref(name)
        nonzero(name, "pool", *r.px)
    # refusals: the library's own message, before any launch (no device is needed to get them)
    lib, calls = _refusals()
    for what, frag, call in calls:
        rc = call()
        msg = (lib.tnr_last_error() or b"").decode()
        assert rc != 0 and frag in msg, (what, rc, msg)
    print("\ncarried by the additive term:", sorted(carried))
    signs = {c for c in carried if c[1] == "hfen map l1"}
    assert len(signs) == len(SHAPES) + len(HFEN_TAPS) and carried - signs == CARRIED, sorted((carried - signs) ^ CARRIED)
    assert case_bytes() == 4 * 3 * 4 * 139 * 139              # 927 408 bytes per operand (planes-N3C4-139x139), 232 k pixels
