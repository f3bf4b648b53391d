"""Edge-shape parity of the HBM-bound and reduction kernels (csrc/elementwise.hip, csrc/norm_loss_optim.hip and the
pad / window / tanh / GAN-loss / column-sum part of csrc/gconv.hip) against the plain PyTorch-CPU statement of each op in
FLOAT64 (autograd for the backwards).  test_gpu_kernels.py checks each of these kernels at one small shape; here every family
runs over the shape classes at which such kernels go wrong (the class is part of the test id):

  tiny    1 pixel, n = 1 / 255 / 256 / 257 for the flat ops
  window  every view at a non-zero channel offset of a wider buffer, source / destination / mask with three different
          widths, the channels outside the view pre-filled with a sentinel that must survive
  oddC    C = 12, 48, 96 (and 4): the non-power-of-two lane split of the reductions, the generic body of the BN backward
  wrap    more work items than one pass of the capped grid (2048 blocks x 256 threads; 4096 blocks per image for the
          InstanceNorm apply launches), the count no multiple of the grid: the second grid-stride iteration.  The launches
          of gconv.hip (pad2d, unpad2d, window2d, tanh) cap at 65535 blocks: a second iteration of theirs needs more than
          16 776 960 items.  The two tanh kernels get it (test_tanh_wrap_65535_blocks, 64 MB per buffer); for the three
          float4 kernels it would take 268 MB per buffer and is not run -- their `big_onepass` cases are one pass.
  cap     the reductions at their block cap, with nblocks < want (C = 512 over 18 433 pixels: want 512, 37 pixels per block,
          499 blocks), L1 / sumsq at 600 001 elements, the relativistic loss around RAGAN_MULTI_MIN = 4096 and at
          256 * 4096 + 4097 logits
  ties    2x2 max-pool windows with two equal positive maxima, planted on purpose

Bounds.  Pure movement, and the ops whose fp32 result is ONE correctly rounded operation on fp32 inputs (a gate multiply, a
sum of two values: the fp64 result rounded to fp32 is then the fp32 result), compare with torch.equal.  Elementwise fp32
arithmetic and losses: 1e-6 x (max|ref| + 1); BN forward, linear, sums of products: 2e-5 likewise; the bilinear and bias_grad
bounds are those of test_gpu_kernels.py (2e-6 / 5e-6, 2e-6).  BN backward, the shifted-input BN case and Adam have no derived
bound: their error against fp64 is held to 2 x the error of the fp32 PyTorch-CPU op on the same inputs + 2e-7 of the output
scale (`yardstick`; the factor allows another, equally valid summation order, the additive term one output rounding).

No comparison skips an element: every gate is either taken from exact inputs (the masks are fp32 test data, `> 0` is the same
predicate on both sides) or, for the BN / InstanceNorm / linear backwards, from the DEVICE's own forward output after that
output has been checked against fp64.  test_inputs_and_references (no device) builds every case's inputs and reference and
checks the share of gate operands within 1e-5 of zero (<= 0.1 %), the planted pool ties and that every yardstick is non-zero.

The module has no module-level `pytestmark`: it holds that one device-free test, so every other test carries the gpu mark
itself.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K

gpu = pytest.mark.gpu
DEV = K.DEV
SENT = -123.0                                                   # the sentinel outside every view
S32 = float(torch.tensor(0.2, dtype=torch.float32))             # the LeakyReLU slope the kernels multiply by: fp32(0.2)
D = torch.double
FLAT_N = [1, 255, 256, 257, 600001]
FLAT_IDS = ["tiny1", "tiny255", "tiny256", "tiny257", "wrap600001"]
cache = functools.lru_cache(maxsize=None)


def _ops():
    return K._ops()


def hi_pad(lo, C):
    return 4 + (-(lo + C)) % 4


_KEPT = {}


def win(x, lo, keep=False):
    """NCHW cpu tensor -> View of a device buffer that holds it at channel offset `lo`; SENT in the other channels.
    keep: the buffer of a large read-only input is built once and shared between the tests that read it (each of them checks
    that it holds the same bits after its launches)."""
    C = x.shape[1]
    hit = _KEPT.get((id(x), lo)) if keep else None
    if hit is not None:
        return _ops().View(hit[1], lo, C)
    buf = K.nhwc_buf(x.float(), lo + C + hi_pad(lo, C), lo, fill=SENT)
    if keep:
        _KEPT[(id(x), lo)] = (x, buf)
    return _ops().View(buf, lo, C)


def blank(N, H, W, C, lo, inner=SENT):
    buf = torch.full((N, H, W, lo + C + hi_pad(lo, C)), SENT, device=DEV)
    if inner != SENT:
        buf[..., lo:lo + C] = inner
    return _ops().View(buf, lo, C)


def got(v):
    """the view as an NCHW tensor, still on the device: the comparisons run there (the references are uploaded)"""
    return v.buf[..., v.coff:v.coff + v.C].permute(0, 3, 1, 2)


def close(a, ref, tol=2e-5, what=""):
    K.close(a, ref.to(a.device), tol=tol, what=what)


def eq(a, ref):
    return torch.equal(a, ref.to(a.device))


def outside_untouched(*views):
    for v in views:
        assert bool((v.buf[..., :v.coff] == SENT).all()) and bool((v.buf[..., v.coff + v.C:] == SENT).all()), "wrote outside the view"


def same_after(fn, *views):
    """run fn; the buffers of `views` (sources) hold the same bits afterwards"""
    snaps = [v.buf.clone() for v in views]
    fn()
    for v, s in zip(views, snaps):
        assert torch.equal(v.buf, s), "a source buffer changed"


def gate(m):
    """LeakyReLU'(m) in fp64 with the kernels' fp32 slope"""
    return torch.where(m > 0, torch.ones_like(m, dtype=D), torch.full_like(m, S32, dtype=D))


def near_zero_share(t, eps=1e-5):
    return float((t.abs() < eps).double().mean())


def yardstick(what, got_, ref64, ref32):
    """err(device) <= 2 x err(fp32 PyTorch-CPU op) + 2e-7 x scale, both against the fp64 reference; prints the figures"""
    scale = float(ref64.abs().max())
    e_dev = float((got_.double() - ref64.to(got_.device)).abs().max())
    e_32 = float((ref32.double() - ref64).abs().max())
    bound = 2.0 * e_32 + 2e-7 * scale
    print("YARDSTICK %-44s dev %.3e  torch-fp32 %.3e  scale %.3e  dev/bound %.3f" % (what, e_dev, e_32, scale, e_dev / bound if bound else float("inf")))
    # worst device / bound measured on an MI355X: 0.45 (bn bwd dgamma, shifted case), 0.37 (Adam), 0.31 (bn bwd gz); DESIGN.md 19
    assert e_dev <= bound, (what, e_dev, e_32, scale)
    return e_dev, e_32


# =====================================================================================================================
# 1. layout and movement (exact)
# =====================================================================================================================
LAYOUT_SHAPES = {"tiny1px": (1, 1, 1), "odd": (2, 5, 7), "wrap": (2, 513, 512)}
N2H = {"C3pad4": (3, 4), "C3pad8": (3, 8), "C5pad8": (5, 8)}


@cache
def n2h_case(C, shape):
    N, H, W = LAYOUT_SHAPES[shape]
    return K.rnd(N, C, H, W, seed=700 + C), K.rnd(C, seed=701, lo=0.5, hi=2.0), K.rnd(C, seed=702)


@gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("shape", list(LAYOUT_SHAPES))
@pytest.mark.parametrize("cc", list(N2H))
def test_nchw_to_nhwc_window(cc, shape, scaled):
    ops = _ops()
    C, Cpad = N2H[cc]
    x, sc, sh = n2h_case(C, shape)
    N, _, H, W = x.shape
    v = blank(N, H, W, Cpad, 8)
    ops.nchw_to_nhwc(x.to(DEV), v, Cpad=Cpad, scale=sc.to(DEV) if scaled else None, shift=sh.to(DEV) if scaled else None)
    out = got(v)
    if scaled:
        close(out[:, :C], x.double() * sc.double().view(1, C, 1, 1) + sh.double().view(1, C, 1, 1), tol=1e-6, what="nchw->nhwc")
    else:
        assert eq(out[:, :C], x)
    assert bool((out[:, C:] == 0).all())                      # the pad channels are zero
    outside_untouched(v)


H2N_SHAPES = {"tiny1px": (1, 3, 1, 1), "oddC5": (2, 5, 5, 7), "wrap": (2, 3, 300, 301)}


@cache
def h2n_case(shape):
    N, C, H, W = H2N_SHAPES[shape]
    return K.rnd(N, C, H, W, seed=710), K.rnd(C, seed=711, lo=0.5, hi=2.0), K.rnd(N, C, H, W, seed=712)


@gpu
@pytest.mark.parametrize("acc", [False, True], ids=["store", "acc"])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scaled"])
@pytest.mark.parametrize("shape", list(H2N_SHAPES))
def test_nhwc_to_nchw_window(shape, scaled, acc):
    ops = _ops()
    x, sc, d0 = h2n_case(shape)
    C = x.shape[1]
    src = win(x, 4)
    dst = d0.to(DEV) if acc else torch.full(x.shape, float("nan"), device=DEV)      # without accumulate dst is not read
    same_after(lambda: ops.nhwc_to_nchw(src, dst, scale=sc.to(DEV) if scaled else None, accumulate=acc), src)
    ref = x.double() * (sc.double().view(1, C, 1, 1) if scaled else 1.0) + (d0.double() if acc else 0.0)
    if scaled:
        close(dst, ref, tol=1e-6, what="nhwc->nchw")
    else:
        assert eq(dst, ref.float())            # a copy, or one correctly rounded addition


D2S_SHAPES = {"tiny1px": (1, 1, 1, 1), "oddC3": (2, 5, 7, 3), "wrap": (2, 64, 65, 64)}      # N, H, W, Cout


@cache
def d2s_case(shape):
    N, H, W, Co = D2S_SHAPES[shape]
    return K.rnd(N, 4 * Co, H, W, seed=720), K.rnd(N, Co, 2 * H, 2 * W, seed=721), K.rnd(N, Co, 2 * H, 2 * W, seed=722)


@gpu
@pytest.mark.parametrize("shape", list(D2S_SHAPES))
def test_depth_to_space_window(shape):
    ops = _ops()
    N, H, W, Co = D2S_SHAPES[shape]
    x = d2s_case(shape)[0]
    xv, yv = win(x, 4), blank(N, 2 * H, 2 * W, Co, 8)
    same_after(lambda: ops.depth_to_space(xv, yv), xv)
    assert eq(got(yv), F.pixel_shuffle(x, 2))
    outside_untouched(yv)


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", list(D2S_SHAPES))
def test_space_to_depth_bwd_window(shape, masked):
    ops = _ops()
    N, H, W, Co = D2S_SHAPES[shape]
    _, gy, m = d2s_case(shape)
    gv, xv, mv = win(gy, 4), blank(N, H, W, 4 * Co, 8), win(m, 12)
    same_after(lambda: ops.space_to_depth_bwd(gv, xv, mask=mv if masked else None, mslope=0.2), gv, mv)
    ref = F.pixel_unshuffle(gy.double() * (gate(m) if masked else 1.0), 2).float()
    assert eq(got(xv), ref)
    outside_untouched(xv)


POOL_SHAPES = {"tiny": (1, 2, 2, 4), "oddC12": (2, 6, 10, 12), "wrap": (2, 192, 194, 128)}      # N, H, W, C of the pool input


@cache
def pool_case(shape):
    """post-ReLU pool input with PLANTED TIES: in a quarter of the 2x2 windows two of the four elements (a pair drawn per window)
    hold the same value, larger than the other two -- the first of them in scan order takes the gradient (aten)."""
    N, H, W, C = POOL_SHAPES[shape]
    x = F.relu(K.rnd(N, C, H, W, seed=730))
    w = x.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4).clone()
    sel = K.rnd(N, C, H // 2, W // 2, seed=731) < -0.5                                        # a quarter of the windows
    pair = ((K.rnd(N, C, H // 2, W // 2, seed=732) + 1.0) * 3.0).long().clamp(0, 5)           # which of the 6 pairs
    pairs = torch.tensor([[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]])
    top = w.max(dim=-1).values + 0.5
    for j in range(2):
        idx = pairs[pair][..., j:j + 1]
        w.scatter_(-1, idx, torch.where(sel, top, w.gather(-1, idx).squeeze(-1)).unsqueeze(-1))
    xt = w.view(N, C, H // 2, W // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H, W).contiguous()
    gp = K.rnd(N, C, H // 2, W // 2, seed=733)
    pre = xt.double().requires_grad_(True)
    pooled = F.max_pool2d(F.relu(pre), 2, 2)
    (gref,) = torch.autograd.grad(pooled, pre, gp.double())
    return xt, gp, pooled.detach().float(), gref.float(), sel


def tie_share(xt):
    N, C, H, W = xt.shape
    w = xt.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    s = w.sort(dim=-1, descending=True).values
    return (s[..., 0] == s[..., 1]) & (s[..., 0] > 0)


@gpu
@pytest.mark.parametrize("shape", list(POOL_SHAPES))
def test_maxpool2_fwd_bwd_ties(shape):
    ops = _ops()
    N, H, W, C = POOL_SHAPES[shape]
    xt, gp, pooled, gref, _ = pool_case(shape)
    xv, pv = win(xt, 4), blank(N, H // 2, W // 2, C, 8)
    same_after(lambda: ops.maxpool2_fwd(xv, pv), xv)
    assert eq(got(pv), pooled)
    gv, gxv = win(gp, 12), blank(N, H, W, C, 8)
    same_after(lambda: ops.maxpool2_bwd(gv, xv, gxv), gv, xv)
    assert eq(got(gxv), gref), "max-pool backward: the FIRST maximum of a window in scan order takes the gradient"
    outside_untouched(pv, gxv)


@gpu
@pytest.mark.parametrize("hw", [(5, 4), (4, 5)], ids=["oddH", "oddW"])
def test_maxpool2_rejects_odd_sizes(hw):
    """forward and backward reject an odd H or W alike (the backward would leave the last row / column of gx unwritten); the
    call returns its error before any launch: the destination keeps its sentinel."""
    from trainner_amd import hip
    ops = _ops()
    H, W = hw
    xv, pv, gxv = win(K.rnd(1, 4, H, W, seed=734), 4), blank(1, H // 2, W // 2, 4, 8), blank(1, H, W, 4, 8)
    with pytest.raises(hip.HipEngineError, match="maxpool2_fwd"):
        ops.maxpool2_fwd(xv, pv)
    with pytest.raises(hip.HipEngineError, match="maxpool2_bwd"):
        ops.maxpool2_bwd(pv, xv, gxv)
    torch.cuda.synchronize()
    assert bool((pv.buf == SENT).all()) and bool((gxv.buf == SENT).all())


PAD_SHAPES = {"min": None, "oddC12": (2, 9, 11, 12), "big_onepass": (2, 96, 97, 128)}      # (65535-block grids: one pass)


@cache
def pad_case(shape, pad):
    N, H, W, C = PAD_SHAPES[shape] or (1, pad + 1, pad + 1, 4)          # min: H = W = pad + 1, the smallest a reflection takes
    x = K.rnd(N, C, H, W, seed=740 + pad)
    gp = K.rnd(N, C, H + 2 * pad, W + 2 * pad, seed=745 + pad)
    xr = x.double().requires_grad_(True)
    (fold,) = torch.autograd.grad(F.pad(xr, (pad,) * 4, mode="reflect"), xr, gp.double())
    return x, gp, fold


@gpu
@pytest.mark.parametrize("pad", [1, 2, 3])
@pytest.mark.parametrize("shape", list(PAD_SHAPES))
def test_pad2d_unpad2d_crop_window(shape, pad):
    ops = _ops()
    x = pad_case(shape, pad)[0]
    N, C, H, W = x.shape
    xv = win(x, 4)
    for refl in (True, False):
        yv = blank(N, H + 2 * pad, W + 2 * pad, C, 8)
        same_after(lambda: ops.pad2d(xv, yv, pad, refl), xv)
        assert eq(got(yv), F.pad(x, (pad,) * 4, mode="reflect") if refl else F.pad(x, (pad,) * 4))
        back = blank(N, H, W, C, 12)
        same_after(lambda: ops.unpad2d(yv, back, pad, False), yv)
        assert eq(got(back), x)
        outside_untouched(yv, back)


@gpu
@pytest.mark.parametrize("pad", [1, 3])
@pytest.mark.parametrize("shape", list(PAD_SHAPES))
def test_unpad2d_fold_window(shape, pad):
    """the adjoint of the reflection padding at pad 1 and 3 (the ResNet blocks and the 7x7 layers), down to H = W = pad + 1 where
    every interior row folds from both sides"""
    ops = _ops()
    x, gp, fold = pad_case(shape, pad)
    N, C, H, W = x.shape
    gv, fv = win(gp, 4), blank(N, H, W, C, 8)
    same_after(lambda: ops.unpad2d(gv, fv, pad, True), gv)
    close(got(fv), fold, tol=1e-6, what="reflection fold")
    outside_untouched(fv)


WINDOW_CASES = {            # N, C, Hs, Ws, Hd, Wd, oy, ox
    "neg_pos": (2, 12, 5, 7, 6, 9, -1, 2), "pos_neg": (2, 12, 5, 7, 6, 9, 2, -1), "neg_neg": (2, 12, 5, 7, 6, 9, -2, -3),
    "pos_pos": (2, 12, 5, 7, 4, 5, 1, 1), "beyond": (1, 4, 5, 7, 6, 9, 6, -10), "tiny1px": (1, 4, 1, 1, 1, 1, 0, 0),
    "big_onepass": (2, 128, 96, 97, 97, 98, -1, 1)}


@cache
def window_case(name):
    N, C, Hs, Ws, Hd, Wd, oy, ox = WINDOW_CASES[name]
    src, d0 = K.rnd(N, C, Hs, Ws, seed=750), K.rnd(N, C, Hd, Wd, seed=751)
    ys, xs = torch.arange(Hd) + oy, torch.arange(Wd) + ox
    ok = ((ys >= 0) & (ys < Hs)).view(Hd, 1) & ((xs >= 0) & (xs < Ws)).view(1, Wd)
    exp = src.double()[:, :, ys.clamp(0, Hs - 1)][:, :, :, xs.clamp(0, Ws - 1)] * ok.double()
    return src, d0, exp


@gpu
@pytest.mark.parametrize("acc", [False, True], ids=["store", "acc"])
@pytest.mark.parametrize("name", list(WINDOW_CASES))
def test_window2d_window(name, acc):
    ops = _ops()
    N, C, Hs, Ws, Hd, Wd, oy, ox = WINDOW_CASES[name]
    src, d0, exp = window_case(name)
    sv = win(src, 4)
    dv = win(d0, 8) if acc else blank(N, Hd, Wd, C, 8, inner=float("nan"))        # without acc dst is not read
    same_after(lambda: ops.window2d(sv, dv, oy, ox, acc=acc), sv)
    assert eq(got(dv), (exp + d0.double()).float() if acc else exp.float())
    outside_untouched(dv)


PIX_SHAPES = {"tiny1px": (1, 1, 1, 4), "oddC12": (2, 5, 7, 12), "oddC48": (1, 3, 5, 48), "wrap": (2, 96, 97, 128)}      # N, H, W, C


@cache
def pix_case(shape):
    N, H, W, C = PIX_SHAPES[shape]
    return tuple(K.rnd(N, C, H, W, seed=760 + i) for i in range(3))


@gpu
@pytest.mark.parametrize("shape", list(PIX_SHAPES))
def test_add2_mask_copy_mask_mul_window(shape):
    ops = _ops()
    N, H, W, C = PIX_SHAPES[shape]
    a, b, m = pix_case(shape)
    av, bv, mv, dv = win(a, 4), win(b, 8), win(m, 12), blank(N, H, W, C, 16)
    same_after(lambda: ops.add2(dv, av, bv), av, bv)
    assert eq(got(dv), (a.double() + b.double()).float())
    same_after(lambda: ops.mask_copy(dv, av, mv, 0.2), av, mv)
    assert eq(got(dv), (a.double() * gate(m)).float())
    same_after(lambda: ops.mask_mul(bv, mv, 0.2), mv, av)
    assert eq(got(bv), (b.double() * gate(m)).float())
    outside_untouched(dv, bv)


@gpu
@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_fill_flat(n):
    ops = _ops()
    buf = torch.full((n + 8,), SENT, device=DEV)
    ops.fill(buf[4:4 + n], 2.5)
    assert bool((buf[4:4 + n] == 2.5).all()) and bool((buf[:4] == SENT).all()) and bool((buf[4 + n:] == SENT).all())


IM2COL_CASES = {      # N, H, W, C, k, stride, pad
    "k3s1p0": (2, 7, 9, 12, 3, 1, 0), "k3s1p1": (2, 7, 9, 12, 3, 1, 1), "k3s2p1": (2, 7, 9, 12, 3, 2, 1), "k3s2p2": (2, 7, 9, 12, 3, 2, 2),
    "k4s1p1": (2, 7, 9, 12, 4, 1, 1), "k4s2p1": (2, 7, 9, 12, 4, 2, 1), "k4s1p2": (2, 7, 9, 12, 4, 1, 2), "k4s2p0_tiny": (1, 4, 4, 4, 4, 2, 0),
    "k3s1p1_wrap": (1, 172, 171, 8, 3, 1, 1)}


@cache
def im2col_case(name):
    N, H, W, C, k, s, p = IM2COL_CASES[name]
    x = K.rnd(N, C, H, W, seed=770)
    u = F.unfold(x, k, padding=p, stride=s)                                    # [N, C k k, L], channel-major
    ref = u.view(N, C, k * k, -1).permute(0, 3, 2, 1).reshape(-1, k * k * C).contiguous()     # [pixel][(ky k + kx) C + c]
    return x, ref


@gpu
@pytest.mark.parametrize("name", list(IM2COL_CASES))
def test_im2col_window(name):
    from trainner_amd import hip
    N, H, W, C, k, s, p = IM2COL_CASES[name]
    x, ref = im2col_case(name)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xv = win(x, 8)
    out = torch.full((ref.numel() + 8,), SENT, device=DEV)
    same_after(lambda: hip.check(hip.load().tnr_im2col(xv.c(), N, H, W, C, k, s, p, Ho, Wo, out[4:].data_ptr(), hip.stream()), "im2col"), xv)
    assert torch.equal(out[4:4 + ref.numel()].cpu().view(ref.shape), ref)
    assert bool((out[:4] == SENT).all()) and bool((out[4 + ref.numel():] == SENT).all())


# =====================================================================================================================
# 2. elementwise arithmetic
# =====================================================================================================================
UP_SHAPES = {"tiny1px": (1, 1, 1, 4), "oddC12": (2, 5, 7, 12), "wrap": (2, 96, 97, 128)}       # N, H, W, C of the low-resolution side


@cache
def up_case(shape):
    N, H, W, C = UP_SHAPES[shape]
    gup, m = K.rnd(N, C, 2 * H, 2 * W, seed=800), K.rnd(N, C, H, W, seed=801)
    s = F.avg_pool2d(gup.double(), 2) * 4
    x = K.rnd(N, C, H, W, seed=802)
    xr = x.double().requires_grad_(True)
    (badj,) = torch.autograd.grad(F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False), xr, gup.double())
    return gup, m, s, x, badj


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", list(UP_SHAPES))
def test_upsample2x_bwd_window(shape, masked):
    ops = _ops()
    N, H, W, C = UP_SHAPES[shape]
    gup, m, s, _, _ = up_case(shape)
    gv, xv, mv = win(gup, 4), blank(N, H, W, C, 8), win(m, 12)
    same_after(lambda: ops.upsample2x_bwd(gv, xv, mask=mv if masked else None, mslope=0.2), gv, mv)
    close(got(xv), s * gate(m) if masked else s, tol=1e-6, what="upsample2x bwd")
    outside_untouched(xv)


@gpu
@pytest.mark.parametrize("shape", ["oddC12", "wrap"])
def test_bilinear2x_oddC_wrap(shape):
    """the tiny shapes are in test_gpu_kernels.py; here C = 12 and the second grid-stride iteration of both kernels (the forward
    at half the size: it has four work items per input pixel)"""
    ops = _ops()
    N, H, W, C = UP_SHAPES[shape]
    gup, m, _, x, badj = up_case(shape)
    xs = x[:, :, :H // 2 + 1, :W // 2 + 1].contiguous() if shape == "wrap" else x
    xv, yv = win(xs, 4), blank(N, 2 * xs.shape[2], 2 * xs.shape[3], C, 8)
    same_after(lambda: ops.bilinear2x_fwd(xv, yv), xv)
    close(got(yv), F.interpolate(xs.double(), scale_factor=2, mode="bilinear", align_corners=False), tol=2e-6, what="bilinear fwd")
    gv, gxv, gzv, mv = win(gup, 4), blank(N, H, W, C, 8), blank(N, H, W, C, 12), win(m, 16)
    same_after(lambda: ops.bilinear2x_bwd(gv, gx=gxv, gz=gzv, mask=mv, mslope=0.2), gv, mv)
    close(got(gxv), badj, tol=5e-6, what="bilinear bwd")
    close(got(gzv), badj * gate(m), tol=5e-6, what="bilinear bwd gated")
    outside_untouched(yv, gxv, gzv)


@gpu
@pytest.mark.parametrize("ab", [(0.75, 0.0), (0.75, -0.5), (0.0, 1.25)], ids=["b0_dst_not_read", "ab", "a0"])
@pytest.mark.parametrize("shape", list(PIX_SHAPES))
def test_axpby_window(shape, ab):
    ops = _ops()
    N, H, W, C = PIX_SHAPES[shape]
    a, b = ab
    s, d0, _ = pix_case(shape)
    sv = win(s, 4)
    dv = win(d0, 8) if b != 0.0 else blank(N, H, W, C, 8, inner=float("nan"))       # b = 0: dst is not read (NaN would spread)
    same_after(lambda: ops.axpby(dv, sv, a=a, b=b), sv)
    close(got(dv), a * s.double() + (b * d0.double() if b != 0.0 else 0.0), tol=1e-6, what="axpby")
    outside_untouched(dv)


@cache
def flat_case(n):
    a, b, g0 = K.rnd(n, seed=810, lo=-3, hi=3), K.rnd(n, seed=811, lo=-3, hi=3), K.rnd(n, seed=812)
    return a, b, g0


@gpu
@pytest.mark.parametrize("n", FLAT_N, ids=FLAT_IDS)
def test_tanh_scale_l1bwd_clip_flat(n):
    """n = 600 001 is the second grid-stride pass of scale_by, l1_mean_bwd, sumsq and clip_by_norm (2048-block grids); the tanh
    kernels run it in one pass, their second pass is test_tanh_wrap_65535_blocks"""
    ops = _ops()
    a, b, g0 = flat_case(n)
    ad, bd, gd = a.to(DEV), b.to(DEV), g0.to(DEV)
    guard = torch.full((n + 8,), SENT, device=DEV)
    y = guard[4:4 + n]
    ops.tanh_fwd(ad, y)
    close(y.cpu(), torch.tanh(a.double()), tol=1e-6, what="tanh")
    gx = torch.empty_like(ad)
    ops.tanh_bwd(gd, y, gx)
    close(gx.cpu(), g0.double() * (1 - y.cpu().double() ** 2), tol=1e-6, what="tanh bwd")
    k = torch.tensor([0.7], device=DEV)
    ops.scale_by(y, ad, k)
    assert torch.equal(y.cpu(), (a.double() * float(k)).float())                    # one correctly rounded product
    assert bool((guard[:4] == SENT).all()) and bool((guard[4 + n:] == SENT).all())
    # L1 backward: sign(a - b) * scale * gscale / n, stored and accumulated (scale = n / 2 keeps the values of order one)
    kk = 0.5 * n * 0.7 / n
    ref = torch.sign(a.double() - b.double()) * kk
    ga = torch.full((n,), float("nan"), device=DEV)
    ops.l1_mean_bwd(ad, bd, 0.5 * n, k, ga)
    close(ga.cpu(), ref, tol=1e-6, what="l1 bwd")
    ga2 = gd.clone()
    ops.l1_mean_bwd(ad, bd, 0.5 * n, k, ga2, accumulate=True)
    close(ga2.cpu(), ref + g0.double(), tol=1e-6, what="l1 bwd accumulate")
    ga3 = gd.clone()
    ops.l1_mean_bwd(ad, bd, 0.5 * n, None, ga3, accumulate=True)
    close(ga3.cpu(), ref / 0.7 + g0.double(), tol=1e-6, what="l1 bwd accumulate, no gscale")
    # clip_by_norm on both sides of coef = 1
    ss = torch.zeros(1, dtype=D, device=DEV)
    ops.sumsq(gd, ss)
    norm = math.sqrt(float((g0.double() ** 2).sum()))
    loose = gd.clone()
    ops.clip_by_norm(loose, ss, 2.0 * norm + 1.0)
    assert torch.equal(loose, gd)                                                    # coef clamps to 1: unchanged
    tight = gd.clone()
    ops.clip_by_norm(tight, ss, 0.25 * norm)
    close(tight.cpu(), g0.double() * (0.25 * norm / (norm + 1e-6)), tol=1e-6, what="clip")


TANH_WRAP_N = 65535 * 256 + 257          # one pass of the 65535-block grid, one more block and one element


@cache
def tanh_wrap_case():
    x = K.rnd(TANH_WRAP_N, seed=820, lo=-3, hi=3)
    y = torch.tanh(x.double())
    return x, y, x.double() * (1 - y ** 2)


@gpu
def test_tanh_wrap_65535_blocks():
    """the second grid-stride iteration of tanh_fwd / tanh_bwd (the gradient fed is x itself)"""
    ops = _ops()
    x, y64, gx64 = tanh_wrap_case()
    xd = x.to(DEV)
    guard = torch.full((TANH_WRAP_N + 8,), SENT, device=DEV)
    y = guard[4:4 + TANH_WRAP_N]
    ops.tanh_fwd(xd, y)
    close(y, y64, tol=1e-6, what="tanh, second pass")
    gx = torch.full((TANH_WRAP_N + 8,), SENT, device=DEV)
    ops.tanh_bwd(xd, y, gx[4:4 + TANH_WRAP_N])
    close(gx[4:4 + TANH_WRAP_N], gx64, tol=1e-6, what="tanh bwd, second pass")
    for b in (guard, gx):
        assert bool((b[:4] == SENT).all()) and bool((b[4 + TANH_WRAP_N:] == SENT).all())


# =====================================================================================================================
# 3. BatchNorm / InstanceNorm
# =====================================================================================================================
BN_CASES = {      # N, H, W, C
    "tiny3px_oddC4": (1, 1, 3, 4), "oddC4": (2, 5, 7, 4), "oddC12": (2, 9, 11, 12), "oddC48": (2, 9, 11, 48), "oddC96": (1, 9, 11, 96),
    "pow2C64": (2, 9, 11, 64), "wrap_oddC48_generic_body": (2, 150, 151, 48), "cap_C512_nblocks499": (1, 1, 18433, 512),
    "cap_wrap_C16": (2, 513, 512, 16), "shifted_oddC48": (2, 33, 17, 48)}
EPS = 1e-5


@cache
def bn_inputs(name):
    N, H, W, C = BN_CASES[name]
    if name.startswith("shifted"):       # per-channel mean about 3, standard deviation about 0.05
        z = K.rnd(N, C, H, W, seed=900) * (0.05 * math.sqrt(3.0)) + (3.0 + 0.2 * K.rnd(1, C, 1, 1, seed=901))
    else:                                # standard deviation about 1.7; |mean| 0.5 .. 0.8 of either sign, so that "relative" has a
        r = K.rnd(1, C, 1, 1, seed=901)    # meaning for the mean of every channel (the device-free test checks |mean| >= std / 100)
        z = K.rnd(N, C, H, W, seed=900) * 3.0 + torch.sign(r) * (0.5 + 0.3 * r.abs())
    gamma, beta = K.rnd(C, seed=902, lo=0.5, hi=1.5), K.rnd(C, seed=903)
    gy = K.rnd(N, C, H, W, seed=904)
    rm0, rv0 = K.rnd(C, seed=905), K.rnd(C, seed=906, lo=0.5, hi=1.5)
    zd = z.double()
    n = N * H * W
    mean = zd.mean(dim=(0, 2, 3))
    var = ((zd - mean.view(1, C, 1, 1)) ** 2).mean(dim=(0, 2, 3))
    return dict(z=z, gamma=gamma, beta=beta, gy=gy, rm0=rm0, rv0=rv0, mean=mean, var=var, unbiased=var * n / (n - 1), n=n)


def bn_pre(i, dtype, inst=False):
    z = i["z"].detach().to(dtype).requires_grad_(True)
    if inst:
        return z, None, None, F.instance_norm(z, eps=EPS)
    ga, be = i["gamma"].detach().to(dtype).requires_grad_(True), i["beta"].detach().to(dtype).requires_grad_(True)
    return z, ga, be, F.batch_norm(z, None, None, ga, be, True, 0.1, EPS)


@cache
def bn_forward_ref(name, inst=False):
    """pre-activation output of the norm in fp64 and in fp32 (the yardstick)"""
    i = in_inputs(name) if inst else bn_inputs(name)
    return bn_pre(i, D, inst)[3].detach(), bn_pre(i, torch.float32, inst)[3].detach() if name.startswith("shifted") else None


_BWD = {}


def bn_backward_ref(name, gatef, inst=False):
    """gradients of sum(gy * pre * gatef) in fp64 and fp32: the backward of act(norm(z)) with the activation's gate GIVEN
    (taken from the device's forward output, so no rounding of a pre-activation near zero can flip it)"""
    hit = _BWD.get((name, inst))
    if hit is not None and torch.equal(hit[0], gatef):
        return hit[1]
    i = in_inputs(name) if inst else bn_inputs(name)
    out = []
    for dtype in (D,) if inst else (D, torch.float32):
        z, ga, be, pre = bn_pre(i, dtype, inst)
        out.append(tuple(g.detach() for g in torch.autograd.grad(pre, (z,) if inst else (z, ga, be), (i["gy"].double() * gatef).to(dtype))))
    _BWD[(name, inst)] = (gatef, out)
    return out


@gpu
@pytest.mark.parametrize("name", list(BN_CASES))
def test_batchnorm_window(name):
    ops = _ops()
    N, H, W, C = BN_CASES[name]
    i = bn_inputs(name)
    shifted = name.startswith("shifted")
    pre64, pre32 = bn_forward_ref(name)
    zv, yv = win(i["z"], 4, keep=True), blank(N, H, W, C, 8)
    gd, bd = i["gamma"].to(DEV), i["beta"].to(DEV)
    rm, rv, nbt = i["rm0"].to(DEV), i["rv0"].to(DEV), torch.full((), 5, dtype=torch.int64, device=DEV)
    sm, si, st = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV), torch.zeros(2 * C, dtype=D, device=DEV)
    same_after(lambda: ops.bn_train_fwd(zv, yv, gd, bd, rm, rv, nbt, sm, si, stat64=st), zv)
    yd = got(yv)
    if shifted:
        yardstick("bn fwd y %s" % name, yd, F.leaky_relu(pre64, S32), F.leaky_relu(pre32, S32))
    else:
        close(yd, F.leaky_relu(pre64, S32), tol=2e-5, what="bn fwd")
    close(rm.cpu(), 0.9 * i["rm0"].double() + 0.1 * i["mean"], tol=1e-5, what="running mean")
    close(rv.cpu(), 0.9 * i["rv0"].double() + 0.1 * i["unbiased"], tol=1e-5, what="running var")
    assert int(nbt) == 6
    # stat64: the fp64 batch statistics, mean and unbiased variance of every channel to 1e-12 relative, the shifted case
    # (mean 3, std 0.05) included: the sums are taken about a pivot pixel, not about zero
    merr = ((st[:C].cpu() - i["mean"]).abs() / i["mean"].abs())
    verr = ((st[C:].cpu() - i["unbiased"]).abs() / i["unbiased"])
    print("STAT64 %-30s max rel err: mean %.3e  var %.3e" % (name, float(merr.max()), float(verr.max())))
    assert bool((merr <= 1e-12).all()), "stat64 mean"
    assert bool((verr <= 1e-12).all()), "stat64 unbiased variance"
    close(sm.cpu(), i["mean"], tol=1e-6, what="save_mean")
    close(si.cpu(), 1.0 / (i["var"] + EPS).sqrt(), tol=1e-6, what="save_invstd")
    outside_untouched(yv)
    # one replay moves the running statistics and the batch counter exactly as a second forward over the same input does
    rm2, rv2, nbt2 = rm.clone(), rv.clone(), nbt.clone()
    y2 = blank(N, H, W, C, 8)
    ops.bn_train_fwd(zv, y2, gd, bd, rm2, rv2, nbt2, torch.zeros(C, device=DEV), torch.zeros(C, device=DEV))
    ops.bn_replay_running(rm, rv, nbt, st)
    assert torch.equal(rm, rm2) and torch.equal(rv, rv2) and torch.equal(nbt, nbt2) and int(nbt) == 7
    assert torch.equal(y2.buf, yv.buf)
    # backward, gate from the device's y
    gatef = gate(yd.cpu())
    (gz64, gg64, gb64), (gz32, gg32, gb32) = bn_backward_ref(name, gatef)
    gyv, gzv = win(i["gy"], 12, keep=True), blank(N, H, W, C, 16)
    dg, db = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)     # acc_beta = 0: not read
    same_after(lambda: ops.bn_train_bwd(gyv, yv, zv, gzv, gd, sm, si, dgamma=dg, dbeta=db, acc_beta=0.0), gyv, yv, zv)
    yardstick("bn bwd gz %s" % name, got(gzv), gz64, gz32)
    yardstick("bn bwd dgamma %s" % name, dg, gg64, gg32)
    yardstick("bn bwd dbeta %s" % name, db, gb64, gb32)
    outside_untouched(gzv)
    # the gate recomputed from z (beta given) is bit-identical to the gate read from y
    assert ops.BN_MASK_FROM_Z
    gzv2 = blank(N, H, W, C, 16)
    dg2, db2 = torch.full((C,), float("nan"), device=DEV), torch.full((C,), float("nan"), device=DEV)
    same_after(lambda: ops.bn_train_bwd(gyv, None, zv, gzv2, gd, sm, si, dgamma=dg2, dbeta=db2, acc_beta=0.0, beta=bd), gyv, zv)
    assert torch.equal(gzv2.buf, gzv.buf) and torch.equal(dg2, dg) and torch.equal(db2, db)
    # accumulation into existing parameter gradients
    dg3, db3 = torch.full((C,), 2.0, device=DEV), torch.full((C,), -4.0, device=DEV)
    ops.bn_train_bwd(gyv, yv, zv, gzv2, gd, sm, si, dgamma=dg3, dbeta=db3, acc_beta=0.5)
    close(dg3.cpu(), 1.0 + dg.cpu().double(), tol=1e-6, what="dgamma accumulate")
    close(db3.cpu(), -2.0 + db.cpu().double(), tol=1e-6, what="dbeta accumulate")


IN_CASES = {      # N, H, W, C
    "tiny2px_N3": (3, 1, 2, 4), "N3_oddC12": (3, 17, 23, 12), "N3_oddC48": (3, 9, 11, 48), "N3_pow2C64": (3, 9, 11, 64),
    "wrap_N2_C256": (2, 160, 161, 256), "cap_C512_nblocks499": (1, 1, 18433, 512)}


@cache
def in_inputs(name):
    N, H, W, C = IN_CASES[name]
    if name in BN_CASES and BN_CASES[name] == IN_CASES[name]:                   # one image: the tensors of the BatchNorm case serve
        i = bn_inputs(name)
        return dict(z=i["z"], gy=i["gy"], mean=i["mean"].view(1, C), var=i["var"].view(1, C))
    per_image = torch.tensor([1.0, 2.5, 0.3])[:N].view(N, 1, 1, 1)              # a different scale per image
    z = K.rnd(N, C, H, W, seed=950).mul_(2.0 * per_image).add_(K.rnd(1, C, 1, 1, seed=951))
    return dict(z=z, gy=K.rnd(N, C, H, W, seed=952), mean=z.double().mean(dim=(2, 3)), var=z.double().var(dim=(2, 3), unbiased=False))


# (the two large cases run once, with the fused ReLU.  The statistics are per image, so the block cap is reached through the pixels
# of ONE image: C = 512 over 18 433 pixels does, C = 16 over 513 x 512 pixels per image asks for 257 blocks and does not -- that
# shape is a BatchNorm case only, where the two images together ask for 513.)
IN_PARAMS = [(n, r) for n, (N, H, W, C) in IN_CASES.items() for r in (True, False) if r or N * H * W * C <= 1 << 20]


@gpu
@pytest.mark.parametrize("name,relu", IN_PARAMS, ids=["%s-%s" % (n, "relu" if r else "noact") for n, r in IN_PARAMS])
def test_instancenorm_window(name, relu):
    ops = _ops()
    N, H, W, C = IN_CASES[name]
    i = in_inputs(name)
    pre64, _ = bn_forward_ref(name, True)
    zv, yv = win(i["z"], 4, keep=True), blank(N, H, W, C, 8)
    mean, inv = torch.zeros(N * C, device=DEV), torch.zeros(N * C, device=DEV)
    same_after(lambda: ops.instnorm_fwd(zv, yv, mean, inv, act=ops.ACT_RELU if relu else ops.ACT_NONE, slope=0.0), zv)
    yd = got(yv)
    close(yd, F.relu(pre64) if relu else pre64, tol=1e-5, what="instnorm fwd")
    close(mean.view(N, C).cpu(), i["mean"], tol=1e-6, what="instnorm mean")
    close(inv.view(N, C).cpu(), 1.0 / (i["var"] + EPS).sqrt(), tol=1e-6, what="instnorm invstd")
    y2, mean2, inv2 = blank(N, H, W, C, 8), torch.zeros(N * C, device=DEV), torch.zeros(N * C, device=DEV)
    ops.instnorm_fwd(zv, y2, mean2, inv2, act=ops.ACT_RELU if relu else ops.ACT_NONE, slope=0.0)
    assert torch.equal(y2.buf, yv.buf) and torch.equal(mean2, mean) and torch.equal(inv2, inv)      # fixed order: the same bits
    gatef = (yd.cpu() > 0).double() if relu else torch.ones(yd.shape, dtype=D)
    ((gz64,),) = bn_backward_ref(name, gatef, True)
    gyv, gzv = win(i["gy"], 12, keep=True), blank(N, H, W, C, 16)
    same_after(lambda: ops.instnorm_bwd(gyv, yv, zv, gzv, mean, inv, mslope=0.0 if relu else 1.0), gyv, yv, zv)
    close(got(gzv), gz64, tol=2e-5, what="instnorm bwd")
    gz2 = blank(N, H, W, C, 16)
    ops.instnorm_bwd(gyv, yv, zv, gz2, mean, inv, mslope=0.0 if relu else 1.0)
    assert torch.equal(gz2.buf, gzv.buf)
    outside_untouched(yv, gzv)


@gpu
def test_norm_entry_points_reject_empty_and_odd_channel_counts():
    """pixels == 0 (bn_plan would divide by zero on the host) and C == 0 / C % 4 != 0 are refused by every BatchNorm entry point
    before anything is launched: the destination keeps its sentinel."""
    from trainner_amd import hip
    ops = _ops()
    lib = hip.load()
    C = 8
    zv, yv, gv = win(K.rnd(1, C, 2, 3, seed=960), 4), blank(1, 2, 3, C, 8), blank(1, 2, 3, C, 12)
    f = [torch.ones(C, device=DEV) for _ in range(6)]
    ws = torch.zeros(lib.tnr_bn_workspace_bytes(C) // 8, dtype=D, device=DEV)
    s = hip.stream()

    def fwd(pixels, c):
        return lib.tnr_bn_train_fwd_stats(zv.c(), yv.c(), pixels, c, f[0].data_ptr(), f[1].data_ptr(), None, None, None, 0.1, EPS, f[2].data_ptr(),
                                          f[3].data_ptr(), None, ops.ACT_LRELU, 0.2, ws.data_ptr(), s)

    def bwd(pixels, c):
        return lib.tnr_bn_train_bwd(gv.c(), yv.c(), zv.c(), gv.c(), pixels, c, f[0].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), 0.2, None, None,
                                    0.0, ws.data_ptr(), s)

    def bwd_z(pixels, c):
        return lib.tnr_bn_train_bwd_z(gv.c(), zv.c(), gv.c(), pixels, c, f[0].data_ptr(), f[1].data_ptr(), f[2].data_ptr(), f[3].data_ptr(), 0.2,
                                      None, None, 0.0, ws.data_ptr(), s)

    for call in (fwd, bwd, bwd_z):
        for pixels, c, msg in ((0, C, "no pixels"), (6, 0, "unsupported C"), (6, 6, "unsupported C")):
            with pytest.raises(hip.HipEngineError, match=msg):
                hip.check(call(pixels, c), call.__name__)
    torch.cuda.synchronize()
    assert bool((yv.buf == SENT).all()) and bool((gv.buf == SENT).all())


# =====================================================================================================================
# 4. reductions and losses
# =====================================================================================================================
@gpu
@pytest.mark.parametrize("n", FLAT_N, ids=["tiny1", "tiny255", "tiny256", "tiny257", "cap600001"])
def test_l1_and_sumsq_cap(n):
    ops = _ops()
    a, b, _ = flat_case(n)
    ad, bd = a.to(DEV), b.to(DEV)
    outs = [torch.zeros((), device=DEV) for _ in range(2)]
    for o in outs:
        ops.l1_mean_fwd(ad, bd, 0.7, o)
    ref = 0.7 * float((a.double() - b.double()).abs().mean())
    assert abs(float(outs[0]) - ref) <= 1e-6 * (abs(ref) + 1.0), (float(outs[0]), ref)
    assert torch.equal(outs[0], outs[1])                                  # fixed summation order: the same bits
    ss = [torch.zeros(1, dtype=D, device=DEV) for _ in range(2)]
    for o in ss:
        ops.sumsq(ad, o)
    ref = float((a.double() ** 2).sum())
    assert abs(float(ss[0]) - ref) <= 1e-6 * (abs(ref) + 1.0), (float(ss[0]), ref)
    assert torch.equal(ss[0], ss[1])


@cache
def gan_case(n, kind, target):
    p = K.rnd(n, seed=1000, lo=-30.0, hi=30.0)                            # out to +-30: both softplus tails
    pr = p.double().requires_grad_(True)
    tt = torch.full_like(pr, target)
    loss = F.binary_cross_entropy_with_logits(pr, tt) if kind == 0 else (F.mse_loss(pr, tt) if kind == 1 else pr.mean())
    (g,) = torch.autograd.grad(loss, pr)
    return p, float(loss.detach()), g


@gpu
@pytest.mark.parametrize("kt", [(0, 1.0), (0, 0.0), (1, 1.0), (1, 0.0), (2, 0.0)], ids=["bce1", "bce0", "mse1", "mse0", "mean"])
@pytest.mark.parametrize("n", [1, 257, 14400], ids=["tiny1", "n257", "n14400"])
def test_gan_loss_tails(n, kt):
    ops = _ops()
    kind, target = kt
    p, loss, g = gan_case(n, kind, target)
    pd = p.to(DEV)
    outs, grads = [torch.zeros(1, device=DEV) for _ in range(2)], [torch.full((n,), float("nan"), device=DEV) for _ in range(2)]
    for o, gr in zip(outs, grads):
        ops.gan_loss(pd, kind, target, o, gr)
    assert abs(float(outs[0]) - loss) <= 1e-6 * (abs(loss) + 1.0), (float(outs[0]), loss)
    close(grads[0].cpu() * n, g * n, tol=1e-6, what="gan loss grad (times n)")
    assert torch.equal(outs[0], outs[1]) and torch.equal(grads[0], grads[1])
    o3 = torch.zeros(1, device=DEV)
    ops.gan_loss(pd, kind, target, o3, None)                              # no gradient asked for
    assert torch.equal(o3, outs[0])


RAGAN_N = [6, 4095, 4096, 4097, 256 * 4096 + 4097]


@cache
def ragan_case(n, stage):
    from oracle import sr_oracle as O
    pf = (K.rnd(n, 1, seed=1010) * 3.0).double().requires_grad_(True)
    pr = (K.rnd(n, 1, seed=1011) * 3.0 + 0.5).double().requires_grad_(True)
    if stage == 0:
        l1, l2 = O.bce_logits(pr.detach() - pf.mean(), False), O.bce_logits(pf - pr.detach().mean(), True)
        (gf,) = torch.autograd.grad((l1 + l2) * 0.5, pf)
        gr = torch.zeros_like(pr)
    else:
        l1, l2 = O.ragan_d_loss(pf, pr)
        gf, gr = torch.autograd.grad((l1 + l2) * 0.5, (pf, pr))
    return pf.detach().float().view(-1), pr.detach().float().view(-1), float(l1.detach()), float(l2.detach()), gf.view(-1), gr.view(-1)


@gpu
@pytest.mark.parametrize("stage", [0, 1], ids=["gen", "disc"])
@pytest.mark.parametrize("n", RAGAN_N, ids=["tiny6", "below4095", "at4096", "above4097", "cap1052673"])
def test_ragan_phases_cap(n, stage):
    """the three relativistic phases on both sides of RAGAN_MULTI_MIN and past the 256-block cap, with scratch (two-stage grid
    forms) and without (one block); the loss weight is n so that the per-logit gradients are of order one under the bound"""
    from trainner_amd import hip
    lib = hip.load()
    pf, pr, l1, l2, gf_r, gr_r = ragan_case(n, stage)
    pfd, prd = pf.to(DEV), pr.to(DEV)
    s = hip.stream()
    wgt = float(n)
    runs = []
    for scratch in (True, True, False):
        ws = torch.zeros(lib.tnr_reduce_workspace_bytes() // 8, dtype=D, device=DEV) if scratch else None
        sums, o5 = torch.zeros(8, device=DEV), torch.zeros(5, device=DEV)
        gf, gr = torch.full((n,), float("nan"), device=DEV), torch.full((n,), float("nan"), device=DEV)
        hip.check(lib.tnr_ragan_phase_a(pfd.data_ptr(), prd.data_ptr(), n, sums.data_ptr(), hip.ptr(ws), s))
        hip.check(lib.tnr_ragan_phase_b(pfd.data_ptr(), prd.data_ptr(), n, stage, sums.data_ptr(), hip.ptr(ws), s))
        hip.check(lib.tnr_ragan_phase_c(pfd.data_ptr(), prd.data_ptr(), n, stage, wgt, sums.data_ptr(), o5.data_ptr(), gf.data_ptr(), gr.data_ptr(), s))
        o = o5.cpu().double()
        assert abs(float(o[1]) - l1) <= 1e-6 * (abs(l1) + 1.0) and abs(float(o[2]) - l2) <= 1e-6 * (abs(l2) + 1.0), (o, l1, l2)
        assert abs(float(o[0]) / wgt - 0.5 * (l1 + l2)) <= 1e-6 * (0.5 * (l1 + l2) + 1.0)
        assert abs(float(o[3]) - float(pr.double().mean())) <= 1e-6 * 2 and abs(float(o[4]) - float(pf.double().mean())) <= 1e-6 * 2
        close(gf.cpu(), gf_r * wgt, tol=1e-6, what="ragan gf (times n)")
        close(gr.cpu(), gr_r * wgt, tol=1e-6, what="ragan gr (times n)")
        runs.append((sums, o5, gf, gr))
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)                                          # fixed order: two launches, the same bits


BIAS_CASES = {      # N, H, W, C, coff
    "tiny1px_oddC4": (1, 1, 1, 4, 4), "oddC12": (2, 9, 11, 12, 4), "oddC48": (2, 33, 17, 48, 8), "oddC96": (1, 33, 17, 96, 4),
    "generic_C6_unaligned": (2, 9, 11, 6, 3), "cap_C512_nblocks499": (1, 1, 18433, 512, 4), "cap_C16": (2, 513, 512, 16, 8)}


@cache
def bias_case(name):
    N, H, W, C, _ = BIAS_CASES[name]
    big = {"cap_C512_nblocks499": "cap_C512_nblocks499", "cap_C16": "cap_wrap_C16"}.get(name)
    g = bn_inputs(big)["gy"] if big else K.rnd(N, C, H, W, seed=1020)          # (the large tensors are drawn once)
    assert tuple(g.shape) == (N, C, H, W)
    return g, g.double().sum(dim=(0, 2, 3)), K.rnd(C, seed=1021)


@gpu
@pytest.mark.parametrize("name", list(BIAS_CASES))
def test_bias_grad_window_cap(name):
    ops = _ops()
    N, H, W, C, coff = BIAS_CASES[name]
    g, ref, d0 = bias_case(name)
    buf = K.nhwc_buf(g, coff + C + (5 if C % 4 else hi_pad(coff, C)), coff, fill=SENT)     # C = 6: nothing aligned
    gv = ops.View(buf, coff, C)
    dbs = [d0.to(DEV) for _ in range(2)]
    for d in dbs:
        same_after(lambda: ops.bias_grad(gv, d, alpha=0.5, beta=2.0), gv)
    close(dbs[0].cpu(), 2.0 * d0.double() + 0.5 * ref, tol=2e-6, what="bias_grad")
    assert torch.equal(dbs[0], dbs[1])
    d3 = torch.full((C,), float("nan"), device=DEV)
    ops.bias_grad(gv, d3, alpha=1.5, beta=0.0)                            # beta = 0: db is not read
    close(d3.cpu(), 1.5 * ref, tol=2e-6, what="bias_grad beta 0")


# =====================================================================================================================
# 5. linear and Adam
# =====================================================================================================================
LINEAR_CASES = {"disc_8192_100": (3, 8192, 100), "disc_100_1": (3, 100, 1), "in130_below256": (2, 130, 5)}


@cache
def linear_inputs(name):
    N, In, Out = LINEAR_CASES[name]
    a = 1.0 / math.sqrt(In)
    x, w, b = K.rnd(N, In, seed=1100), K.rnd(Out, In, seed=1101, lo=-a, hi=a), K.rnd(Out, seed=1102)
    return x, w, b, K.rnd(N, Out, seed=1103), K.rnd(Out, In, seed=1104), K.rnd(Out, seed=1105), (F.linear(x.double(), w.double(), b.double()))


_LIN = {}


@gpu
@pytest.mark.parametrize("name", list(LINEAR_CASES))
def test_linear_geometries(name):
    from trainner_amd import hip
    ops = _ops()
    N, In, Out = LINEAR_CASES[name]
    x, w, b, gy, dw0, db0, pre64 = linear_inputs(name)
    xd, wd, bd, gyd = x.to(DEV), w.to(DEV), b.to(DEV), gy.to(DEV)
    yd = torch.full((N, Out), float("nan"), device=DEV)
    ops.linear_fwd(xd, wd, bd, yd, act=ops.ACT_LRELU, slope=0.2)
    close(yd.cpu(), F.leaky_relu(pre64, S32), what="linear fwd")
    y0 = torch.full((N, Out), float("nan"), device=DEV)
    ops.linear_fwd(xd, wd, None, y0, act=ops.ACT_NONE)
    close(y0.cpu(), pre64 - b.double(), what="linear fwd, no bias, no activation")
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)      # noqa: E731
    for gated in (True, False):
        gatef = gate(yd.cpu()) if gated else torch.ones(N, Out, dtype=D)
        gx_r, dw_r, db_r = linear_backward_ref(name, gated, gatef)
        ya = yd if gated else None
        gx, dw, db = nan(N, In), nan(Out, In), nan(Out)           # acc_beta = 0: dw / db are not read
        ops.linear_bwd(xd, wd, gyd, ya, gx=gx, dw=dw, db=db, acc_beta=0.0, mslope=0.2)
        close(gx.cpu(), gx_r, what="linear gx")
        close(dw.cpu(), dw_r, what="linear dw")
        close(db.cpu(), db_r, what="linear db")
        dwa, dba = dw0.to(DEV), db0.to(DEV)
        ops.linear_bwd(xd, wd, gyd, ya, gx=None, dw=dwa, db=dba, acc_beta=1.0, mslope=0.2)      # gx omitted, accumulate
        close(dwa.cpu(), dw0.double() + dw_r, what="linear dw accumulate")
        close(dba.cpu(), db0.double() + db_r, what="linear db accumulate")
        dw2 = nan(Out, In)
        ops.linear_bwd(xd, wd, gyd, ya, gx=None, dw=dw2, db=None, acc_beta=0.0, mslope=0.2)     # db omitted
        assert torch.equal(dw2, dw)
        gx2 = nan(N, In)
        ops.linear_bwd(xd, wd, gyd, ya, gx=gx2, dw=None, db=None, acc_beta=0.0, mslope=0.2)     # dw (and with it db) omitted
        assert torch.equal(gx2, gx)
    # db is written by the dw launch: asking for it alone is refused (it used to be left unwritten without a word)
    dbx = nan(Out)
    with pytest.raises(hip.HipEngineError, match="linear_bwd"):
        ops.linear_bwd(xd, wd, gyd, None, gx=None, dw=None, db=dbx, acc_beta=0.0)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dbx).all())


def linear_backward_ref(name, gated, gatef):
    hit = _LIN.get((name, gated))
    if hit is not None and torch.equal(hit[0], gatef):
        return hit[1]
    x, w, b, gy = linear_inputs(name)[:4]
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    res = torch.autograd.grad(F.linear(xr, wr, br), (xr, wr, br), gy.double() * gatef)
    _LIN[(name, gated)] = (gatef, res)
    return res


ADAM_N = [1, 257, 600001]
LR, B1, B2, AEPS = 1e-4, 0.9, 0.999, 1e-8


@cache
def adam_case(n, wd):
    """three steps of torch.optim.Adam(weight_decay=wd) in fp64 (reference) and fp32 (yardstick) with gradients g0 * t"""
    p0, g0 = K.rnd(n, seed=1200), K.rnd(n, seed=1201) * 0.01
    res = []
    for dtype in (D, torch.float32):
        p = p0.to(dtype).clone().requires_grad_(True)
        opt = torch.optim.Adam([p], lr=LR, betas=(B1, B2), eps=AEPS, weight_decay=wd)
        for t in range(1, 4):
            p.grad = (g0 * t).to(dtype)
            opt.step()
        st = opt.state[p]
        res.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone()))
    return p0, g0, res[0], res[1]


@gpu
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=["wd0", "wd1e-2"])
@pytest.mark.parametrize("n", ADAM_N, ids=["tiny1", "n257", "wrap600001"])
def test_adam_three_steps(n, wd):
    ops = _ops()
    p0, g0, r64, r32 = adam_case(n, wd)
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t in range(1, 4):
        ops.adam_step(pd, (g0 * t).to(DEV), md, vd, LR / (1 - B1 ** t), B1, B2, math.sqrt(1 - B2 ** t), AEPS, wd=wd)
    for what, dev, a, b in (("p", pd, r64[0], r32[0]), ("exp_avg", md, r64[1], r32[1]), ("exp_avg_sq", vd, r64[2], r32[2])):
        yardstick("adam %s n=%d wd=%g" % (what, n, wd), dev, a, b)
    # the unguarded export (tnr_adam_step: no fault latch) is the same kernel: the same bits
    from trainner_amd import hip
    p2, m2, v2 = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for t in range(1, 4):
        g = (g0 * t).to(DEV)
        hip.check(hip.load().tnr_adam_step(p2.data_ptr(), g.data_ptr(), m2.data_ptr(), v2.data_ptr(), n, LR / (1 - B1 ** t), B1, B2,
                                           math.sqrt(1 - B2 ** t), AEPS, wd, hip.stream()), "adam_step")
    assert torch.equal(p2, pd) and torch.equal(m2, md) and torch.equal(v2, vd)


# =====================================================================================================================
# the device-free self-check of every case's inputs and reference
# =====================================================================================================================
def test_inputs_and_references():
    """Builds every case's inputs and fp64 reference on the CPU (no device).  No tensor a kernel gates on has more than 0.1 % of
    its elements within 1e-5 of zero -- the tests skip none, this bounds how many COULD sit on the fence --; the max-pool ties
    exist in the planted quarter of the windows, with the first maximum taking the gradient; every yardstick (the error of the
    fp32 PyTorch-CPU op against fp64) is non-zero, so no yardstick bound degenerates to its additive term by accident of a
    reference that happens to be exact."""
    # this module has no module-level gpu mark (see the docstring): every other test of it must carry the mark itself
    for k, f in list(globals().items()):
        if k.startswith("test_") and k != "test_inputs_and_references":
            assert any(m.name == "gpu" for m in getattr(f, "pytestmark", [])), "%s lacks @gpu" % k
    fin = lambda *ts: all(bool(torch.isfinite(t).all()) for t in ts)      # noqa: E731
    for C, _ in N2H.values():
        for shape in LAYOUT_SHAPES:
            assert fin(*n2h_case(C, shape))
    for shape in H2N_SHAPES:
        assert fin(*h2n_case(shape))
    for shape in D2S_SHAPES:
        assert near_zero_share(d2s_case(shape)[2]) <= 1e-3
    for shape in POOL_SHAPES:
        xt, gp, pooled, gref, sel = pool_case(shape)
        ties = tie_share(xt)
        assert not bool((sel & ~ties).any()), "every planted window holds a tie"
        share = float(ties.double().mean())
        if shape != "tiny":
            assert 0.2 <= share <= 0.3, share
            assert float((sel & ~tie_share(F.relu(K.rnd(*xt.shape, seed=730)))).double().mean()) >= 0.2       # planted, not found
        # the gradient of a tied window sits on its first maximum only
        N, C, H, W = xt.shape
        gw = gref.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
        xw = xt.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
        first = xw.argmax(dim=-1, keepdim=True)          # ties: torch returns the first index of the maximum on the CPU
        assert bool(((gw != 0).sum(-1) <= 1).all())
        assert bool((gw.gather(-1, first).squeeze(-1)[ties] == gp[ties]).all())
    for shape in PAD_SHAPES:
        for pad in (1, 2, 3):
            assert fin(*pad_case(shape, pad))
    for name in WINDOW_CASES:
        assert fin(*window_case(name))
    for shape in PIX_SHAPES:
        assert near_zero_share(pix_case(shape)[2]) <= 1e-3
    for name in IM2COL_CASES:
        assert fin(*im2col_case(name))
    for shape in UP_SHAPES:
        c = up_case(shape)
        assert near_zero_share(c[1]) <= 1e-3 and fin(*c)
    assert fin(*tanh_wrap_case())
    for n in FLAT_N:
        a, b, _ = flat_case(n)
        assert near_zero_share(a - b) <= 1e-3 or n == 1               # the sign of the L1 backward
    yard = {}
    for name in BN_CASES:
        i = bn_inputs(name)
        pre64, pre32 = bn_forward_ref(name)
        assert near_zero_share(pre64) <= 1e-3, name                   # the activation gate of the backward
        if name.startswith("shifted"):
            assert bool(((i["mean"] - 3.0).abs() < 0.25).all()) and bool(((i["var"].sqrt() - 0.05).abs() < 0.005).all())
            yard["bn fwd " + name] = float((pre32.double() - pre64).abs().max())
        else:
            assert bool((i["mean"].abs() <= i["var"].sqrt()).all()) or i["n"] < 100
        assert bool((i["mean"].abs() >= 0.01 * i["var"].sqrt()).all()), name      # stat64's mean is checked RELATIVE to it
        (gz64, gg64, gb64), (gz32, gg32, gb32) = bn_backward_ref(name, gate(pre64))
        for k, a, b in (("gz", gz64, gz32), ("dgamma", gg64, gg32), ("dbeta", gb64, gb32)):
            yard["bn bwd %s %s" % (k, name)] = float((b.double() - a).abs().max())
    for name in IN_CASES:
        pre64, _ = bn_forward_ref(name, True)
        assert near_zero_share(pre64) <= 1e-3, name
        assert fin(*bn_backward_ref(name, (pre64 > 0).double(), True)[0])
    for n in (1, 257, 14400):
        for kind, target in ((0, 1.0), (0, 0.0), (1, 1.0), (1, 0.0), (2, 0.0)):
            p, loss, g = gan_case(n, kind, target)
            assert math.isfinite(loss) and fin(g) and (n == 1 or float(p.abs().max()) > 25.0)
    for n in RAGAN_N:
        for stage in (0, 1):
            c = ragan_case(n, stage)
            assert math.isfinite(c[2]) and math.isfinite(c[3]) and fin(c[4], c[5])
    for name in BIAS_CASES:
        assert fin(*bias_case(name))
    for name in LINEAR_CASES:
        pre64 = linear_inputs(name)[6]
        assert float((pre64.abs() < 1e-5).double().sum()) <= max(1.0, 1e-3 * pre64.numel()), name
        assert fin(*linear_backward_ref(name, True, gate(pre64)))
    for n in ADAM_N:
        for wd in (0.0, 1e-2):
            _, _, r64, r32 = adam_case(n, wd)
            for k, a, b in zip(("p", "exp_avg", "exp_avg_sq"), r64, r32):
                yard["adam %s n=%d wd=%g" % (k, n, wd)] = float((b.double() - a).abs().max())
    zero = [k for k, v in yard.items() if not v > 0.0]
    assert not zero, zero
