"""conv + ReLU + MaxPool2d(2, 2) as ONE launch (ops.conv_pool2: the pooled store of the Winograd form) and the gradient
routed by its byte map (ops.unpool2_bwd), against the present pair on the same operands, BIT FOR BIT (torch.equal):
    the Winograd launch (ops.conv, wino=True) + ops.maxpool2_fwd, and ops.maxpool2_bwd on the full-resolution map it stored.
Nothing here is compared with a tolerance: `max` is exact and every value entering it goes through the plain store's own arithmetic.

Shapes (N x H x W, cin -> cout), the smallest at which each path of the store can go wrong:
  1 x 16 x 16, 64 -> 64     one tile
  2 x 32 x 40, 64 -> 64     ragged in W, two images, several tiles
  1 x 18 x 22, 64 -> 64     ragged both ways, an odd number of patches per ragged tile row
  1 x 64 x 64, 128 -> 128   two cout blocks, two input-chunk pairs
  1 x 16 x 16, 64 -> 512    eight cout blocks (the width of the 64 x 64 stage) at a small size
each without the map (nothing saved), with it, and with it into a channel-offset output view.  Ties: 1 x 16 x 16 and 2 x 32 x 40 again with
inputs, bias and (sparse) weights in {-1, 0, 1}: every form computes those sums exactly, equal maxima and all-zero windows are frequent
(the test asserts that at least a quarter of the windows tie under the present kernels' own output), and values, routed gradients and
zeros must still equal the present kernels'.  Declines: odd H, LeakyReLU, an r1 operand and the f32 matrix-core arithmetic each get
"no" from tnr_conv_pool_ok and launch nothing.

Network level: FeatureExtractor(["conv5_4"]) at 2 x 3 x 64 x 64, fold on against fold off -- feature and input gradient bit-identical.  At
that size only conv1_2 is a Winograd launch (ops.conv_plan: conv2_2 and conv3_4 lie under WINO_MIN_PIXELS, conv4_4 at 8 x 8 is a
split-K conv_tile launch), so the fold takes pool1 and the other three keep their launches -- the counters say exactly that; the
same comparison at 2 x 3 x 736 x 736, the smallest square input at which conv4_4 (92 x 92 x 2 = 16 928 pixels > 16 384) is a Winograd
launch too, shows ZERO maxpool2_fwd / maxpool2_bwd calls.  A multi-tap list with relu1_2 keeps conv1_2 + pool1 as they are, folds
conv2_2 + pool2 (itself a tap: the stored tensor), and equals the fold-off run bit for bit.

The pooled store exists in the bf16x3 arithmetic only (the Winograd form), so these tests pin ops.MMA to it in both parametrisations of
the suite; test_declines covers f32.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.0
SHAPES = [(1, 16, 16, 64, 64), (2, 32, 40, 64, 64), (1, 18, 22, 64, 64), (1, 64, 64, 128, 128), (1, 16, 16, 64, 512)]
IDS = ["tile16", "ragged32x40", "ragged18x22", "c128", "cout512"]
TIE_SHAPES, TIE_IDS = SHAPES[:2], IDS[:2]
VARIANTS = ["nomap", "map", "map_offset_view"]


def _engine(monkeypatch):
    from trainner_amd import hip, ops
    monkeypatch.setattr(ops, "FP32_MMA", hip.MMA_BF16X3)
    monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    monkeypatch.delenv("TNR_POOL_FOLD", raising=False)
    return hip, ops


@functools.lru_cache(maxsize=None)
def _case(shape, integers=False):
    """Operands of one layer (fp32, CPU, NHWC / OIHW); computed once, shared, never written."""
    N, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(4000 + 11 * H + W + Cout)
    if integers:          # sparse {-1, 0, 1} weights: sums of a dozen terms, so that equal maxima are frequent
        x = torch.randint(-1, 2, (N, H, W, Cin), generator=gen).float()
        w = torch.randint(-1, 2, (Cout, Cin, 3, 3), generator=gen).float() * (torch.rand(Cout, Cin, 3, 3, generator=gen) < 1.0 / 64).float()
        b = torch.randint(-1, 2, (Cout,), generator=gen).float()
    else:
        x = torch.randn(N, H, W, Cin, generator=gen)
        w = torch.randn(Cout, Cin, 3, 3, generator=gen) * (Cin * 9) ** -0.5
        b = torch.randn(Cout, generator=gen)
    g = torch.randn(N, H // 2, W // 2, Cout, generator=gen)
    return dict(x=x, w=w, b=b, g=g)


def _packed(ops, w):
    packer = ops.WeightPacker(torch.device(DEV))
    i = packer.add(w, ops.PACK_FWD)
    packer.run()
    return packer, packer.get(i)


def _present(ops, c, shape, act):
    """The present pair on the device -> (full-resolution map, pooled map, input gradient of the pool)."""
    N, H, W, Cin, Cout = shape
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    packer, wp = _packed(ops, w)
    x, g = ops.View(c["x"].to(DEV)), ops.View(c["g"].to(DEV))
    full = ops.View(torch.full((N, H, W, Cout), SENTINEL, device=DEV))
    ops.conv(x, wp, full, wino=True, bias=b, act=act)
    pooled = ops.View(torch.full((N, H // 2, W // 2, Cout), SENTINEL, device=DEV))
    ops.maxpool2_fwd(full, pooled)
    gx = ops.View(torch.full((N, H, W, Cout), SENTINEL, device=DEV))
    ops.maxpool2_bwd(g, full, gx)
    return full.buf, pooled.buf, gx.buf


def _route_of(full):
    """The byte map from the full-resolution activation by the present kernels' rule (scan k = 0 .. 3, `v > best`; bit 2: best > 0)."""
    N, H, W, Cc = full.shape
    v = full.reshape(N, H // 2, 2, W // 2, 2, Cc)
    best, arg = v[:, :, 0, :, 0], torch.zeros((N, H // 2, W // 2, Cc), dtype=torch.uint8, device=full.device)
    for k in (1, 2, 3):
        vk = v[:, :, k >> 1, :, k & 1]
        gt = vk > best
        best, arg = torch.where(gt, vk, best), torch.where(gt, torch.full_like(arg, k), arg)
    return arg | ((best > 0).to(torch.uint8) << 2)


def _folded(ops, c, shape, act, variant):
    """The pooled launch (+ map, + the gradient routed by it) -> (pooled buffer, route, gx buffer); the buffers whole, so that an
    offset view's other channels are compared too."""
    N, H, W, Cin, Cout = shape
    w, b = c["w"].to(DEV), c["b"].to(DEV)
    packer, wp = _packed(ops, w)
    x, g = ops.View(c["x"].to(DEV)), ops.View(c["g"].to(DEV))
    off = 32 if variant == "map_offset_view" else 0
    ybuf = torch.full((N, H // 2, W // 2, Cout + 2 * off), SENTINEL, device=DEV)
    route = None if variant == "nomap" else torch.full((N, H // 2, W // 2, Cout), 255, dtype=torch.uint8, device=DEV)
    assert ops.conv_pool2(x, wp, ops.View(ybuf, off, Cout), route=route, wino=True, bias=b, act=act) is True
    gxbuf = None
    if route is not None:
        gxbuf = torch.full((N, H, W, Cout + 2 * off), SENTINEL, device=DEV)
        ops.unpool2_bwd(g, route, ops.View(gxbuf, off, Cout))
    return ybuf, route, gxbuf, off


def _same(ops, c, shape, act, variant):
    N, H, W, Cin, Cout = shape
    full, pooled, gx = _present(ops, c, shape, act)
    ybuf, route, gxbuf, off = _folded(ops, c, shape, act, variant)
    torch.cuda.synchronize()
    assert torch.equal(ybuf[..., off:off + Cout], pooled)
    assert off == 0 or (bool((ybuf[..., :off] == SENTINEL).all()) and bool((ybuf[..., off + Cout:] == SENTINEL).all()))
    if route is not None:
        assert torch.equal(route, _route_of(full))
        assert torch.equal(gxbuf[..., off:off + Cout], gx)
        assert off == 0 or (bool((gxbuf[..., :off] == SENTINEL).all()) and bool((gxbuf[..., off + Cout:] == SENTINEL).all()))
    return full


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_pooled_store_equals_conv_then_pool(shape, variant, monkeypatch):
    hip, ops = _engine(monkeypatch)
    _same(ops, _case(shape), shape, ops.ACT_RELU, variant)


def test_pooled_store_without_activation(monkeypatch):
    """No activation: negative maxima; bit 2 of the byte then does real work in the gradient."""
    hip, ops = _engine(monkeypatch)
    full = _same(ops, _case(SHAPES[1]), SHAPES[1], ops.ACT_NONE, "map")
    assert bool((full < 0).any())


@pytest.mark.parametrize("variant", ["nomap", "map"])
@pytest.mark.parametrize("shape", TIE_SHAPES, ids=TIE_IDS)
def test_ties_and_zero_windows(shape, variant, monkeypatch):
    hip, ops = _engine(monkeypatch)
    full = _same(ops, _case(shape, integers=True), shape, ops.ACT_RELU, variant)
    N, H, W, Cc = full.shape
    v = full.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)
    best = v.max(dim=-1, keepdim=True).values
    tied = float(((v == best).sum(-1) >= 2).float().mean())
    zero = float((best == 0).float().mean())
    print("windows with a tie: %.3f, all-zero windows: %.3f" % (tied, zero))
    assert tied >= 0.25 and zero > 0.0, (tied, zero)


def test_tape_stand_in_names_the_winners_and_their_branches(monkeypatch):
    """PooledAway.dense(), what the gate-pinned oracle reads off the tape in the place of the map that was never stored: the window
    maximum sits at the position the present rule picks (ties included: integer operands), alone, and carries the pooled value."""
    hip, ops = _engine(monkeypatch)
    from trainner_amd.models.modules.architectures.perceptual import PooledAway
    shape = TIE_SHAPES[1]
    c = _case(shape, integers=True)
    full, pooled, _ = _present(ops, c, shape, ops.ACT_RELU)
    ybuf, route, _, _ = _folded(ops, c, shape, ops.ACT_RELU, "map")
    s = PooledAway(route, ops.View(ybuf)).dense()
    assert s.shape == full.shape
    N, H, W, Cc = s.shape
    win = s.reshape(N, H // 2, 2, W // 2, 2, Cc).permute(0, 1, 3, 5, 2, 4).reshape(N, H // 2, W // 2, Cc, 4)
    assert torch.equal(win.max(dim=-1).values, pooled)
    assert bool(((win > float("-inf")).sum(-1) == 1).all())
    assert torch.equal(win.argmax(dim=-1).to(torch.uint8), _route_of(full) & 3)


def _desc(hip, ops, x, wp, y, **epi):
    d = hip.ConvDesc()
    ops._conv_desc(d, x, wp, y, ops.CONV_3x3, **epi)
    d.Ho, d.Wo = x.H, x.W
    return d


@pytest.mark.parametrize("why", ["odd_h", "lrelu", "r1", "mma_f32"])
def test_declines(why, monkeypatch):
    """The library's answer is "no", ops.conv_pool2 returns False and nothing is written."""
    hip, ops = _engine(monkeypatch)
    lib = hip.load()
    N, H, W, Cc = 1, (17 if why == "odd_h" else 16), 16, 64
    c = _case((1, 16, 16, 64, 64))
    packer, wp = _packed(ops, c["w"].to(DEV))
    b = c["b"].to(DEV)
    x = ops.View(torch.zeros((N, H, W, Cc), device=DEV))
    y = ops.View(torch.full((N, H // 2, W // 2, Cc), SENTINEL, device=DEV))
    ok = _desc(hip, ops, ops.View(torch.zeros((1, 16, 16, Cc), device=DEV)), wp, y, bias=b, act=ops.ACT_RELU)
    assert lib.tnr_conv_pool_ok(C.byref(ok)) == 1          # (the control: the same launch without the reason to decline)
    epi = dict(bias=b, act=ops.ACT_RELU)
    if why == "lrelu":
        epi = dict(bias=b, act=ops.ACT_LRELU, slope=0.2)
    elif why == "r1":
        epi["r1"] = ops.View(torch.zeros((N, H, W, Cc), device=DEV))
    elif why == "mma_f32":
        monkeypatch.setattr(ops, "MMA", hip.MMA_F32)
    assert lib.tnr_conv_pool_ok(C.byref(_desc(hip, ops, x, wp, y, **epi))) == 0
    assert ops.conv_pool2(x, wp, y, wino=None if why == "mma_f32" else True, **epi) is False
    torch.cuda.synchronize()
    assert bool((y.buf == SENTINEL).all())


def test_switch_keeps_the_two_launches(monkeypatch):
    hip, ops = _engine(monkeypatch)
    c = _case(SHAPES[0])
    packer, wp = _packed(ops, c["w"].to(DEV))
    x = ops.View(c["x"].to(DEV))
    y = ops.View(torch.full((1, 8, 8, 64), SENTINEL, device=DEV))
    monkeypatch.setenv("TNR_POOL_FOLD", "0")          # (read at call time)
    assert ops.conv_pool2(x, wp, y, wino=True, act=ops.ACT_RELU) is False
    torch.cuda.synchronize()
    assert bool((y.buf == SENTINEL).all())
    monkeypatch.setenv("TNR_POOL_FOLD", "1")
    assert ops.conv_pool2(x, wp, y, wino=True, act=ops.ACT_RELU) is True


# ----------------------------------------------------------------------------------------------
# network level
# ----------------------------------------------------------------------------------------------
def _counted(monkeypatch, ops):
    counts = dict(maxpool2_fwd=0, maxpool2_bwd=0, unpool2_bwd=0, conv_pool2=0)

    def wrap(name, fn):
        def counted(*a, **k):
            r = fn(*a, **k)
            counts[name] += 1 if (name != "conv_pool2" or r) else 0
            return r
        monkeypatch.setattr(ops, name, counted)
    for name in counts:
        wrap(name, getattr(ops, name))
    return counts


def _extractor_run(monkeypatch, ops, listen, size, fold):
    """One forward + backward of a seeded FeatureExtractor -> (features, input gradient, launch counts)."""
    from trainner_amd.models.modules.architectures.perceptual import FeatureExtractor
    monkeypatch.setenv("TNR_POOL_FOLD", "1" if fold else "0")
    from oracle import fixtures as FX
    net = FeatureExtractor(listen, allow_random_init=True)
    sd = net.state_dict()
    sd.update({k: v for k, v in FX.vgg_state(77).items() if k in sd})      # seeded weights (a shorter network owns fewer)
    net.load_state_dict(sd)
    net = net.to(DEV)
    gen = torch.Generator().manual_seed(17)
    x = torch.rand(2, 3, size, size, generator=gen).to(DEV).requires_grad_(True)
    counts = _counted(monkeypatch, ops)
    feats = net(x)
    outs = [feats[n] for n in net.taps]
    gouts = [torch.randn(o.shape, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last) for o in outs]
    gx, = torch.autograd.grad(outs, x, gouts)
    torch.cuda.synchronize()
    return [o.detach().clone() for o in outs], gx.detach().clone(), dict(counts)


@pytest.mark.parametrize("size,folds", [(64, 1), (736, 4)], ids=["64_pool1", "736_every_pool"])
def test_extractor_conv5_4_fold_on_equals_fold_off(size, folds, monkeypatch):
    hip, ops = _engine(monkeypatch)
    f1, g1, n1 = _extractor_run(monkeypatch, ops, ["conv5_4"], size, True)
    f0, g0, n0 = _extractor_run(monkeypatch, ops, ["conv5_4"], size, False)
    print("fold on:", n1, "fold off:", n0)
    assert n0 == dict(maxpool2_fwd=4, maxpool2_bwd=4, unpool2_bwd=0, conv_pool2=0)
    assert n1 == dict(maxpool2_fwd=4 - folds, maxpool2_bwd=4 - folds, unpool2_bwd=folds, conv_pool2=folds)
    assert torch.equal(f1[0], f0[0]) and torch.equal(g1, g0)
    assert float(g0.abs().max()) > 0.0


def test_extractor_taps_skip_the_fold_for_a_listened_relu(monkeypatch):
    """relu1_2 listened: conv1_2 + pool1 stay two launches (the tap IS the full-resolution map); conv2_2 + pool2 fold, and the pool2 tap
    is the tensor the launch stored."""
    hip, ops = _engine(monkeypatch)
    listen = ["relu1_2", "pool2", "relu3_1"]
    f1, g1, n1 = _extractor_run(monkeypatch, ops, listen, 128, True)
    f0, g0, n0 = _extractor_run(monkeypatch, ops, listen, 128, False)
    print("fold on:", n1, "fold off:", n0)
    assert n0 == dict(maxpool2_fwd=2, maxpool2_bwd=2, unpool2_bwd=0, conv_pool2=0)
    assert n1 == dict(maxpool2_fwd=1, maxpool2_bwd=1, unpool2_bwd=1, conv_pool2=1)
    assert len(f1) == 3 and all(torch.equal(a, b) for a, b in zip(f1, f0)) and torch.equal(g1, g0)
    assert float(g0.abs().max()) > 0.0
