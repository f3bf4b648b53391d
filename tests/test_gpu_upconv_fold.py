"""The generator's `Upsample(nearest, x2) -> Conv2d(3, 1, 1)` layers folded into the four-tap stride-2 launches (ops.upconv_plan,
DESIGN.md 3.12): engine.ConvOp(ups=True) in its folded form and in the present TNR_CONV_3x3_UP2 form, on the same inputs, against torch
on the CPU in FLOAT64 -- F.interpolate(nearest, 2) -> conv2d(padding 1) -> bias -> LeakyReLU, autograd for both gradients.

Bound: max |folded - fp64| <= 3 x max |present form - fp64| + 2e-7 x max |fp64| -- the allowance the project gives a form of these layers
that is not bit-identical to the direct one (test_gpu_kernels.test_conv3x3_winograd_form_error_vs_fp64).  The yardstick is the present
launch (the code this change leaves alone), in the same bf16x3 arithmetic, on the same operands.

Shapes (N x low-resolution H x W, channels) -- the smallest at which each path can go wrong:
  1 x 16 x 16, 64 -> 64   the stream kernel declines grids narrower than 32 pixels: conv_tile in the four-tap modes
  2 x 32 x 40, 64 -> 64   the stream kernels, a ragged last tile, two images
  1 x 17 x 19, 64 -> 64   odd sizes: every border, ragged tiles in both directions
  1 x 32 x 32, 32 -> 32   Cout % 64 != 0: conv_tile, the 32-cout weight-gradient class
Forward: bias + LeakyReLU(0.2), and no activation.  Data gradient: with the previous activation's mask and without.  Weight and bias
gradient: alpha = 0.5 and beta = 1 over a random non-zero start (ConvOp.wgrad always accumulates).

The forward is folded only on request (TNR_UPCONV_FOLD=fwd,dgrad,wgrad: ops.upconv_plan keeps it on TNR_CONV_3x3_UP2 by default); the
tests ask for all three passes.  The fold exists in the bf16x3 arithmetic only, so these tests pin ops.MMA to it in both parametrisations of the suite;
test_present_launches_outside_the_policy runs the other arithmetics.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = torch.double
SLOPE = 0.2
ALPHA = 0.5
SHAPES = [(1, 16, 16, 64, 64), (2, 32, 40, 64, 64), (1, 17, 19, 64, 64), (1, 32, 32, 32, 32)]
IDS = ["tile16", "stream32x40", "odd17x19", "c32"]


def _engine(monkeypatch, bf16x3=True):
    from trainner_amd import engine, hip, ops
    if bf16x3:
        monkeypatch.setattr(ops, "FP32_MMA", hip.MMA_BF16X3)
        monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    return engine, hip, ops


@functools.lru_cache(maxsize=None)
def _case(shape, integers=False, slope=SLOPE):
    """Inputs (fp32, CPU) and the fp64 references of one layer; computed once, shared by the tests, never written."""
    N, H, W, Cin, Cout = shape
    gen = torch.Generator().manual_seed(1000 + 7 * H + W + Cin)
    if integers:
        rnd = lambda *s: torch.randint(-2, 3, s, generator=gen).float()
    else:
        rnd = lambda *s: torch.randn(*s, generator=gen)
    p = rnd(N, Cin, H, W)                                      # pre-activation of the layer's input
    w = rnd(Cout, Cin, 3, 3) * (1.0 if integers else (Cin * 9) ** -0.5)
    b = rnd(Cout)
    gz = rnd(N, Cout, 2 * H, 2 * W)                            # gradient of the layer's PRE-activation output
    dw0, db0 = rnd(Cout, Cin, 3, 3), rnd(Cout)                 # the gradients' non-zero start
    x = F.leaky_relu(p, slope)                                 # the layer's input as the engine reads it: an activation's fp32 output
    x64, w64, b64 = (t.to(D).requires_grad_(True) for t in (x, w, b))
    z = F.conv2d(F.interpolate(x64, scale_factor=2, mode="nearest"), w64, b64, padding=1)
    z.backward(gz.to(D))
    gate = torch.where(x64.detach() > 0, torch.ones_like(x64), torch.full_like(x64, slope)).detach()      # LeakyReLU' read from its output
    ref = dict(z=z.detach(), y=F.leaky_relu(z.detach(), slope), gx=x64.grad, gp=x64.grad * gate,
               dw=dw0.to(D) + ALPHA * w64.grad, db=db0.to(D) + ALPHA * b64.grad)
    return dict(x=x, w=w, b=b, gz=gz, dw0=dw0, db0=db0, ref=ref)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _nchw(buf):
    return buf.permute(0, 3, 1, 2).double().cpu()


def _layer(engine, ops, c, shape):
    from trainner_amd.models.modules.architectures.block import Conv2dHIP
    N, H, W, Cin, Cout = shape
    mod = Conv2dHIP(Cin, Cout, 3, 1).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(c["w"])
        mod.bias.copy_(c["b"])
    packer = ops.WeightPacker(torch.device(DEV))
    op = engine.ConvOp(mod, packer, ups=True)
    packer.run()
    return mod, op


def _run(monkeypatch, ops, engine, c, shape, fold, what, act=True, mask=True, slope=SLOPE):
    """One pass of the engine's layer, folded or not -> the result as fp64 NCHW on the CPU (dict for the weight pass)."""
    N, H, W, Cin, Cout = shape
    monkeypatch.setenv("TNR_UPCONV_FOLD", "fwd,dgrad,wgrad" if fold else "0")
    mod, op = _layer(engine, ops, c, shape)
    x = ops.View(_nhwc(c["x"]))
    if what == "fwd":
        y = ops.View(torch.full((N, 2 * H, 2 * W, Cout), float("nan"), device=DEV))
        op.fwd_up2(x, y, **(dict(act=ops.ACT_LRELU, slope=slope) if act else {}))
        return _nchw(y.buf)
    g = ops.View(_nhwc(c["gz"]))
    if what == "dgrad":
        gx = ops.View(torch.full((N, H, W, Cin), float("nan"), device=DEV))
        op.dgrad_up2(g, gx, mask=x if mask else None, m_slope=slope)
        return _nchw(gx.buf)
    mod.weight.grad = c["dw0"].to(DEV).clone()
    mod.bias.grad = c["db0"].to(DEV).clone()
    op.wgrad(x, g, alpha=ALPHA)
    return dict(dw=mod.weight.grad.double().cpu(), db=mod.bias.grad.double().cpu())


def _held(name, got, direct, ref):
    e_f, e_d, scale = float((got - ref).abs().max()), float((direct - ref).abs().max()), float(ref.abs().max())
    rms_f, rms_d = float((got - ref).pow(2).mean().sqrt()), float((direct - ref).pow(2).mean().sqrt())
    print("%s: max err folded %.3e direct %.3e (ratio %.2f), rms %.3e / %.3e, scale %.3e" % (name, e_f, e_d, e_f / max(e_d, 1e-30), rms_f, rms_d, scale))
    assert e_f <= 3.0 * e_d + 2e-7 * scale, (name, e_f, e_d, scale)


@pytest.mark.parametrize("act", [True, False], ids=["bias_lrelu", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_error_vs_fp64(shape, act, monkeypatch):
    engine, hip, ops = _engine(monkeypatch)
    c = _case(shape)
    ref = c["ref"]["y" if act else "z"]
    got, direct = (_run(monkeypatch, ops, engine, c, shape, fold, "fwd", act=act) for fold in (True, False))
    _held("forward", got, direct, ref)


@pytest.mark.parametrize("mask", [True, False], ids=["mask", "plain"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_data_gradient_error_vs_fp64(shape, mask, monkeypatch):
    engine, hip, ops = _engine(monkeypatch)
    c = _case(shape)
    ref = c["ref"]["gp" if mask else "gx"]
    got, direct = (_run(monkeypatch, ops, engine, c, shape, fold, "dgrad", mask=mask) for fold in (True, False))
    _held("data gradient", got, direct, ref)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weight_and_bias_gradient_error_vs_fp64(shape, monkeypatch):
    engine, hip, ops = _engine(monkeypatch)
    c = _case(shape)
    got, direct = (_run(monkeypatch, ops, engine, c, shape, fold, "wgrad") for fold in (True, False))
    _held("weight gradient", got["dw"], direct["dw"], c["ref"]["dw"])
    _held("bias gradient", got["db"], direct["db"], c["ref"]["db"])


def test_integer_case_is_exact(monkeypatch):
    """Small-integer weights and inputs, slopes of 0.5, alpha = 0.5: the fold, every product and every sum are exact in fp32, so all
    three folded passes equal the fp64 reference bit for bit (stream kernels, ragged last tile)."""
    engine, hip, ops = _engine(monkeypatch)
    shape = (1, 32, 40, 64, 64)
    c = _case(shape, True, 0.5)
    r = c["ref"]
    assert torch.equal(_run(monkeypatch, ops, engine, c, shape, True, "fwd", act=True, slope=0.5), r["y"])
    assert torch.equal(_run(monkeypatch, ops, engine, c, shape, True, "fwd", act=False), r["z"])
    assert torch.equal(_run(monkeypatch, ops, engine, c, shape, True, "dgrad", mask=True, slope=0.5), r["gp"])
    assert torch.equal(_run(monkeypatch, ops, engine, c, shape, True, "dgrad", mask=False), r["gx"])
    got = _run(monkeypatch, ops, engine, c, shape, True, "wgrad")
    assert torch.equal(got["dw"], r["dw"]) and torch.equal(got["db"], r["db"])


def _families(monkeypatch, ops, engine, shape):
    """The PROFILE families (and the tnr_upsample2x_bwd calls) of the three passes of one layer under the current settings."""
    c = _case(shape)
    calls = []
    real = ops.upsample2x_bwd
    monkeypatch.setattr(ops, "upsample2x_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    N, H, W, Cin, Cout = shape
    mod, op = _layer(engine, ops, c, shape)
    mod.weight.grad, mod.bias.grad = c["dw0"].to(DEV).clone(), c["db0"].to(DEV).clone()
    x, g = ops.View(_nhwc(c["x"])), ops.View(_nhwc(c["gz"]))
    y, gx = ops.View(torch.empty((N, 2 * H, 2 * W, Cout), device=DEV)), ops.View(torch.empty((N, H, W, Cin), device=DEV))
    monkeypatch.setattr(ops, "PROFILE", ops.ConvProfile())
    op.fwd_up2(x, y, act=ops.ACT_LRELU, slope=SLOPE)
    op.dgrad_up2(g, gx, mask=x, m_slope=SLOPE)
    op.wgrad(x, g)
    fam = {k: v["launches"] for k, v in ops.PROFILE.summary().items()}
    return fam, len(calls)


def test_present_launches_outside_the_policy(monkeypatch):
    """TNR_MMA=f32, `use_amp` (bf16 operands) and TNR_UPCONV_FOLD=0 keep the present launches; the default folds the two gradient passes
    and keeps the forward on TNR_CONV_3x3_UP2; the list of all three folds them all into the family of their own, counted with the FLOP
    they execute."""
    engine, hip, ops = _engine(monkeypatch, bf16x3=False)
    shape = (2, 32, 40, 64, 64)
    present = [(hip.MMA_F32, "1"), (hip.MMA_BF16, "1"), (hip.MMA_BF16X3, "0")]
    for mma, switch in present:
        monkeypatch.setattr(ops, "MMA", mma)
        monkeypatch.setenv("TNR_UPCONV_FOLD", switch)
        fam, ups_bwd = _families(monkeypatch, ops, engine, shape)
        assert ops.UPFOLD_FAMILY not in fam and fam.get("conv_tile_3x3_up2") == 1 and fam.get("wgrad_tile") == 1 and ups_bwd == 1, (mma, switch, fam)
        assert fam.get("conv_tile_3x3", 0) + fam.get("conv_wino_3x3", 0) == 1, (mma, switch, fam)
    monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    monkeypatch.setenv("TNR_UPCONV_FOLD", "1")
    fam, ups_bwd = _families(monkeypatch, ops, engine, shape)
    assert fam == {ops.UPFOLD_FAMILY: 2, "conv_tile_3x3_up2": 1} and ups_bwd == 0, fam
    monkeypatch.setenv("TNR_UPCONV_FOLD", "fwd,dgrad,wgrad")
    fam, ups_bwd = _families(monkeypatch, ops, engine, shape)
    assert fam == {ops.UPFOLD_FAMILY: 3} and ups_bwd == 0, fam
    N, H, W, Cin, Cout = shape
    flops = ops.PROFILE.summary()[ops.UPFOLD_FAMILY]["flops"]
    assert flops == 3 * 2.0 * N * H * W * 16 * Cin * Cout, flops
