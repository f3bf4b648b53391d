"""The image-to-image decoders' up-conv layer on the device (-m gpu): tnr_upconv_i2i_fwd / _dgrad / _wgrad against
F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1) and its autograd gradients in fp64, and the two generators with
upsample_mode="upconv" against torch fp64 modules of the same structure (nn.Upsample + nn.Conv2d) loaded with the engine's state_dict.

Kernel level, N = 2: Cin = Cout, 2 Cout and 4 Cout; 1 x 1 (every neighbour is padding) and 1 x 2 under 1024 -> 512 channels (the weight-bound
end: one active wave, 32-channel row blocks), sizes below one 8 x 16 tile, and 9 x 17 (four tiles, none of them full); with and without bias.
Bound: the project's rule for its matrix-core convolutions, err <= 1.5 x err(the same statement in fp32 on the CPU) + 2e-7 x max |ref|, both
against fp64, over every element, in both TNR_MMA modes.  The weight gradient runs twice, with equal bits."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import test_gpu_kernels as K
import test_gpu_membound_kernels as M
from oracle import detrand
from test_gpu_nets import rel_err, robust_err, seeded, to64

gpu = pytest.mark.gpu
NAN = float("nan")
# Cin, Cout, H, W of the LR tensor, bias
CASES = [(128, 64, 5, 7, True), (256, 128, 3, 3, False), (64, 64, 1, 1, True), (1024, 512, 1, 2, False), (512, 256, 2, 2, True),
         (128, 32, 9, 4, False), (64, 32, 9, 17, True)]
case_id = lambda c: "%dto%d-%dx%d-%s" % (c[:4] + ("bias" if c[4] else "nobias",))


def layer(x, w, b):
    return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, b, padding=1)


@functools.lru_cache(maxsize=None)
def case(c):
    """x, w, b, g and (y, gx, dW) in fp64 and in torch's fp32"""
    cin, cout, H, W, bias = c
    x, w = K.rnd(2, cin, H, W, seed=5100), K.rnd(cout, cin, 3, 3, seed=5101, lo=-0.1, hi=0.1)
    b, g = K.rnd(cout, seed=5102) if bias else None, K.rnd(2, cout, 2 * H, 2 * W, seed=5103)
    out = {}
    for dt in (torch.double, torch.float32):
        xr, wr = x.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        y = layer(xr, wr, None if b is None else b.to(dt))
        out[dt] = (y.detach(),) + torch.autograd.grad(y, (xr, wr), g.to(dt))
    return x, w, b, g, out[torch.double], out[torch.float32]


def held(what, got, r64, r32):
    scale = float(r64.abs().max())
    e_dev, e_32 = float((got.double() - r64.to(got.device)).abs().max()), float((r32.double() - r64).abs().max())
    bound = 1.5 * e_32 + 2e-7 * scale
    print("UPCONV-I2I %-44s dev %.3e  torch-fp32 %.3e  scale %.3e  dev/bound %.3f" % (what, e_dev, e_32, scale, e_dev / bound))
    assert e_dev <= bound, (what, e_dev, e_32, scale)


def packed(ops, w):
    wts = ops.UpconvI2IWeights(w.to(K.DEV))
    wts.pack()
    return wts


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forward(c, mma_mode):
    from trainner_amd import ops
    x, w, b, _, r64, r32 = case(c)
    yv = M.blank(2, 2 * c[2], 2 * c[3], c[1], 8, inner=NAN)
    ops.upconv_i2i_fwd(M.win(x, 4), packed(ops, w), yv, bias=None if b is None else b.to(K.DEV))
    torch.cuda.synchronize()
    M.outside_untouched(yv)
    held("fwd %s %s" % (case_id(c), mma_mode), M.got(yv), r64[0], r32[0])


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_data_gradient(c, mma_mode):
    from trainner_amd import ops
    x, w, _, g, r64, r32 = case(c)
    gxv = M.blank(2, c[2], c[3], c[0], 8, inner=NAN)
    ops.upconv_i2i_dgrad(M.win(g, 4), packed(ops, w), gxv)
    torch.cuda.synchronize()
    M.outside_untouched(gxv)
    held("dgrad %s %s" % (case_id(c), mma_mode), M.got(gxv), r64[1], r32[1])


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_weight_gradient(c, mma_mode):
    from trainner_amd import ops
    x, _, _, g, r64, r32 = case(c)
    xv, gv = M.win(x, 4), M.win(g, 8)
    runs = []
    for _rep in range(2):
        dw = torch.full((c[1], c[0], 3, 3), NAN, device=K.DEV)
        ops.upconv_i2i_wgrad(xv, gv, dw, None, alpha=1.0, beta=0.0)
        torch.cuda.synchronize()
        runs.append(dw)
    assert torch.equal(runs[0], runs[1]), "two launches differ"
    held("dW %s %s" % (case_id(c), mma_mode), runs[0], r64[2], r32[2])


# ---------------------------------------------------------------------------------------------------------------------
# the generators: torch modules of the reference's structure, fp64
# ---------------------------------------------------------------------------------------------------------------------
def up(cin, cout, bias):
    return nn.Sequential(nn.Upsample(scale_factor=2, mode="nearest"), nn.Conv2d(cin, cout, 3, 1, 1, bias=bias))


class ResBlock(nn.Module):
    def __init__(self, d):
        super().__init__()
        half = lambda: [nn.ReflectionPad2d(1), nn.Conv2d(d, d, 3), nn.InstanceNorm2d(d)]
        self.conv_block = nn.Sequential(*half(), nn.ReLU(True), *half())

    def forward(self, x):
        return x + self.conv_block(x)


class TorchResnet(nn.Module):
    def __init__(self, ngf, nb):
        super().__init__()
        IN, act = nn.InstanceNorm2d, lambda: nn.ReLU(True)
        m = [nn.ReflectionPad2d(3), nn.Conv2d(3, ngf, 7), IN(ngf), act()]
        for c in (ngf, 2 * ngf):
            m += [nn.Conv2d(c, 2 * c, 3, 2, 1), IN(2 * c), act()]
        m += [ResBlock(4 * ngf) for _ in range(nb)]
        for c in (4 * ngf, 2 * ngf):
            m += [up(c, c // 2, True), IN(c // 2), act()]
        self.model = nn.Sequential(*m, nn.ReflectionPad2d(3), nn.Conv2d(ngf, 3, 7), nn.Tanh())

    def forward(self, x):
        return self.model(x)


class UBlock(nn.Module):
    def __init__(self, outer, inner, inp=None, sub=None, outermost=False, innermost=False):
        super().__init__()
        self.outermost = outermost
        down, BN = nn.Conv2d(outer if inp is None else inp, inner, 4, 2, 1, bias=False), nn.BatchNorm2d
        if outermost:
            m = [down, sub, nn.ReLU(True), up(2 * inner, outer, True), nn.Tanh()]
        elif innermost:
            m = [nn.LeakyReLU(0.2, True), down, nn.ReLU(True), up(inner, outer, False), BN(outer)]
        else:
            m = [nn.LeakyReLU(0.2, True), down, BN(inner), sub, nn.ReLU(True), up(2 * inner, outer, False), BN(outer)]
        self.model = nn.Sequential(*m)

    def forward(self, x):
        return self.model(x) if self.outermost else torch.cat([x, self.model(x)], 1)


class TorchUnet5(nn.Module):
    def __init__(self, ngf):
        super().__init__()
        blk = UBlock(8 * ngf, 8 * ngf, innermost=True)
        for outer in (4 * ngf, 2 * ngf, ngf):
            blk = UBlock(outer, 2 * outer, sub=blk)
        self.model = UBlock(3, ngf, inp=3, sub=blk, outermost=True)

    def forward(self, x):
        return self.model(x)


def against_torch(net, ref, size, seed, zero_grad_bias):
    """output, input gradient and every parameter gradient of the engine's `net` against `ref` (fp64, the engine's state_dict); bounds of test_gpu_nets"""
    sd = seeded(net, seed, gain=0.5)
    ref = ref.double().train()
    ref.load_state_dict(to64(sd))
    net = net.to(K.DEV).train()
    x, gout = detrand.uniform((2, 3) + size, seed + 1, -1.0, 1.0), detrand.uniform((2, 3) + size, seed + 2, -1.0, 1.0)
    xd, xr = x.to(K.DEV).requires_grad_(True), x.double().requires_grad_(True)
    out = net(xd)
    out.backward(gout.to(K.DEV))
    want = ref(xr)
    want.backward(gout.double())
    assert out.shape == want.shape and rel_err(out, want) < 5e-5
    l2, med = robust_err(xd.grad, xr.grad)          # (CycleGAN chains two generators; ReLU gates: bounded like test_gpu_nets)
    assert l2 < 2e-2 and med < 2e-5, (l2, med)
    rp = dict(ref.named_parameters())
    for k, p in net.named_parameters():
        if zero_grad_bias(k):
            continue          # a conv bias in front of an InstanceNorm has an exactly-zero true gradient: noise on both sides
        l2, med = robust_err(p.grad, rp[k].grad)
        assert l2 < 2e-2 and med < 5e-5, (k, l2, med)


@gpu
def test_resnet_generator_upconv():
    from trainner_amd.models.modules.architectures.ResNet_arch import ResnetGenerator
    net = ResnetGenerator(3, 3, 32, norm_type="instance", n_blocks=1, upsample_mode="upconv")
    against_torch(net, TorchResnet(32, 1), (16, 16), 61, lambda k: k.endswith(".bias") and k != "model.18.bias")


@gpu
def test_unet_generator_upconv():
    from trainner_amd.models.modules.architectures.UNet_arch import UnetGenerator
    net = UnetGenerator(3, 3, 5, ngf=16, upsample_mode="upconv")
    against_torch(net, TorchUnet5(16), (32, 32), 71, lambda k: False)
