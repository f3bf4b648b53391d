"""RRDBNet's x3 up-conv layer on the device (-m gpu): tnr_upconv3_fwd / _dgrad / _wgrad against
leaky_relu(F.conv2d(F.interpolate(x, scale_factor=3, mode="nearest"), w, b, padding=1), 0.2) and its autograd.grad in fp64, RRDBNet(upscale=3)
against the oracle's trunk + that tail, and a `scale: 3` SR step.

Kernel level.  LR sizes 1 x 1 (every neighbour is padding), 1 x 19, an odd grid of several tiles (17 x 23) and one 8 x 16 workgroup tile plus
one pixel each way, for nf in {32, 64}.  Bound: the project's rule for these layers (test_gpu_membound_kernels.yardstick: device error <= 2 x
the error of torch's fp32 statement of the same expression + 2e-7 x max |ref|, both against fp64), over every element; the bf16 form from
the bf16-rounded x (g) and the bf16-rounded FOLDED taps.  The weight gradient runs with alpha = 0.75 and beta = 1 onto non-zero dW / db,
twice, with equal bits."""
import functools

import pytest
import torch
import torch.nn.functional as F

import test_gpu_kernels as K
import test_gpu_membound_kernels as M
from oracle import detrand, ref_harness, sr_oracle as O
from test_gpu_conv_edges import ARITH, NAN, same_bits
from test_gpu_nets import oracle_params, rel_err, seeded, to64

gpu = pytest.mark.gpu
ALPHA = 0.75
SHAPES = {"px1": (1, 1, 1), "line": (1, 1, 19), "odd": (2, 17, 23), "tile+1": (2, 9, 17)}          # N, H, W of the LR tensor
CASES = [(nf, cls) for nf in (32, 64) for cls in SHAPES]
case_id = lambda c: "nf%d-%s" % c
T3 = ((2,), (1, 2), (0, 1, 2), (0, 1), (0,))          # the issue's table: 3x3 taps summed into folded tap k, per axis


def layer(x, w, b):
    return F.conv2d(F.interpolate(x, scale_factor=3, mode="nearest"), w, b, padding=1)


@functools.lru_cache(maxsize=None)
def case(nf, cls, rounded):
    """x, w, b, g, m, dw0, db0 and, in fp64 / torch's fp32: y, gx, gx * LeakyReLU'(m), dw0 + ALPHA dW, db0 + ALPHA db"""
    from trainner_amd import ops
    N, H, W = SHAPES[cls]
    x, w, b = K.rnd(N, nf, H, W, seed=4300), K.rnd(nf, nf, 3, 3, seed=4301, lo=-0.1, hi=0.1), K.rnd(nf, seed=4302)
    g, m = K.rnd(N, nf, 3 * H, 3 * W, seed=4303), K.rnd(N, nf, H, W, seed=4304)
    dw0, db0 = K.rnd(nf, nf, 3, 3, seed=4305), K.rnd(nf, seed=4306)
    out = {}
    for dt in (torch.double, torch.float32):
        xr, br, wr = x.to(dt).requires_grad_(True), b.to(dt).requires_grad_(True), w.to(dt).requires_grad_(True)
        if rounded:      # what the bf16 matrix core is handed: bf16(x) | bf16(g) and the bf16 rounding of the folded taps
            kf = ops.upconv3_fold_weights(w).bfloat16().to(dt).transpose(0, 1)
            z = F.conv_transpose2d(x.bfloat16().to(dt), kf, br, stride=3, padding=1)
            zg = F.conv_transpose2d(xr, kf, None, stride=3, padding=1)
            gx, = torch.autograd.grad(zg, xr, g.bfloat16().to(dt))
            gw = gb = torch.zeros(())
        else:
            z = layer(xr, wr, br)
            gx, gw, gb = torch.autograd.grad(z, (xr, wr, br), g.to(dt))
        gm = gx * torch.where(m > 0, 1.0, 0.2).to(dt)
        out[dt] = (F.leaky_relu(z, 0.2).detach(), gx, gm, dw0.to(dt) + ALPHA * gw, db0.to(dt) + ALPHA * gb)
    return x, w, b, g, m, dw0, db0, out[torch.double], out[torch.float32]


def ariths(mma_mode):
    return [mma_mode] + (["bf16"] if mma_mode == "bf16x3" else [])


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forward(c, mma_mode, monkeypatch):
    from trainner_amd import ops
    for arith in ariths(mma_mode):
        monkeypatch.setattr(ops, "MMA", ARITH[arith])
        x, w, b, _, _, _, _, r64, r32 = case(*c, arith == "bf16")
        xv = M.win(x, 4)
        snap = xv.buf.clone()
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_UP3_FWD)
        yv = M.blank(x.shape[0], 3 * x.shape[2], 3 * x.shape[3], c[0], 8, inner=NAN)
        ops.upconv3_fwd(xv, wp, yv, bias=b.to(K.DEV), act=ops.ACT_LRELU, slope=0.2)
        torch.cuda.synchronize()
        outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
        outside[8:8 + c[0]] = False
        assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT)) and same_bits(xv.buf, snap)
        M.yardstick("upconv3 fwd %s %s" % (case_id(c), arith), M.got(yv), r64[0], r32[0])


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "mask"])
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_data_gradient(c, masked, mma_mode, monkeypatch):
    from trainner_amd import ops
    for arith in ariths(mma_mode):
        monkeypatch.setattr(ops, "MMA", ARITH[arith])
        x, w, _, g, m, _, _, r64, r32 = case(*c, arith == "bf16")
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_UP3_DGRAD)
        gxv = M.blank(x.shape[0], x.shape[2], x.shape[3], c[0], 8, inner=NAN)
        ops.upconv3_dgrad(M.win(g, 4), wp, gxv, mask=M.win(m, 8) if masked else None, m_slope=0.2)
        torch.cuda.synchronize()
        M.yardstick("upconv3 dgrad %s %s %s" % (case_id(c), arith, masked), M.got(gxv), r64[1 + masked], r32[1 + masked])


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_weight_gradient(c):
    from trainner_amd import ops
    x, _, _, g, _, dw0, db0, r64, r32 = case(*c, False)
    xv, gv = M.win(x, 4), M.win(g, 8)
    runs = []
    for rep_ in range(2):
        dw, db = dw0.to(K.DEV), db0.to(K.DEV)
        ops.upconv3_wgrad(xv, gv, dw, db, alpha=ALPHA, beta=1.0)
        torch.cuda.synchronize()
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    M.yardstick("upconv3 dW %s" % case_id(c), runs[0][0], r64[3], r32[3])
    M.yardstick("upconv3 db %s" % case_id(c), runs[0][1], r64[4], r32[4])


@gpu
def test_fold_table():
    from trainner_amd import ops
    want = torch.tensor([[float(ty in T3[ky] and tx in T3[kx]) for ty in range(3) for tx in range(3)] for ky in range(5) for kx in range(5)],
                        dtype=torch.double)
    assert torch.equal(ops.upconv3_fold_table(), want)
    assert torch.equal(ops.upconv3_unfold_grad(torch.eye(25, dtype=torch.double).view(25, 5, 5)).view(25, 9), want)      # row k: d tap / d dK[k]
    assert torch.equal(ops.upconv3_fold_weights(torch.eye(9, dtype=torch.double).view(9, 3, 3)).view(9, 25), want.t())


@gpu
def test_network():
    """RRDBNet(3, 3, 32, 1, upscale=3) against the fp64 oracle: its trunk from sr_oracle, the x3 tail stated here; bounds of test_gpu_unshuffle"""
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    net = RRDBNet(3, 3, 32, 1, upscale=3)
    sd = seeded(net, 7)
    net = net.to(K.DEV)
    lr = detrand.uniform((2, 3, 10, 18), 3, 0.0, 1.0)
    gout = detrand.uniform((2, 3, 30, 54), 4, -1.0, 1.0)
    out = net(lr.to(K.DEV))
    out.backward(gout.to(K.DEV))
    osd = oracle_params(to64(sd))
    conv = lambda t, k: F.conv2d(t, osd[k + ".weight"], osd[k + ".bias"], padding=1)
    fea = conv(lr.double(), "model.0")
    y = fea + conv(O.rrdb_forward(fea, osd, "model.1.sub.0"), "model.1.sub.1")
    y = F.leaky_relu(conv(F.interpolate(y, scale_factor=3, mode="nearest"), "model.3"), 0.2)
    ref = conv(F.leaky_relu(conv(y, "model.5"), 0.2), "model.7")
    ref.backward(gout.double())
    assert out.shape == ref.shape and rel_err(out, ref) < 2e-5
    for k in ("model.3.weight", "model.3.bias", "model.0.weight"):
        assert rel_err(dict(net.named_parameters())[k].grad, osd[k].grad) < 2e-4, k


@gpu
def test_model_steps_and_validates(tmp_path):
    """scale 3 over the esrgan recipe: two optimize_parameters steps, test() on a 32 x 32 input"""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="upconv3_case", out_root=str(tmp_path), gpu_ids="[0]", nb=1, nf=32, batch=2, crop=96, d_nf=16)
    with open(yml) as fh:
        txt = fh.read()
    assert "\nscale: 4\n" in txt
    with open(yml, "w") as fh:
        fh.write(txt.replace("\nscale: 4\n", "\nscale: 3\n"))
    opt = options.parse(yml, is_train=True)
    assert opt["network_G"]["upscale"] == 3
    model = create_model(opt, verbose=False)
    w0 = model.netG.state_dict()["model.3.weight"].clone()
    for step in (1, 2):
        model.feed_data({"LR": detrand.uniform((2, 3, 32, 32), 40 + step, 0.0, 1.0), "HR": detrand.uniform((2, 3, 96, 96), 50 + step, 0.0, 1.0)})
        model.optimize_parameters(step)
        log = model.get_current_log()
        assert log and all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert not torch.equal(model.netG.state_dict()["model.3.weight"], w0)
    model.feed_data({"LR": detrand.uniform((1, 3, 32, 32), 60, 0.0, 1.0)}, need_HR=False)
    model.test()
    assert tuple(model.fake_H.shape) == (1, 3, 96, 96) and bool(torch.isfinite(model.fake_H).all())
