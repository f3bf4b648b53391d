"""The pixel-unshuffle generator input on the device (-m gpu): tnr_conv_unshuffle_fwd / tnr_wgrad_unshuffle against
F.conv2d(F.pixel_unshuffle(x, s), w, b, padding=1) in fp64, RRDBNet(12 | 48, ...) against the oracle, and an x2 `use_unshuffle` SR step.

Kernel level.  Output sizes 1 x 1 (every tap but the centre is padding), 1 x 19, an odd grid of several tiles (17 x 23 at s = 2, 9 x 19 at
s = 4) and one 8 x 16 workgroup tile plus one pixel in each direction, for s in {2, 4} and nf in {32, 64}.  The image's pad channel holds a
finite non-zero sentinel.  Bound: the project's rule for these layers (test_gpu_membound_kernels.yardstick: device error <= 2 x the error of
torch's fp32 statement of the same expression + 2e-7 x max |ref|, both against fp64; the bf16 form from the bf16-rounded x and w), over
every element.  The weight gradient runs with alpha = 0.75 and beta = 1 onto non-zero dW / db, twice, with equal bits."""
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
PAD_SENT, ALPHA = 7.5, 0.75
SHAPES = {2: {"px1": (1, 1, 1), "line": (1, 1, 19), "odd": (2, 17, 23), "tile+1": (2, 9, 17)},          # N, Ho, Wo
          4: {"px1": (1, 1, 1), "line": (1, 1, 19), "odd": (2, 9, 19), "tile+1": (2, 9, 17)}}
CASES = [(s, nf, cls) for s in (2, 4) for nf in (32, 64) for cls in SHAPES[s]]
case_id = lambda c: "s%d-nf%d-%s" % c


@functools.lru_cache(maxsize=None)
def case(s, nf, cls, rounded):
    """x, w, b, g, dw0, db0 and, in fp64 / torch's fp32: y, dw0 + ALPHA dW, db0 + ALPHA db"""
    N, Ho, Wo = SHAPES[s][cls]
    x, w, b = K.rnd(N, 3, Ho * s, Wo * s, seed=4100 + s), K.rnd(nf, 3 * s * s, 3, 3, seed=4101 + s, lo=-0.2, hi=0.2), K.rnd(nf, seed=4102)
    g, dw0, db0 = K.rnd(N, nf, Ho, Wo, seed=4103), K.rnd(nf, 3 * s * s, 3, 3, seed=4104), K.rnd(nf, seed=4105)
    out = {}
    for dt in (torch.double, torch.float32):
        xr, wr = ((t.bfloat16().float() if rounded else t).to(dt) for t in (x, w))
        wr.requires_grad_(True)
        br = b.to(dt).requires_grad_(True)
        y = F.conv2d(F.pixel_unshuffle(xr, s), wr, br, padding=1)
        gw, gb = torch.autograd.grad(y, (wr, br), g.to(dt))
        out[dt] = (y.detach(), dw0.to(dt) + ALPHA * gw, db0.to(dt) + ALPHA * gb)
    return x, w, b, g, dw0, db0, out[torch.double], out[torch.float32]


def image4(x):
    return K.nhwc_buf(x, ctot=4, fill=PAD_SENT)


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_forward(c, mma_mode, monkeypatch):
    from trainner_amd import ops
    s, nf, cls = c
    for arith in [mma_mode] + (["bf16"] if mma_mode == "bf16x3" else []):
        monkeypatch.setattr(ops, "MMA", ARITH[arith])
        x, w, b, _, _, _, r64, r32 = case(s, nf, cls, arith == "bf16")
        x4 = image4(x)
        snap = x4.clone()
        wp, _keep = K.pack(ops, w.to(K.DEV), ops.PACK_UNSHUFFLE_FWD)
        yv = M.blank(x.shape[0], r64[0].shape[2], r64[0].shape[3], nf, 8, inner=NAN)
        ops.conv_unshuffle(ops.View(x4), wp, yv, s, bias=b.to(K.DEV))
        torch.cuda.synchronize()
        outside = torch.ones(yv.ctot, dtype=torch.bool, device=K.DEV)
        outside[8:8 + nf] = False
        assert same_bits(yv.buf[..., outside], torch.full_like(yv.buf[..., outside], M.SENT)) and same_bits(x4, snap)
        M.yardstick("unshuffle fwd %s %s" % (case_id(c), arith), M.got(yv), r64[0], r32[0])


@gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_weight_gradient(c):
    from trainner_amd import ops
    s, nf, cls = c
    x, _, _, g, dw0, db0, r64, r32 = case(s, nf, cls, False)
    x4, gv = image4(x), M.win(g, 8)
    runs = []
    for rep_ in range(2):
        dw, db = dw0.to(K.DEV), db0.to(K.DEV)
        ops.wgrad_unshuffle(gv, ops.View(x4), dw, db, s, alpha=ALPHA, beta=1.0)
        torch.cuda.synchronize()
        runs.append((dw, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "two launches differ"
    M.yardstick("unshuffle dW %s" % case_id(c), runs[0][0], r64[1], r32[1])
    M.yardstick("unshuffle db %s" % case_id(c), runs[0][1], r64[2], r32[2])


@gpu
@pytest.mark.parametrize("s", [2, 4])
def test_network(s):
    """RRDBNet(3 s^2, 3, 32, 1) through block.SpaceToDepth's handle against the fp64 oracle over the unshuffled image; bounds of test_gpu_nets"""
    from trainner_amd.models.modules.architectures import block as B
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    net = RRDBNet(3 * s * s, 3, 32, 1, upscale=4)
    sd = seeded(net, 7)
    assert tuple(sd["model.0.weight"].shape) == (32, 3 * s * s, 3, 3)
    net = net.to(K.DEV)
    lr = detrand.uniform((2, 3, 10 * s, 18 * s), 3, 0.0, 1.0)          # trunk 10 x 18: two tiles each way
    gout = detrand.uniform((2, 3, 40, 72), 4, -1.0, 1.0)
    out = net(B.SpaceToDepth(s)(lr.to(K.DEV)))
    out.backward(gout.to(K.DEV))
    osd = oracle_params(to64(sd))
    ref = O.rrdbnet_forward(F.pixel_unshuffle(lr.double(), s), osd, 1)
    ref.backward(gout.double())
    assert out.shape == ref.shape and rel_err(out, ref) < 2e-5
    for k in ("model.0.weight", "model.0.bias"):
        assert rel_err(dict(net.named_parameters())[k].grad, osd[k].grad) < 2e-4, k


@gpu
def test_model_steps_and_validates(tmp_path):
    """scale 2 + use_unshuffle over the x4 esrgan net: two optimize_parameters steps, test() on a 32 x 32 input"""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = ref_harness.esrgan_yaml(name="unshuffle_case", out_root=str(tmp_path), gpu_ids="[0]", nb=1, nf=32, batch=2, crop=64, d_nf=16)
    with open(yml) as fh:
        txt = fh.read()
    assert "\nscale: 4\n" in txt and "  type: esrgan\n" in txt
    with open(yml, "w") as fh:
        fh.write(txt.replace("\nscale: 4\n", "\nscale: 2\nuse_unshuffle: true\n").replace("  type: esrgan\n", "  type: esrgan\n  scale: 4\n"))
    opt = options.parse(yml, is_train=True)
    assert opt["unshuffle_scale"] == 2 and opt["network_G"]["in_nc"] == 12 and opt["network_G"]["upscale"] == 4
    model = create_model(opt, verbose=False)
    assert model.unshuffle is not None and model.unshuffle.bs == 2
    w0 = model.netG.state_dict()["model.0.weight"].clone()
    assert tuple(w0.shape) == (32, 12, 3, 3)
    for step in (1, 2):
        model.feed_data({"LR": detrand.uniform((2, 3, 32, 32), 40 + step, 0.0, 1.0), "HR": detrand.uniform((2, 3, 64, 64), 50 + step, 0.0, 1.0)})
        model.optimize_parameters(step)
        log = model.get_current_log()
        assert log and all(v == v and abs(v) != float("inf") for v in log.values()), log
    assert not torch.equal(model.netG.state_dict()["model.0.weight"], w0)
    model.feed_data({"LR": detrand.uniform((1, 3, 32, 32), 60, 0.0, 1.0)}, need_HR=False)
    model.test()
    assert tuple(model.fake_H.shape) == (1, 3, 64, 64) and bool(torch.isfinite(model.fake_H).all())
