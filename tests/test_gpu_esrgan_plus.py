"""ESRGAN+ residual paths (network_G `plus: true`) on the device (-m gpu): the weight-space fold and its adjoint (csrc/dense_plus.hip)
against fp64 with bounds derived from the fp32 FMA chains they run, and RRDBNet(plus=True) -- forward, every parameter gradient,
accumulation, the no-grad path -- against a plain-torch fp64 restatement of ResidualDenseBlock_5C.forward (RRDBNet_arch.py:150-163)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import detrand, sr_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24          # fp32 unit round-off


def _blocks(nf, gc, n, seed):
    """n blocks of (P, W3, W4, W5) with gradients: real values and real gradients from detrand, on the device."""
    shapes = [(gc, nf, 1, 1)] + [(gc if k < 5 else nf, nf + (k - 1) * gc, 3, 3) for k in (3, 4, 5)]
    out = []
    for b in range(n):
        row = []
        for i, s in enumerate(shapes):
            t = detrand.uniform(s, seed + 10 * b + i, -0.5, 0.5).to(DEV)
            t.grad = detrand.uniform(s, seed + 500 + 10 * b + i, -1.0, 1.0).to(DEV)
            row.append(t)
        out.append(row)
    return out


@pytest.mark.parametrize("nf,n", [(64, 1), (64, 3), (32, 1), (32, 3)])
def test_fold_and_unfold_against_fp64(nf, n):
    from trainner_amd import ops
    gc, x2, x4 = 32, nf + 32, nf + 96
    blocks = _blocks(nf, gc, n, 7 * nf + n)
    dp = ops.DensePlus(blocks, nf, gc, torch.device(DEV))
    dp.fold()
    for i, e in enumerate(e for row in dp.eff for e in row):          # this backward's gradient w.r.t. the effective weights
        e.grad.copy_(detrand.uniform(e.shape, 900 + i, -1.0, 1.0))
    before = [[t.grad.double().cpu() for t in row] for row in blocks]
    dp.unfold(0, n)
    first = [[t.grad.clone() for t in row] for row in blocks]
    for row, old in zip(blocks, before):                  # the same inputs once more: bit-identical (fixed reduction order)
        for t, o in zip(row, old):
            t.grad.copy_(o)
    dp.unfold(0, n)
    for (p, *ws), effs, old, got1 in zip(blocks, dp.eff, before, first):
        P, dP, bP = p.double().cpu()[:, :, 0, 0], 0.0, 0.0
        for L, (w, e) in enumerate(zip(ws, effs)):
            W, E, G, D = w.double().cpu(), e.double().cpu(), e.grad.double().cpu(), w.grad.double().cpu()
            A = W[:, x2:x2 + gc] + (W[:, x4:x4 + gc] if L == 2 else 0.0)
            absA = W[:, x2:x2 + gc].abs() + (W[:, x4:x4 + gc].abs() if L == 2 else 0.0)
            # fold: a chain of gc FMAs from the original value (+ one addition forming conv5's A)
            ref = W.clone()
            ref[:, :nf] += torch.einsum("okyx,kc->ocyx", A, P)
            if L == 2:
                ref[:, x2:x2 + gc] = A
            bound = (gc + 2) * U * (W[:, :nf].abs() + torch.einsum("okyx,kc->ocyx", absA, P.abs()))
            assert ((E - ref)[:, :nf].abs() <= bound).all(), (L, ((E - ref)[:, :nf].abs() / bound).max())
            assert ((E - ref)[:, x2:x2 + gc].abs() <= U * absA).all()
            keep = torch.ones(W.shape[1], dtype=torch.bool)
            keep[:nf] = False
            if L == 2:
                keep[x2:x2 + gc] = False
            assert torch.equal(e.cpu()[:, keep], w.cpu()[:, keep])          # untouched slices: bit-identical
            # unfold: at most nf + 3 terms per element (old gradient, G, conv5's second G, nf products)
            gp = torch.einsum("ocyx,kc->okyx", G[:, :nf], P)
            agp = torch.einsum("ocyx,kc->okyx", G[:, :nf].abs(), P.abs())
            ref, b = old[1 + L] + G, old[1 + L].abs() + G.abs()
            ref[:, x2:x2 + gc] += gp
            b[:, x2:x2 + gc] += agp
            if L == 2:
                ref[:, x4:x4 + gc] += G[:, x2:x2 + gc] + gp
                b[:, x4:x4 + gc] += G[:, x2:x2 + gc].abs() + agp
            assert ((D - ref).abs() <= (nf + 3) * U * b).all(), (L, ((D - ref).abs() / ((nf + 3) * U * b)).max())
            dP = dP + torch.einsum("okyx,ocyx->kc", A, G[:, :nf])
            bP = bP + torch.einsum("okyx,ocyx->kc", absA, G[:, :nf].abs())
        terms = 9 * (2 * gc + nf) + 6                       # the products, conv5's A, the 4-way tree, the old gradient
        ref = old[0][:, :, 0, 0] + dP
        assert ((p.grad.double().cpu()[:, :, 0, 0] - ref).abs() <= terms * U * (old[0][:, :, 0, 0].abs() + bP)).all()
        for t, g1 in zip((p, *ws), got1):
            assert torch.equal(t.grad, g1)


def _restate(lr, sd, up, mode, gates):
    """RRDBNet(nb=1, plus=True) in plain torch (RRDBNet_arch.py:23-49, 89-96, 150-163), in the dtype of lr / sd.  gates: the LeakyReLU
    branches in forward order, as the engine took them -- one element within round-off of zero may take either branch in two valid
    fp32 evaluations, which moves whole gradients by 1e-3; with the branches pinned every gradient is held to round-off."""
    it = iter(gates)
    act = lambda t: t * torch.where(next(it), 1.0, 0.2).to(t.dtype)
    fea = t = O._conv(lr, sd, "model.0")
    for r in (1, 2, 3):
        pre, x = "model.1.sub.0.RDB%d" % r, t
        conv = lambda i, *f: O._conv(torch.cat(f, 1), sd, "%s.conv%d.0" % (pre, i))
        x1 = act(conv(1, x))
        x2 = act(conv(2, x, x1)) + F.conv2d(x, sd[pre + ".conv1x1.weight"])
        x3 = act(conv(3, x, x1, x2))
        x4 = act(conv(4, x, x1, x2, x3)) + x2
        t = conv(5, x, x1, x2, x3, x4) * 0.2 + x
    y = fea + O._conv(t * 0.2 + fea, sd, "model.1.sub.1")
    idx = 2
    for _ in range(up // 2):
        if mode == "upconv":
            y = act(O._conv(F.interpolate(y, scale_factor=2.0, mode="nearest"), sd, "model.%d" % (idx + 1)))
        else:
            y = act(F.pixel_shuffle(O._conv(y, sd, "model.%d" % idx), 2))
        idx += 3
    return O._conv(act(O._conv(y, sd, "model.%d" % idx)), sd, "model.%d" % (idx + 2))


def _engine_gates(saved, nf, gc=32):
    """sign of every activation the forward kept: [x1 | u2 | x3 | u4] of the dense-block buffers, the up stages, HR_conv0."""
    nchw = lambda t: t.permute(0, 3, 1, 2).detach().cpu() > 0
    g = [nchw(buf[..., nf + gc * k: nf + gc * (k + 1)]) for buf in saved["bufs"] for k in range(4)]
    return g + [nchw(dst.dense()) for _s, dst, _t in saved["stages"]] + [nchw(saved["h0"].dense())]


def rel_err(got, ref):
    return (got.detach().cpu().double() - ref.detach()).abs().max().item() / (ref.detach().abs().max().item() + 1e-12)


@pytest.mark.parametrize("mode", ["upconv", "pixelshuffle"])
@pytest.mark.parametrize("nf,kw", [(64, {}), (32, dict(upscale=2, gaussian_noise=False))])
def test_rrdbnet_plus_forward_backward(nf, kw, mode):
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    up = kw.get("upscale", 4)
    net = RRDBNet(3, 3, nf, 1, plus=True, upsample_mode=mode, **kw)
    sd = {k: v.clone() for k, v in detrand.fill_state_dict_(net.state_dict(), 5).items()}
    net = net.to(DEV)
    lr = detrand.uniform((2, 3, 12, 20), 3, 0.0, 1.0)
    gout = detrand.uniform((2, 3, 12 * up, 20 * up), 4, -1.0, 1.0)
    taken, inner = [], net.engine_forward
    net.engine_forward = lambda x, save: (lambda r: (taken.append(r[1]), r)[1])(inner(x, save))
    out = net(lr.to(DEV))
    out.backward(gout.to(DEV))
    net.engine_forward = inner
    osd = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    ref = _restate(lr.double(), osd, up, mode, _engine_gates(taken[0], nf))
    ref.backward(gout.double())
    assert rel_err(out, ref) < 2e-5
    for k, p in net.named_parameters():
        assert rel_err(p.grad, osd[k].grad) < 2e-4, k
    with torch.no_grad():                                   # the no-grad path (buffer ring) gives the same image
        assert rel_err(net(lr.to(DEV)), ref) < 2e-5
    net(lr.to(DEV)).backward(gout.to(DEV))                  # a second backward doubles every gradient, conv1x1's included
    for k, p in net.named_parameters():
        assert rel_err(p.grad, 2 * osd[k].grad) < 2e-4, k
