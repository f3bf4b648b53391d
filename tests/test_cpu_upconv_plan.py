"""ops.upconv_plan over its inputs, and the two folding tables of the nearest-x2 + 3x3 fold against plain torch
constructions -- no device, no launch: the library's 16 x 9 matrix (tnr_upconv_fold_table, generated from the helpers the pack and the
unfold kernels use) and the Python statements of both fixed addition orders (ops.upconv_fold_weights / ops.upconv_unfold_grad)."""
import itertools
import types

import pytest
import torch
import torch.nn.functional as F

from trainner_amd import hip, ops

D = torch.double


def _view(on_device):
    return types.SimpleNamespace(buf=types.SimpleNamespace(is_cuda=on_device))


@pytest.mark.parametrize("switch,mma,on_device", list(itertools.product(["0", "1", "fwd", "dgrad,wgrad", "wgrad,fwd,dgrad"],
                                                                        [hip.MMA_F32, hip.MMA_BF16, hip.MMA_BF16X3], [True, False])))
def test_upconv_plan_table(switch, mma, on_device, monkeypatch):
    want = ((), "switch") if switch == "0" else ((), "arithmetic") if mma != hip.MMA_BF16X3 else ((), "device") if not on_device else \
        (("dgrad", "wgrad") if switch == "1" else tuple(p for p in ("fwd", "dgrad", "wgrad") if p in switch.split(",")), None)
    assert ops.upconv_plan(_view(on_device), mma=mma, switch=switch) == want
    # the same answer from the live state: the environment is read at call time, the arithmetic is the module's
    monkeypatch.setenv("TNR_UPCONV_FOLD", switch)
    monkeypatch.setattr(ops, "MMA", mma)
    assert ops.upconv_plan(_view(on_device)) == want


def test_upconv_plan_default_switch_is_on(monkeypatch):
    monkeypatch.delenv("TNR_UPCONV_FOLD", raising=False)
    monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    passes, why = ops.upconv_plan(_view(True))
    assert why is None and passes == ("dgrad", "wgrad")          # the forward keeps TNR_CONV_3x3_UP2 unless it is named
    assert ops.upconv_plan(_view(True), switch="fwd,dgrad,wgrad") == (ops.UPFOLD_PASSES, None)
    assert ops.upconv_plan(_view(True), switch=0) == ((), "switch")


def _fold_matrix():
    """16 x 9, from the identity itself: per axis f[0] = w[2], f[1] = w[1] + w[2], f[2] = w[0] + w[1], f[3] = w[0]."""
    a = torch.tensor([[0, 0, 1], [0, 1, 1], [1, 1, 0], [1, 0, 0]], dtype=D)
    return torch.kron(a, a)


def test_fold_table_of_the_library():
    M = ops.upconv_fold_table()
    assert torch.equal(M, _fold_matrix())
    assert [int(v) for v in M.sum(1)] == [1, 2, 2, 1, 2, 4, 4, 2, 2, 4, 4, 2, 1, 2, 2, 1]      # 1, 2 or 4 addends per folded tap
    for k, taps in enumerate(ops.UPFOLD_TAPS):                # the Python table names the same sets
        assert [t for t in range(3) if _fold_matrix()[k * 4 + k, t * 3 + t]] == list(taps)


def _dyadic(*shape, seed):
    """Multiples of 1/64 in [-1, 1]: every sum of four is exact in fp32, so ANY addition order gives the same bits."""
    return torch.randint(-64, 65, shape, generator=torch.Generator().manual_seed(seed)).float() / 64


def test_fold_and_unfold_equal_the_matrix_exactly():
    M = _fold_matrix()
    w = _dyadic(5, 7, 3, 3, seed=1)
    assert torch.equal(ops.upconv_fold_weights(w).double(), (w.double().view(5, 7, 9) @ M.t()).view(5, 7, 4, 4))
    dF = _dyadic(7, 5, 4, 4, seed=2)
    assert torch.equal(ops.upconv_unfold_grad(dF).double(), (dF.double().view(7, 5, 16) @ M).view(7, 5, 3, 3))


def test_documented_addition_order():
    """Random fp32 values: the Python statements add in the order csrc/common.h documents (inside a row over ascending kx first, then
    the rows over ascending ky), written out here tap by tap."""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(4, 6, 3, 3, generator=g)
    Fw = ops.upconv_fold_weights(w)
    T = ops.UPFOLD_TAPS
    for ky, kx in itertools.product(range(4), range(4)):
        rows = []
        for ty in T[ky]:
            r = w[..., ty, T[kx][0]]
            for tx in T[kx][1:]:
                r = r + w[..., ty, tx]
            rows.append(r)
        want = rows[0] if len(rows) == 1 else rows[0] + rows[1]
        assert torch.equal(Fw[..., ky, kx], want), (ky, kx)
    dF = torch.randn(6, 4, 4, 4, generator=g)
    dw = ops.upconv_unfold_grad(dF)
    for ty, tx in itertools.product(range(3), range(3)):
        want = (dF[..., 2 - ty, 2 - tx] + dF[..., 2 - ty, 3 - tx]) + (dF[..., 3 - ty, 2 - tx] + dF[..., 3 - ty, 3 - tx])
        assert torch.equal(dw[..., ty, tx], want), (ty, tx)


@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (8, 8)])
def test_the_identity_borders_included(H, W):
    """nearest x2 -> conv3x3(padding 1) == conv_transpose(k 4, s 2, p 1) with the folded taps and swapped channel roles; its adjoint and
    its weight gradient follow -- in fp64, on dyadic operands (every sum exact), all borders included."""
    x = _dyadic(2, 3, H, W, seed=10 + H).double().requires_grad_(True)
    w = _dyadic(4, 3, 3, 3, seed=20 + W).double().requires_grad_(True)
    g = _dyadic(2, 4, 2 * H, 2 * W, seed=30).double()
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, padding=1)
    y.backward(g)
    Ws = ops.upconv_fold_weights(w.detach()).transpose(0, 1).contiguous()        # W_S[co_S = ci][ci_S = co]
    assert torch.equal(F.conv_transpose2d(x.detach(), Ws, stride=2, padding=1), y.detach())         # forward = data-gradient of S
    assert torch.equal(F.conv2d(g, Ws, stride=2, padding=1), x.grad)                                # data gradient = S itself
    Wl = Ws.clone().requires_grad_(True)
    F.conv2d(g, Wl, stride=2, padding=1).backward(x.detach())                                       # wgrad_S(x := g_hi, g := x_lo)
    assert torch.equal(ops.upconv_unfold_grad(Wl.grad).transpose(0, 1), w.grad)
