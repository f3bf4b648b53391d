"""Colour, averaging-downscale and multi-scale pixel losses, backed by the HIP kernels of csrc/pooled_losses.hip.

Keeps the reference's surface (codes/models/modules/loss.py): `ColorLoss` (:587-597), `AverageLoss` (:601-609), `MultiscalePixelLoss`
(:431-454) and the `L1CosineSim` criterion (:364-384), restricted to what `get_loss_fn` builds.  Every other option value raises
NotImplementedError naming it: there is no eager-PyTorch fallback.

All three have the form  box average -> (RGB -> UV) -> criterion -> sum; no pooled image is ever stored.  x carries the gradient, y (the
HR batch) is data; both are fp32 N x C x H x W with C <= 4 in one dense layout (NCHW-contiguous or channels-last).  The modules detach
y, as the reference's training step hands them a target without a graph.
"""
import torch
import torch.nn as nn

from ... import ops
from . import image_losses as IL
from ._dense import dense_layout, gscale

MAX_POOL = 8
INNER = ("l1", "l2", "cb", "elastic", "clipl1", "l1cosinesim")


class _PoolFn(torch.autograd.Function):
    """The mean-reduced criterion of the k x k box averages of x and y (`uv`: of their two chroma planes).  One launch each way."""

    @staticmethod
    def forward(ctx, x, y, k, uv, crit):
        layout = dense_layout("pooled loss", x, y)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ops.pool_loss_fwd(x, y, layout, k, uv, crit, out)
        ctx.save_for_backward(x, y)
        ctx.cfg = (layout, k, uv, crit)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx = torch.empty_like(x)          # preserves x's (possibly channels-last) strides
        ops.pool_loss_bwd(x, y, *ctx.cfg, gscale(g), gx)
        return gx, None, None, None, None


class _MultiscaleFn(torch.autograd.Function):
    """sum over five levels of w_i * the mean-reduced criterion of the 2^i x 2^i box averages.  One launch each way."""

    @staticmethod
    def forward(ctx, x, y, crit):
        layout = dense_layout("multi-scale loss", x, y)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ops.multiscale_loss_fwd(x, y, layout, crit, out)
        ctx.save_for_backward(x, y)
        ctx.cfg = (layout, crit)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx = torch.empty_like(x)
        ops.multiscale_loss_bwd(x, y, *ctx.cfg, gscale(g), gx)
        return gx, None, None


def _images(what, x, channels=None):
    if x.dim() != 4 or x.shape[1] > 4 or (channels is not None and x.shape[1] != channels):
        raise NotImplementedError("{}: expected N x {} x H x W images, got {} (other channel counts are not implemented by the HIP "
                                  "engine)".format(what, "3" if channels else "(1..4)", tuple(x.shape)))


class L1CosineSim(nn.Module):
    """mean |x - y| + loss_lambda * mean over the pixels of (1 - cosine of their channel vectors) (loss.py:364-384), the cosine as
    nn.CosineSimilarity(dim=1, eps=1e-20) forms it.  Not one of the difference-only criteria: HFEN and the image-gradient loss refuse
    it; ColorLoss, AverageLoss and MultiscalePixelLoss read `crit` and run their own fused kernels.  On its own it is the k = 1 pool."""
    crit = ops.CRIT_L1COS
    reduction = "mean"

    def __init__(self, loss_lambda=5, reduction="mean"):
        super().__init__()
        if loss_lambda != 5:
            raise NotImplementedError("L1CosineSim option loss_lambda={!r} is not implemented by the HIP engine".format(loss_lambda))
        if reduction != "mean":
            raise NotImplementedError("L1CosineSim option reduction={!r} is not implemented by the HIP engine".format(reduction))
        self.loss_lambda = loss_lambda

    def forward(self, x, y):
        _images("L1CosineSim", x)
        return _PoolFn.apply(x, y.detach(), 1, False, self.crit)


def inner_criterion(name):
    """The criterion <crit> of color-<crit>, avg-<crit> and multiscale-<crit>: the recurrent branch of the reference's get_loss_fn
    (losses.py:34-58) with the default mean reduction."""
    if name in ("l1cosinesim", "L1CosineSim"):
        return L1CosineSim()
    if name in ("L1", "l1", "MSE", "l2", "cb", "elastic", "clipl1"):
        return IL.criterion(name)
    raise NotImplementedError("criterion [{}] is not implemented by the HIP engine for the colour, average and multi-scale losses "
                              "(only {})".format(name, ", ".join(INNER)))


def _crit_of(loss_f, what):
    if isinstance(loss_f, L1CosineSim) or (isinstance(loss_f, IL._Criterion) and loss_f.reduction == "mean"):
        return loss_f.crit
    raise NotImplementedError("{}: loss_f must be a mean-reduced criterion of the HIP engine ({}), got {!r}".format(
        what, ", ".join(INNER), loss_f))


def _pool_of(ds_f, what):
    """k of a ds_f = AvgPool2d(kernel_size=k): square, stride k, no padding, floor mode."""
    def pair(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    ok = isinstance(ds_f, nn.AvgPool2d)
    if ok:
        k = pair(ds_f.kernel_size)
        ok = (k[0] == k[1] and pair(ds_f.stride if ds_f.stride is not None else ds_f.kernel_size) == k and pair(ds_f.padding) == (0, 0)
              and not ds_f.ceil_mode and ds_f.divisor_override is None and isinstance(k[0], int) and k[0] >= 1)
    if not ok:
        raise NotImplementedError("{} option ds_f={!r} is not implemented by the HIP engine (only nn.AvgPool2d with a square kernel "
                                  "equal to its stride, no padding, floor mode)".format(what, ds_f))
    if k[0] > MAX_POOL:
        raise NotImplementedError("{} option ds_f={!r}: kernel_size {} > {} is not implemented by the HIP engine".format(
            what, ds_f, k[0], MAX_POOL))
    return k[0]


class _Pooled(nn.Module):
    uv = False

    def __init__(self, loss_f=None, reduction="mean", ds_f=None):
        super().__init__()          # `reduction` is accepted and unused, as in the reference: the criterion carries its own
        what = type(self).__name__
        self.crit = _crit_of(loss_f, what)
        self.k = _pool_of(ds_f, what)
        self.criterion, self.ds_f = loss_f, ds_f

    def forward(self, x, y):
        _images(type(self).__name__, x, channels=3 if self.uv else None)
        return _PoolFn.apply(x, y.detach(), self.k, self.uv, self.crit)


class ColorLoss(_Pooled):
    """The criterion of the U and V planes (BT.601, rgb_to_yuv(..., consts='uv')) of the pooled images (loss.py:587-597)."""
    uv = True


class AverageLoss(_Pooled):
    """The criterion of the pooled images (loss.py:601-609)."""


class MultiscalePixelLoss(nn.Module):
    """sum_i w_i criterion(x_i, y_i) over five levels of 2 x 2 average pooling, w = 1, .5, .25, .125, .125 (loss.py:431-454)."""

    def __init__(self, loss_f=None, scale=5):
        super().__init__()
        self.crit = _crit_of(loss_f, "MultiscalePixelLoss")
        if scale != 5:
            raise NotImplementedError("MultiscalePixelLoss option scale={!r} is not implemented by the HIP engine (five levels "
                                      "only)".format(scale))
        self.criterion = loss_f
        self.weights = [1, 0.5, 0.25, 0.125, 0.125]

    def forward(self, x, y, mask=None):
        if mask is not None:
            raise NotImplementedError("MultiscalePixelLoss argument mask is not implemented by the HIP engine")
        _images("MultiscalePixelLoss", x)
        if min(x.shape[2:]) < 16:
            raise ValueError("MultiscalePixelLoss: five levels need min(H, W) >= 16, got {} x {} (the reference fails there too: "
                             "'Output size is too small')".format(*x.shape[2:]))
        return _MultiscaleFn.apply(x, y.detach(), self.crit)
