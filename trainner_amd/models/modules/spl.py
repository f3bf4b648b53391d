"""Spatial profile losses and the overflow loss, backed by the HIP kernels of csrc/spl_loss.hip and csrc/image_losses.hip.

Keeps the reference's surface (codes/models/modules/loss.py): `GPLoss` (:616-649), `CPLoss` (:652-707), both over `SPLoss` (:741-757),
and `OFLoss` (:527-542), with its signatures and defaults, restricted to what `get_loss_fn` builds.  Every other option value raises
NotImplementedError naming it: there is no eager-PyTorch fallback.

x carries the gradient, y (the HR batch) is data; both are fp32 N x C x H x W in one dense layout (NCHW-contiguous or channels-last).
The modules detach y, as the reference's training step hands them a target without a graph.
"""
import torch
import torch.nn as nn

from ... import ops
from ._dense import dense_layout, gscale


class _SPLFn(torch.autograd.Function):
    """The sum of the SPLoss traces over the derived-plane families of `mask` (ops.SPL_*): three launches forward, one backward."""

    @staticmethod
    def forward(ctx, x, y, mask, denorm):
        layout = dense_layout("SPL", x, y)
        loss = torch.empty(5, dtype=torch.float32, device=x.device)
        coef = ops.spl_coef(x, mask)
        ops.spl_loss_fwd(x, y, layout, mask, denorm, loss, coef)
        ctx.save_for_backward(x, y, coef)
        ctx.cfg = (layout, mask, denorm)
        return loss[4]

    @staticmethod
    def backward(ctx, g):
        x, y, coef = ctx.saved_tensors
        layout, mask, denorm = ctx.cfg
        gx = torch.empty_like(x)          # preserves x's (possibly channels-last) strides
        ops.spl_loss_bwd(x, y, layout, mask, denorm, coef, gscale(g).expand(4).contiguous(), gx)
        return gx, None, None, None


class _OverflowFn(torch.autograd.Function):
    """scale * sum log(|x - clamp(x, 0, 1)| + 1) over a dense x."""

    @staticmethod
    def forward(ctx, x, scale):
        dense_layout("overflow", x, any_rank=True)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ops.overflow_loss_fwd(x, scale, out)
        ctx.save_for_backward(x)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        gx = torch.empty_like(x)
        ops.overflow_loss_bwd(x, ctx.scale, gscale(g), gx)
        return gx, None


def _images(what, x, channels=None):
    if x.dim() != 4 or x.shape[1] > 4 or (channels is not None and x.shape[1] != channels):
        raise NotImplementedError("{}: expected N x {} x H x W images, got {} (other channel counts are not implemented by the HIP "
                                  "engine)".format(what, "3" if channels else "(1..4)", tuple(x.shape)))


class GPLoss(nn.Module):
    """Gradient profile loss: SPLoss of dy(x), dy(y) plus SPLoss of dx(x), dx(y) (loss.py:616-649)."""

    def __init__(self, trace=False, spl_denorm=False):
        super().__init__()
        if trace:
            raise NotImplementedError("GPLoss option trace=True (SPL_ComputeWithTrace) is not implemented by the HIP engine")
        self.spl_denorm = bool(spl_denorm)

    def forward(self, x, y):
        _images("GPLoss", x)
        return _SPLFn.apply(x, y.detach(), ops.SPL_GPL, self.spl_denorm)


class CPLoss(nn.Module):
    """Colour profile loss: SPLoss on RGB, on YUV and on dy / dx of YUV (loss.py:652-707).  `denorm` is applied once, before the RGB
    trace, when `spl_denorm` (the kernels apply it on load); `yuv_denorm` alone would denorm before the YUV conversion only and is
    refused."""

    def __init__(self, rgb=True, yuv=True, yuvgrad=True, trace=False, spl_denorm=False, yuv_denorm=False):
        super().__init__()
        if trace:
            raise NotImplementedError("CPLoss option trace=True (SPL_ComputeWithTrace) is not implemented by the HIP engine")
        for name, val in (("rgb", rgb), ("yuv", yuv), ("yuvgrad", yuvgrad)):
            if not val:
                raise NotImplementedError("CPLoss option {}=False is not implemented by the HIP engine (rgb, yuv and yuvgrad are all "
                                          "on, as get_loss_fn builds it)".format(name))
        if yuv_denorm and not spl_denorm:
            raise NotImplementedError("CPLoss options spl_denorm=False with yuv_denorm=True (a raw RGB trace beside a denormed YUV one) "
                                      "are not implemented by the HIP engine")
        self.rgb = self.yuv = self.yuvgrad = True
        self.spl_denorm, self.yuv_denorm = bool(spl_denorm), bool(yuv_denorm)

    def forward(self, x, y):
        _images("CPLoss", x, channels=3)
        return _SPLFn.apply(x, y.detach(), ops.SPL_CPL, self.spl_denorm)


class OFLoss(nn.Module):
    """Overflow loss: the mean of log(|x - clamp(x, 0, 1)| + 1) (loss.py:527-542)."""

    def __init__(self, legit_range=None, out_norm="bci"):
        super().__init__()
        if legit_range is None:
            legit_range = [0, 1]
        if list(legit_range) != [0, 1]:
            raise NotImplementedError("OFLoss option legit_range={!r} is not implemented by the HIP engine".format(legit_range))
        if out_norm != "bci":
            raise NotImplementedError("OFLoss option out_norm={!r} is not implemented by the HIP engine".format(out_norm))
        self.legit_range, self.out_norm = list(legit_range), out_norm

    def forward(self, x):
        if x.dim() != 4:
            raise NotImplementedError("OFLoss: only N x C x H x W batches are implemented by the HIP engine")
        return _OverflowFn.apply(x, 1.0 / x.numel())
