"""HFEN, image-gradient, total-variation and difference-only pixel losses, backed by the HIP kernels of csrc/image_losses.hip.

Keeps the reference's surface (codes/models/modules/loss.py): `CharbonnierLoss` (:47-58), `HFENLoss` (:173-224), `TVLoss` (:227-299),
`GradientLoss` (:302-325), `ElasticLoss` (:328-343), `ClipL1` (:387-402) plus `MSELoss` / `L1Loss` with a `reduction`, restricted to
what `get_loss_fn` builds.  Every other option value raises NotImplementedError naming it: there is no eager-PyTorch fallback.

All of them have the form  stencil -> criterion rho(e) -> sum.  x carries the gradient, y (the HR batch) is data; both are fp32
N x C x H x W in one dense layout (NCHW-contiguous or channels-last).  The modules detach y, as the reference's training step
hands them a target without a graph: no gradient flows to the second operand.
"""
import math

import torch
import torch.nn as nn

from ... import ops
from ._dense import dense_layout, gscale


def log_kernel_taps(kernel_size=15, sigma=2.5):
    """The reference's Laplacian-of-Gaussian kernel (dataops/filters.py:224-251 as `get_log_kernel(15, 2.5)` reaches it), with the
    same fp32 torch operations in the same order: an integer grid -(k-1)/2 .. (k-1)/2, the separable Gaussian, times
    (u^2 + v^2 - 2 sigma sigma) / (2 pi sigma^4), then -k / k.sum().  Returns a fp32 [kernel_size, kernel_size] tensor."""
    if not isinstance(kernel_size, int) or kernel_size < 3 or kernel_size % 2 == 0:
        raise TypeError("kernel_size must be an odd integer >= 3. Got {}".format(kernel_size))
    half = (kernel_size - 1) // 2
    axis = torch.arange(-half, half + 1, 1)
    gu, gv = torch.meshgrid([axis, axis], indexing="ij")
    k = 1
    for g in (gu, gv):
        k = k * torch.exp(-(g ** 2 / (2. * sigma ** 2)))
    k = k * ((gu ** 2 + gv ** 2) - (2 * sigma * sigma)) * (1 / ((2 * math.pi) * (sigma ** 2) * (sigma ** 2)))
    return -k / torch.sum(k)


# ----------------------------------------------------------------------------------------------
# autograd functions
# ----------------------------------------------------------------------------------------------
class _PointFn(torch.autograd.Function):
    """scale * sum rho(a - b) over two tensors of one dense layout.  b carries no gradient."""

    @staticmethod
    def forward(ctx, a, b, crit, scale):
        dense_layout("pixel criterion", a, b, any_rank=True)
        out = torch.empty((), dtype=torch.float32, device=a.device)
        ops.pointwise_loss_fwd(a, b, crit, scale, out)
        ctx.save_for_backward(a, b)
        ctx.cfg = (crit, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = torch.empty_like(a)          # preserves a's (possibly channels-last) strides
        ops.pointwise_loss_bwd(a, b, ctx.cfg[0], ctx.cfg[1], gscale(g), ga)
        return ga, None, None, None


class _FilterFn(torch.autograd.Function):
    """scale * sum rho(L * (x - y)), L a zero-padded K x K correlation shared by the channels."""

    @staticmethod
    def forward(ctx, x, y, taps, K, crit, scale):
        layout = dense_layout("HFEN", x, y)
        out = torch.empty((), dtype=torch.float32, device=x.device)
        dmap = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        ops.filter_loss_fwd(x, y, layout, taps, K, crit, scale, out, dmap)
        ctx.save_for_backward(dmap)
        ctx.cfg = (layout, taps, K, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        (dmap,) = ctx.saved_tensors
        layout, taps, K, scale = ctx.cfg
        gx = torch.empty_like(dmap)
        ops.filter_loss_bwd(dmap, layout, taps, K, scale, gscale(g), gx)
        return gx, None, None, None, None, None


class _FdFn(torch.autograd.Function):
    """scale * sum over the `dirs` finite-difference directions of rho(dir(x) - dir(y)); y None: rho(dir(x))."""

    @staticmethod
    def forward(ctx, x, y, dirs, crit, scale):
        layout = dense_layout("image gradients", x, *(() if y is None else (y,)))
        out = torch.empty((), dtype=torch.float32, device=x.device)
        ops.fd_loss_fwd(x, y, layout, dirs, crit, scale, out)
        ctx.save_for_backward(x, y)
        ctx.cfg = (layout, dirs, crit, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        layout, dirs, crit, scale = ctx.cfg
        gx = torch.empty_like(x)
        ops.fd_loss_bwd(x, y, layout, dirs, crit, scale, gscale(g), gx)
        return gx, None, None, None, None


# ----------------------------------------------------------------------------------------------
# criteria that depend on the difference only
# ----------------------------------------------------------------------------------------------
class _Criterion(nn.Module):
    """rho over a - b, 'mean' or 'sum' reduced.  Used on its own as a pixel loss and as the `loss_f` of HFENLoss / GradientLoss,
    which read `crit` and `reduction` and run their own fused kernels."""
    crit = None

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction not in ("mean", "sum"):
            raise NotImplementedError("reduction='{}' is not implemented by the HIP engine".format(reduction))
        self.reduction = reduction

    def scale(self, numel):
        return 1.0 / numel if self.reduction == "mean" else 1.0

    def forward(self, x, y):
        return _PointFn.apply(x, y.detach(), self.crit, self.scale(x.numel()))


class L1Loss(_Criterion):
    crit = ops.CRIT_L1


class MSELoss(_Criterion):
    crit = ops.CRIT_L2


class ElasticLoss(_Criterion):
    """0.2 * mse + 0.8 * l1 with one reduction for both (loss.py:328-343)."""
    crit = ops.CRIT_ELASTIC

    def __init__(self, a=0.2, reduction="mean"):
        super().__init__(reduction)
        if a != 0.2:
            raise NotImplementedError("ElasticLoss option a={!r} is not implemented by the HIP engine".format(a))
        self.alpha = torch.FloatTensor([a, 1 - a])


class CharbonnierLoss(_Criterion):
    """sum sqrt(e^2 + eps^2) / (b c h w): always a mean, whatever reduction the builder asked for (loss.py:47-58)."""
    crit = ops.CRIT_CB

    def __init__(self, eps=1e-6, out_norm="bci"):
        super().__init__("mean")
        if eps != 1e-6 or out_norm != "bci":
            raise NotImplementedError("CharbonnierLoss options eps={!r}, out_norm={!r} are not implemented by the HIP engine".format(
                eps, out_norm))
        self.eps, self.out_norm = eps, out_norm


class ClipL1(_Criterion):
    """mean clamp(|e|, 0, 10) (loss.py:387-402)."""
    crit = ops.CRIT_CLIPL1

    def __init__(self, clip_min=0.0, clip_max=10.0):
        super().__init__("mean")
        if clip_min != 0.0 or clip_max != 10.0:
            raise NotImplementedError("ClipL1 options clip_min={!r}, clip_max={!r} are not implemented by the HIP engine".format(
                clip_min, clip_max))
        self.clip_min, self.clip_max = clip_min, clip_max


_REFUSED = ("relativel1", "rel_l1", "rel_l2", "l1cosinesim", "L1CosineSim", "fro")


def criterion(name, reduction="mean"):
    """The recurrent branch of the reference's get_loss_fn (losses.py:34-58) for the criteria the kernels implement."""
    if name in ("L1", "l1"):
        return L1Loss(reduction)
    if name in ("MSE", "l2"):
        return MSELoss(reduction)
    if name == "cb":
        return CharbonnierLoss()
    if name == "elastic":
        return ElasticLoss(reduction=reduction)
    if name == "clipl1":
        return ClipL1()
    if name in _REFUSED or (name or "").find("multiscale") >= 0:
        raise NotImplementedError("criterion [{}] is not implemented by the HIP engine (only criteria of the difference alone: "
                                  "l1, l2, cb, elastic, clipl1)".format(name))
    raise NotImplementedError("criterion [{}] is not implemented by the HIP engine".format(name))


def _need_criterion(loss_f, what):
    if not isinstance(loss_f, _Criterion):
        raise NotImplementedError("{}: loss_f must be one of the HIP engine's difference-only criteria (l1, l2, cb, elastic, "
                                  "clipl1), got {!r}".format(what, loss_f))


# ----------------------------------------------------------------------------------------------
# the three losses
# ----------------------------------------------------------------------------------------------
class HFENLoss(nn.Module):
    """High-frequency error norm (loss.py:173-224): the criterion of the LoG-filtered images.  Every supported criterion depends on
    L * x - L * y only, so the difference is filtered once, with the reference's 225 taps."""

    def __init__(self, loss_f=None, kernel="log", kernel_size=15, sigma=2.5, norm=False):
        super().__init__()
        _need_criterion(loss_f, "HFENLoss")
        if kernel != "log":
            raise NotImplementedError("HFENLoss option kernel={!r} is not implemented by the HIP engine".format(kernel))
        if norm:
            raise NotImplementedError("HFENLoss option norm=True is not implemented by the HIP engine")
        if kernel_size > 15:
            raise NotImplementedError("HFENLoss option kernel_size={} (> 15) is not implemented by the HIP engine".format(kernel_size))
        self.criterion, self.norm, self.kernel_size = loss_f, False, kernel_size
        k = log_kernel_taps(kernel_size, sigma)
        self.register_buffer("kernel", k, persistent=False)
        self.taps = tuple(float(v) for v in k.flatten())
        self.sum_reduced = loss_f.reduction == "sum"

    def forward(self, x, y):
        if x.dim() != 4 or x.shape[1] != 3:
            # the reference's load_filter builds a 3-channel depthwise convolution (dataops/filters.py:457)
            raise RuntimeError("HFEN: expected N x 3 x H x W images (the reference's filter is fixed at 3 channels), got {}".format(
                tuple(x.shape)))
        return _FilterFn.apply(x, y.detach(), self.taps, self.kernel_size, self.criterion.crit, self.criterion.scale(x.numel()))


class GradientLoss(nn.Module):
    """Mean over the 2 or 4 finite-difference directions of the mean-reduced criterion (loss.py:302-325)."""

    def __init__(self, loss_f=None, reduction="mean", gradientdir="2d"):
        super().__init__()
        _need_criterion(loss_f, "GradientLoss")
        if loss_f.reduction != "mean":
            raise NotImplementedError("GradientLoss with a sum-reduced criterion is not implemented by the HIP engine")
        self.criterion, self.gradientdir = loss_f, gradientdir
        self.dirs = 4 if gradientdir == "4d" else 2          # anything but '4d' is '2d' in the reference

    def forward(self, x, y):
        if x.dim() != 4:
            raise ValueError("Expected N x C x H x W images, got {} dimensions".format(x.dim()))
        return _FdFn.apply(x, y.detach(), self.dirs, self.criterion.crit, 1.0 / (self.dirs * x.numel()))


class TVLoss(nn.Module):
    """Total variation (loss.py:227-299) as get_loss_fn builds it: per image the sum over the directions of mean |g| or g^2, summed
    over the batch and divided by the batch size."""

    def __init__(self, tv_type="tv", p=2, reduction="mean", out_norm="b", beta=2):
        super().__init__()
        if isinstance(p, str):
            p = 1 if "1" in p else 2
        if p not in (1, 2):
            raise ValueError("Expected p value to be 1 or 2, but got {}".format(p))
        for name, val, want in (("reduction", reduction, "mean"), ("out_norm", out_norm, "b"), ("beta", beta, 2)):
            if val != want:
                raise NotImplementedError("TVLoss option {}={!r} is not implemented by the HIP engine".format(name, val))
        self.p, self.tv_type, self.out_norm, self.beta = p, tv_type.lower(), out_norm, beta
        self.dirs = 4 if self.tv_type in ("dtv", "4d") else 2

    def forward(self, x):
        if x.dim() != 4:
            raise NotImplementedError("TVLoss: only N x C x H x W batches are implemented by the HIP engine")
        return _FdFn.apply(x, None, self.dirs, ops.CRIT_L1 if self.p == 1 else ops.CRIT_L2, 1.0 / x.numel())
