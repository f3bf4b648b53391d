"""Host-side plumbing the image-space modules share (ssim.py, image_losses.py, models/losses.py, dataops/filters.py): the dense-layout
check of the operands, the two small adaptations of an incoming gradient, and the reference's 1-D Gaussian window."""
import math

import torch

from ... import hip


def dense_layout(what, x, *others, any_rank=False):
    """The `layout` the kernels take for fp32 N x C x H x W operands that share one dense layout: 0 NCHW-contiguous, 1 channels-last.
    `any_rank`: contiguous operands of any rank pass too (the flat criteria read them as one range)."""
    hip.require_device(x)
    if any(t.dtype != torch.float32 for t in (x,) + others) or not (any_rank or x.dim() == 4):
        raise hip.HipEngineError("{}: fp32 N x C x H x W images only (got {} with {} dimensions)".format(
            what, " / ".join(str(t.dtype) for t in (x,) + others), x.dim()))
    if any(t.shape != x.shape or t.stride() != x.stride() for t in others):
        raise hip.HipEngineError("{}: operands must share one dense layout".format(what))
    if x.is_contiguous():
        return 0
    if x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous():
        return 1
    raise hip.HipEngineError("{}: operands must be NCHW-contiguous or channels-last".format(what))


def as_layout(g, layout):
    """The incoming gradient in the forward's dense layout (autograd may hand over other strides)."""
    fmt = torch.channels_last if layout else torch.contiguous_format
    return g if g.is_contiguous(memory_format=fmt) else g.contiguous(memory_format=fmt)


def gscale(g):
    """The incoming gradient of a scalar loss as the one fp32 element the backward kernels read."""
    return g.float().reshape(1).contiguous()


def gaussian_taps(size, sigma):
    """The reference's 1-D window (dataops/filters.py:84-87): exp(-(x - size // 2)^2 / (2 sigma^2)) in fp64 rounded to fp32, then
    normalised in fp32.  Returns a fp32 tensor of `size` taps."""
    if not isinstance(size, int) or size <= 0 or size % 2 == 0:
        raise TypeError("kernel_size must be an odd positive integer. Got {}".format(size))
    g = torch.tensor([math.exp(-(x - size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(size)], dtype=torch.float32)
    g /= g.sum()
    return g
