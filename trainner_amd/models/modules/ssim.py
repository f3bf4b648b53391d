"""SSIM and MS-SSIM as training losses, backed by the HIP kernels of csrc/ssim_loss.hip.

Keeps the reference's surface (codes/models/modules/ssim.py): `SSIM` and `MS_SSIM` modules with the same constructor signatures
and `forward(X, Y, shave=4, nonnegative_ssim=False)`, restricted to what `get_loss_fn` builds (losses.py:70-85):
`size_average=True`, `use_padding=False`, `per_channel=False`, `full=False`, and for MS-SSIM `option=1`, `normalize='relu'`.
Every other value raises NotImplementedError naming the option: there is no eager-PyTorch fallback.

X carries the gradient, Y (the HR batch) is data.  Both are fp32 N x C x H x W in one dense layout (NCHW-contiguous, which is what
`fake_H` / `real_H` have, or channels-last).  All level geometry (sizes, window taps, the sigma carried from level to level) is
worked out on the host from the shape, once per shape.
"""
import functools

import torch
import torch.nn as nn

from ... import hip, ops
from ._dense import dense_layout, gaussian_taps, gscale

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)


def pooled_size(h, w):
    """F.avg_pool2d(kernel_size=2, padding=(h % 2, w % 2)): the next MS-SSIM level's size (ssim.py:384-386)."""
    return (h + 2 * (h % 2) - 2) // 2 + 1, (w + 2 * (w % 2) - 2) // 2 + 1


@functools.lru_cache(maxsize=64)
def msssim_levels(h, w, window_size=11, window_sigma=1.5, levels=5):
    """Per level of an MS-SSIM over an h x w image (the size AFTER the shave): (h, w, taps K, sigma).  Where a level is smaller
    than the window, the window shrinks to the largest odd size that fits and sigma is scaled by new / old, and both stay
    changed for the following levels (ssim.py:345-355)."""
    out = []
    k, sigma = int(window_size), float(window_sigma)
    for i in range(levels):
        if h < 1 or w < 1:
            raise ValueError("MS-SSIM: level {} of the image is empty".format(i))
        if k > h or k > w:
            size = min(k, h, w)
            if size % 2 == 0:
                size -= 1
            if size < 1:
                raise ValueError("MS-SSIM: level {} ({} x {}) is too small for any window".format(i, h, w))
            sigma = size * sigma / k if k else 0
            k = size
        out.append((h, w, k, sigma))
        if i < levels - 1:
            if h < 2 or w < 2:
                raise ValueError("MS-SSIM: a {} x {} level cannot be pooled; the image is too small for {} levels".format(h, w, levels))
            h, w = pooled_size(h, w)
    return tuple(out)


@functools.lru_cache(maxsize=64)
def _taps_list(size, sigma):
    return tuple(float(v) for v in gaussian_taps(size, sigma))


def _constants(data_range, K):
    return float((K[0] * data_range) ** 2), float((K[1] * data_range) ** 2)


class _SSIMFn(torch.autograd.Function):
    """mean over N, C and the map of the SSIM map of the shaved images.  Y carries no gradient."""

    @staticmethod
    def forward(ctx, x, y, shave, taps, C1, C2):
        layout = dense_layout("SSIM", x, y)
        N, C, H, W = x.shape
        k = len(taps)
        dev = x.device
        sums = torch.empty((N, 2), dtype=torch.float64, device=dev)
        ops.ssim_fwd(x, y, layout, shave, taps, C1, C2, sums)
        value = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty((N, 2), dtype=torch.float32, device=dev)
        ops.msssim_combine(sums, 1, N, [C * (H - 2 * shave - k + 1) * (W - 2 * shave - k + 1)], None, 0, value, coef)
        ctx.save_for_backward(x, y, coef)
        ctx.cfg = (layout, shave, taps, C1, C2)
        return value

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[1]:
            raise hip.HipEngineError("SSIM: no gradient is implemented for the second operand (the HR batch is data)")
        x, y, coef = ctx.saved_tensors
        layout, shave, taps, C1, C2 = ctx.cfg
        gx = torch.empty_like(x)          # preserves x's (possibly channels-last) strides
        ops.ssim_bwd(x, y, layout, shave, taps, C1, C2, coef, gscale(g), gx)
        return gx, None, None, None, None, None


class _MSSSIMFn(torch.autograd.Function):
    """MS-SSIM with normalize='relu', option 1, averaged over the batch (ssim.py:320-420).

    An image for which the relu zeroes a level's `cs` (or the last level's `ssim`) has the value 0 and gets the gradient 0.  The
    reference's autograd can produce inf * 0 = NaN there (from the derivative of 0 ** w); the engine deliberately does not."""

    @staticmethod
    def forward(ctx, x, y, shave, geom, weights, C1, C2):
        layout = dense_layout("MS-SSIM", x, y)
        N, C = x.shape[:2]
        dev = x.device
        L = len(geom)
        sums = torch.empty((L, N, 2), dtype=torch.float64, device=dev)
        pyramid, counts = [], []
        cx, cy, clay, cshave = x, y, layout, shave
        for i, (h, w, k, sigma) in enumerate(geom):
            taps = _taps_list(k, sigma)
            ops.ssim_fwd(cx, cy, clay, cshave, taps, C1, C2, sums[i])
            counts.append(C * (h - k + 1) * (w - k + 1))
            pyramid.append((cx, cy, clay, cshave, taps))
            if i < L - 1:
                nh, nw = geom[i + 1][:2]
                nx = torch.empty((N, C, nh, nw), dtype=torch.float32, device=dev)
                ny = torch.empty_like(nx)
                ops.avgpool2_pad_fwd(cx, cy, clay, cshave, nx, ny)
                cx, cy, clay, cshave = nx, ny, 0, 0
        value = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty((L, N, 2), dtype=torch.float32, device=dev)
        ops.msssim_combine(sums, L, N, counts, weights, 1, value, coef)
        ctx.save_for_backward(coef, *[t for lev in pyramid for t in lev[:2]])
        ctx.meta, ctx.consts = [lev[2:] for lev in pyramid], (C1, C2)
        return value

    @staticmethod
    def backward(ctx, g):
        if ctx.needs_input_grad[1]:
            raise hip.HipEngineError("MS-SSIM: no gradient is implemented for the second operand (the HR batch is data)")
        C1, C2 = ctx.consts
        g = gscale(g)
        coarse = None
        coef, images = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        for i in range(len(ctx.meta) - 1, -1, -1):
            cx, cy = images[2 * i], images[2 * i + 1]
            clay, cshave, taps = ctx.meta[i]
            gx = torch.empty_like(cx)
            ops.ssim_bwd(cx, cy, clay, cshave, taps, C1, C2, coef[i], g, gx)
            if coarse is not None:
                ops.avgpool2_pad_bwd(coarse, gx, clay, cshave)
            coarse = gx
        return coarse, None, None, None, None, None, None


def _check_images(X, Y, channels, shave):
    if len(X.shape) != 4:
        raise ValueError("Input images must 4-d tensor.")
    if not X.shape == Y.shape:
        raise ValueError("Input images must have the same dimensions.")
    if X.shape[1] != channels:
        # the reference's depthwise conv2d with `channels` filters fails on any other channel count
        raise RuntimeError("expected input with {} channels (the `channels` the window was built for), got {}".format(
            channels, X.shape[1]))
    shave = int(shave or 0)
    if X.shape[2] - 2 * shave < 1 or X.shape[3] - 2 * shave < 1:
        raise ValueError("nothing is left of a {} x {} image after shaving {} pixels off every side".format(
            X.shape[2], X.shape[3], shave))
    return shave


class SSIM(nn.Module):
    """SSIM of two image batches (ssim.py:189-279), the batch mean of the map, as a differentiable loss term."""

    def __init__(self, window_size: int = 11, window_sigma: float = 1.5, win=None, data_range=255., K=(0.01, 0.03),
                 compensation=1.0, size_average: bool = True, channels=3, per_channel: bool = False, full: bool = False,
                 use_padding: bool = False):
        super().__init__()
        if not (window_size % 2 == 1):
            raise ValueError("Window size must be odd.")
        for name, val, want in (("win", win, None), ("compensation", compensation, 1.0), ("size_average", size_average, True),
                                ("per_channel", per_channel, False), ("full", full, False), ("use_padding", use_padding, False)):
            if val != want:
                raise NotImplementedError("SSIM option {}={!r} is not implemented by the HIP engine".format(name, val))
        if window_size > 11:
            raise NotImplementedError("SSIM option window_size={} (> 11) is not implemented by the HIP engine".format(window_size))
        win = gaussian_taps(window_size, window_sigma)
        self.window = nn.Parameter(win.repeat(channels, 1, 1, 1), requires_grad=False)
        self.taps = tuple(float(v) for v in win)
        self.channels = channels
        self.data_range, self.K = data_range, K
        self.compensation, self.use_padding, self.size_average, self.per_channel, self.full = 1.0, False, True, False, False

    def forward(self, X, Y, shave=4, nonnegative_ssim=False):
        if nonnegative_ssim:
            raise NotImplementedError("SSIM option nonnegative_ssim=True is not implemented by the HIP engine")
        shave = _check_images(X, Y, self.channels, shave)
        k = len(self.taps)
        if X.shape[2] - 2 * shave < k or X.shape[3] - 2 * shave < k:
            raise ValueError("a {}-tap window does not fit a {} x {} image shaved by {}".format(k, X.shape[2], X.shape[3], shave))
        C1, C2 = _constants(self.data_range, self.K)
        return _SSIMFn.apply(X, Y.detach(), shave, self.taps, C1, C2)


class MS_SSIM(nn.Module):
    """MS-SSIM of two image batches (ssim.py:423-512), five levels with the paper's weights, as a differentiable loss term."""

    def __init__(self, window_size: int = 11, window_sigma: float = 1.5, win=None, data_range=255., K=(0.01, 0.03),
                 size_average: bool = True, channels=3, use_padding: bool = False, weights=None, levels=None,
                 normalize=False, option=1):
        super().__init__()
        if not (window_size % 2 == 1):
            raise ValueError("Window size must be odd.")
        for name, val, want in (("win", win, None), ("size_average", size_average, True), ("use_padding", use_padding, False),
                                ("weights", weights, None), ("levels", levels, None), ("normalize", normalize, "relu"),
                                ("option", option, 1)):
            if val != want:
                raise NotImplementedError("MS_SSIM option {}={!r} is not implemented by the HIP engine".format(name, val))
        if window_size > 11:
            raise NotImplementedError("MS_SSIM option window_size={} (> 11) is not implemented by the HIP engine".format(window_size))
        w = torch.tensor(MS_WEIGHTS, dtype=torch.float32)
        self.weights = nn.Parameter(w, requires_grad=False)
        self.window = nn.Parameter(gaussian_taps(window_size, window_sigma).repeat(channels, 1, 1, 1), requires_grad=False)
        self.level_weights = tuple(float(v) for v in w)
        self.channels = channels
        self.window_size, self.win_sigma = window_size, window_sigma
        self.data_range, self.K = data_range, K
        self.use_padding, self.size_average, self.normalize, self.option = False, True, "relu", 1

    def forward(self, X, Y, shave=4, nonnegative_ssim=False):
        shave = _check_images(X, Y, self.channels, shave)
        geom = msssim_levels(X.shape[2] - 2 * shave, X.shape[3] - 2 * shave, self.window_size, float(self.win_sigma),
                             len(self.level_weights))
        C1, C2 = _constants(self.data_range, self.K)
        return _MSSSIMFn.apply(X, Y.detach(), shave, geom, self.level_weights, C1, C2)
