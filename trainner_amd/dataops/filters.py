"""Frequency-separation filters, backed by the HIP kernels of csrc/freqsep.hip.

Keeps the reference's surface (codes/dataops/filters.py): `FilterLow` (:643-671) and `FilterHigh` (:674-717) with their constructor
signatures, restricted to what `BaseModel.setup_fs` builds (base_model.py:629-639): one application of the zero-padded 9 x 9
low-pass -- `AvgPool2d(9, 1, 4, count_include_pad=True)`, or the depthwise Gaussian of `get_gaussian_kernel2d(9, 9 / 6.0)` -- and the
"separator" high-pass `clamp((x - low(x) + 1) / 2, 0, 1)`.  Every other option value raises NotImplementedError naming it: there is no
eager-PyTorch fallback.

Both modules memoize within one training step (see `_StepMemo`): the models clear the memo where they clear the networks' forward
memos (base_model.training_step).
"""
import torch
import torch.nn as nn

from .. import ops
from ..models.modules._dense import as_layout, dense_layout, gaussian_taps

KERNEL_SIZE = 9


def gaussian_taps1d(kernel_size=KERNEL_SIZE, sigma=KERNEL_SIZE / 6.0):
    """The reference's `get_gaussian_kernel1d` for an odd size (filters.py:85-87), operation for operation."""
    return gaussian_taps(kernel_size, sigma)


def gaussian_taps2d(kernel_size=KERNEL_SIZE, sigma=KERNEL_SIZE / 6.0):
    """`get_gaussian_kernel2d` (filters.py:143-148): the fp32 outer product of the 1-D taps -- FilterLow's depthwise weights."""
    k = gaussian_taps1d(kernel_size, sigma)
    return torch.matmul(k.unsqueeze(-1), k.unsqueeze(-1).t())


class _LowFn(torch.autograd.Function):
    """L x; backward: L g, the same launch (symmetric taps, zero padding: L is its own adjoint)."""

    @staticmethod
    def forward(ctx, x, taps, reuse):
        layout = dense_layout("FilterLow", x)
        if reuse is not None:
            out = reuse.detach()              # this step's earlier result for the same input values: no launch
        else:
            out = torch.empty_like(x)         # preserves x's (possibly channels-last) strides
            ops.freqsep_low(x, layout, taps, out)
        ctx.cfg = (layout, taps)
        return out

    @staticmethod
    def backward(ctx, g):
        layout, taps = ctx.cfg
        g = as_layout(g, layout)
        gx = torch.empty_like(g)
        ops.freqsep_low(g, layout, taps, gx)
        return gx, None, None


class _HighFn(torch.autograd.Function):
    """clamp((x - L x + 1) / 2, 0, 1); backward from the saved output (the clamp mask is recomputed from it, csrc/freqsep.hip)."""

    @staticmethod
    def forward(ctx, x, taps, reuse):
        layout = dense_layout("FilterHigh", x)
        if reuse is not None:
            out = reuse.detach()
        else:
            out = torch.empty_like(x)
            ops.freqsep_high_fwd(x, layout, taps, out)
        ctx.save_for_backward(out)
        ctx.cfg = (layout, taps)
        return out

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        layout, taps = ctx.cfg
        g = as_layout(g, layout)
        gx = torch.empty_like(out)
        ops.freqsep_high_bwd(g, out, layout, taps, gx)
        return gx, None, None


class _StepMemo(nn.Module):
    """Per-step memo of a filter: within one training step each filter is applied once per distinct input.  Keyed like
    engine.HipNet._memo_key (storage pointer, shape, stride, version counter); an entry pins its input, so the address cannot be
    recycled while it lives.  A repeated call with the very tensor that built the entry's graph gets the SAME result tensor -- autograd
    then sums the gradients of all its uses and the adjoint runs once; a call without a graph (`fake.detach()` in the discriminator
    stage) gets a detached alias, which keeps the discriminator's own forward memo hitting; a call that needs a graph the entry does
    not have gets a new autograd node around the stored values (no forward launch).  `memo_clear()` drops everything: entries are
    valid between the stages of ONE step only (base_model.training_step).

    Memory: an entry keeps its input, its result and (for a graph-carrying result) the autograd node alive until the next
    `memo_clear()`, i.e. through the discriminator stage and until the next step begins.  With fs that is four full-resolution fp32
    results (sr_f, hr_f, high(fake), high(real)) -- 4 x 50 MB at 16 x 3 x 512 x 512 -- that would otherwise be freed after the
    generator stage's backward; the inputs are the model's own fake_H / real_H / var_ref, which live that long anyway."""

    fn = None
    what = ""

    def _init_memo(self):
        self._memo = {}

    def memo_clear(self):
        self._memo = {}

    def forward(self, img):
        if self.gaussian and img.dim() == 4 and img.shape[1] != 3:
            # the reference loads the Gaussian as a depthwise convolution over image_channels = 3 (filters.py:658-660)
            raise RuntimeError("{}: the gaussian filter is built for 3 channels, got {}".format(self.what, img.shape[1]))
        key = (img.data_ptr(), tuple(img.shape), tuple(img.stride()), img._version)
        hit = self._memo.get(key)
        need_graph = torch.is_grad_enabled() and img.requires_grad
        if hit is not None:
            src, raw, out = hit
            if not need_graph:
                return raw.detach()
            if out is not None and src is img:
                return out
        out = self.fn.apply(img, self.taps, None if hit is None else hit[1])
        self._memo[key] = (img, out.detach(), out if need_graph else None)
        return out


def _refuse(cond, what):
    if cond:
        raise NotImplementedError("{} is not implemented by the HIP engine".format(what))


class FilterLow(_StepMemo):
    fn, what = _LowFn, "FilterLow"

    def __init__(self, recursions=1, kernel_size=9, stride=1, padding=True, image_channels=3, include_pad=True, filter_type=None):
        super().__init__()
        _refuse(recursions != 1, "FilterLow: recursions={} (1 only)".format(recursions))
        _refuse(kernel_size != KERNEL_SIZE, "FilterLow: kernel_size={} (9 only)".format(kernel_size))
        _refuse(stride != 1, "FilterLow: stride={} (1 only)".format(stride))
        _refuse(not padding, "FilterLow: padding=False")
        _refuse(not include_pad, "FilterLow: include_pad=False")
        self.gaussian = filter_type == "gaussian"
        _refuse(self.gaussian and image_channels != 3, "FilterLow: the gaussian filter with image_channels={} (3 only)".format(image_channels))
        self.recursions, self.filter_type = recursions, filter_type
        if self.gaussian:
            self.register_buffer("kernel", gaussian_taps2d(), persistent=False)      # the reference's depthwise weights, bit for bit
            self.taps = tuple(float(v) for v in gaussian_taps1d())
        else:
            # any other value, None included, is the 9 x 9 mean with the padding counted (filters.py:662-665): 1 / 81 everywhere,
            # evaluated as two passes of fp32(1 / 9)
            self.taps = (float(torch.tensor(1.0 / KERNEL_SIZE, dtype=torch.float32)),) * KERNEL_SIZE
        self._init_memo()


class FilterHigh(_StepMemo):
    fn, what = _HighFn, "FilterHigh"

    def __init__(self, recursions=1, kernel_size=9, stride=1, include_pad=True, image_channels=3, normalize=True, filter_type=None,
                 kernel=None):
        super().__init__()
        # any other type is the reference's "independent" filter, which it builds from kernel=None and cannot construct
        _refuse(filter_type not in ("gaussian", "average"),
                "FilterHigh: hpf_type / filter_type={!r} (an independent high-pass kernel; 'average' and 'gaussian' only)".format(filter_type))
        _refuse(recursions != 1, "FilterHigh: recursions={} (1 only)".format(recursions))
        _refuse(not normalize, "FilterHigh: normalize=False")
        self.filter_low = FilterLow(recursions=1, kernel_size=kernel_size, stride=stride, image_channels=image_channels,
                                    include_pad=include_pad, filter_type=filter_type)
        self.type, self.recursions, self.normalize = "separator", recursions, normalize
        self.gaussian, self.taps = self.filter_low.gaussian, self.filter_low.taps
        self._init_memo()

    def memo_clear(self):
        self._memo = {}
        self.filter_low.memo_clear()
