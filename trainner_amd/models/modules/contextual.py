"""Contextual loss (modules/loss.py:769-1092: Contextual_Loss, https://arxiv.org/abs/1803.02077) on the HIP engine: the cosine
distance and the 'regular' form over VGG taps, which is what `cx_type: contextual` builds (losses.py:129-135).  Kernels:
csrc/contextual.hip; DESIGN.md section 15.

The loss owns its own FeatureExtractor (as the reference does: a second VGG next to the `fea` term's).  The gradient is formed in the
forward call, where g = -1 / (N P CS_n) is known as soon as CS_n is: the autograd node saves only d loss / d tap, and its backward is
one scale_by.  Under no_grad, or when the SR tap needs no gradient, the gradient kernels do not run.
"""
import torch
import torch.nn as nn

from ... import hip, ops
from .architectures import perceptual

DIS_TYPES = ["cosine", "l1", "l2"]


def alt_layers_names(layers):
    """perceptual.py:43-49: conv_3_2 -> conv3_2; a key with no '_' among its first five characters is DROPPED (the reference's quirk:
    its own default {"conv3_2": 1.0, "conv4_2": 1.0} becomes {})."""
    new_layers = {}
    for k, v in layers.items():
        if "_" in k[:5]:
            new_layers[k[:5].replace("_", "") + k[5:]] = v
    return new_layers


def pooling_indices(S, n):
    """_random_sampling (loss.py:857-869): the first n entries of a permutation drawn on the CPU's global generator."""
    indices = torch.randperm(S)[:n].contiguous()
    return indices.clamp(indices.min(), S - 1)


class _CxLayerFn(torch.autograd.Function):
    """One layer's loss.  fea_x / fea_y: logical NCHW taps over NHWC storage; idx_x / idx_y: int64 CPU index lists of the pooled
    positions or None."""

    @staticmethod
    def forward(ctx, fea_x, fea_y, idx_x, idx_y, b, h, group, record):
        hip.require_device(fea_x)
        views = []
        for f in (fea_x, fea_y):
            v = f.detach().permute(0, 2, 3, 1)
            views.append(ops.View(v if v.is_contiguous() else v.contiguous()))
        x, y = views
        dev = fea_x.device
        need_grad = ctx.needs_input_grad[0]
        ix = iy = inv = None
        if idx_x is not None:
            ix = idx_x.to(torch.int32).to(dev)
            iy = idx_y.to(torch.int32).to(dev)
            if need_grad:
                inv_host = torch.full((x.H * x.W,), -1, dtype=torch.int32)
                inv_host[idx_x] = torch.arange(idx_x.numel(), dtype=torch.int32)
                inv = inv_host.to(dev)
        dx = torch.empty_like(x.buf) if need_grad else None
        out = ops.cx_layer(x, y, ix, iy, inv, b=b, h=h, dx=None if dx is None else ops.View(dx), group=group)
        if record is not None:
            record.append(out)
        ctx.save_for_backward(dx)
        return out["loss"]

    @staticmethod
    def backward(ctx, g):
        (dx,) = ctx.saved_tensors
        # data parallelism: the channel mean is global, the loss a mean over this rank's images -- nothing to rescale here, the
        # ranks' averaged gradient is the global-batch one (GeneratorLoss._log)
        of = torch.empty_like(dx)
        ops.scale_by(of, dx, g.reshape(1).contiguous())
        return of.permute(0, 3, 1, 2), None, None, None, None, None, None, None


class Contextual_Loss(nn.Module):
    """layers_weights: e.g. {'conv_3_2': 1.0, 'conv_4_2': 1.0} (the recipe's spelling; see alt_layers_names)."""

    def __init__(self, layers_weights=None, crop_quarter=False, max_1d_size=100, distance_type="cosine", b=1.0, band_width=0.5,
                 use_vgg=True, net="vgg19", calc_type="regular", z_norm=False, load_path=None, allow_random_init=False):
        super().__init__()
        assert band_width > 0, "band_width parameter must be positive."
        assert distance_type in DIS_TYPES, f"select a distance type from {DIS_TYPES}."
        for name, bad in (("b", b <= 0), ("distance_type", distance_type != "cosine"), ("calc_type", calc_type != "regular"), ("crop_quarter", crop_quarter),
                          ("use_vgg=False", not use_vgg), ("z_norm", z_norm)):
            if bad:
                raise NotImplementedError("Contextual_Loss option '%s' is not implemented by the HIP engine (b > 0, cosine distance, regular "
                                          "form, VGG taps, no crop_quarter, no z_norm)" % name)
        given = dict(layers_weights or {})
        self.layers_weights = alt_layers_names(given)
        if not self.layers_weights:
            raise ValueError("Contextual_Loss: no layer is left of cx_vgg_layers %r: layer names are written conv_3_2 (an underscore "
                             "after 'conv'); names like conv3_2 are dropped by the reference's own mapping" % (given,))
        self.crop_quarter, self.distanceType, self.max_1d_size = crop_quarter, distance_type, int(max_1d_size)
        self.b, self.band_width = float(b), float(band_width)
        self.vgg_model = perceptual.FeatureExtractor(listen_list=list(self.layers_weights.keys()), net=net, z_norm=bool(z_norm), pooling_stride=2,
                                                     load_path=load_path, allow_random_init=allow_random_init)
        self.dp_group = None          # set by GeneratorLoss when running data-parallel
        self.record = None            # a list here receives every layer's ops.cx_layer result (tests, tools)
        self.last_indices = {}        # layer -> (SR indices, HR indices) of the last pooled call

    def _taps(self, t):
        f = self.vgg_model(t)
        return f if isinstance(f, dict) else {self.vgg_model.taps[0]: f}

    def forward(self, images, gt):
        assert images.shape[1] == 3 and gt.shape[1] == 3, "VGG model takes 3 channel images."
        vgg_images = self._taps(images)
        with torch.no_grad():
            vgg_gt = self._taps(gt.detach())
        loss = 0
        self.last_indices = {}
        for key in self.layers_weights.keys():
            N, C, H, W = vgg_images[key].shape
            idx_x = idx_y = None
            if H * W > self.max_1d_size ** 2:
                # two host draws per pooled layer, SR first, as _random_pooling is called twice (loss.py:835-837)
                idx_x = pooling_indices(H * W, self.max_1d_size ** 2)
                idx_y = pooling_indices(H * W, self.max_1d_size ** 2)
                self.last_indices[key] = (idx_x, idx_y)
            loss_t = _CxLayerFn.apply(vgg_images[key], vgg_gt[key], idx_x, idx_y, self.b, self.band_width, self.dp_group, self.record)
            loss = loss + loss_t * self.layers_weights[key]
        return loss
