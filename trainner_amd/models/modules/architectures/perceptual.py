"""VGG feature extractor for the perceptual and style losses, on the MI355X engine.

Follows codes/models/modules/architectures/perceptual.py FeatureExtractor (:73-214): ImageNet
(x-mean)/std, torchvision cfg-E/D `features` truncated after the last listened layer, listened
features taken BEFORE the ReLU when a 'convX_Y' name is listened (the `x.clone()` at :211-212
happens before the in-place ReLU that follows).  Parameters are frozen (requires_grad False,
:185-188): only the data-gradient schedule exists.

`listen_list` is any non-empty set of convX_Y / reluX_Y / poolX names.  One forward taps the network at
every listened layer and returns {name: feature} in network order; it is ONE autograd node with one
output per tap, and its backward is one reverse sweep that takes one gradient per tap (absent ones are
skipped) and injects it where the tap was taken: a relu or pool tap's gradient joins the running
gradient before that layer's derivative, a conv tap's after the ReLU mask of the layer above.  No
convolution runs twice.  A conv tap below the last layer costs one elementwise pass (its pre-ReLU map is
the tap, relu(map) feeds the next layer); an injected gradient costs one (conv, pool) or two (relu: mask,
then add) elementwise passes.  The configuration with one conv tap that is also the last layer (the
ESRGAN recipe's conv5_4) runs the launches it always ran.  Still refused, by name: remove_pooling,
change_padding, requires_grad, z_norm (and rotations / flips in PerceptualLoss, which draw random numbers).

torchvision is not a dependency of the kernels: the layer table is the public VGG configuration.
Weights: `load_path` (a torchvision `vggNN` state_dict, keys `features.N.*`) when given, else
torchvision's pretrained ImageNet weights exactly like the reference (:139-144).  If neither is
available the constructor RAISES -- a perceptual loss against random features is never entered
silently; benchmarks and parity tests (no network access: they load their own seeded weights right
after construction) opt in with `allow_random_init=True` (option `train.perceptual_allow_random_init`).
"""
import logging
import os

import torch
import torch.nn as nn

from .... import ops
from ....engine import ConvOp, HipNet
from ....ops import View, new_act
from . import block as B

logger = logging.getLogger("base")

VGG_CFG = {
    "vgg16": [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"],
    "vgg19": [64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512, 512, 512, "M"],
}


def vgg_layer_names(net):
    names, blk, idx = [], 1, 1
    for v in VGG_CFG[net]:
        if v == "M":
            names.append("pool%d" % blk)
            blk, idx = blk + 1, 1
        else:
            names += ["conv%d_%d" % (blk, idx), "relu%d_%d" % (blk, idx)]
            idx += 1
    return names


# file names of torchvision's ImageNet checkpoints (torchvision/models/vgg.py model_urls), as cached under <torch hub dir>/checkpoints
TORCHVISION_FILES = {"vgg11": "vgg11-8a719046.pth", "vgg13": "vgg13-19584684.pth", "vgg16": "vgg16-397923af.pth", "vgg19": "vgg19-dcbb9e9d.pth"}


class PooledAway:
    """The tape's place-holder for the full-resolution activation of a conv + ReLU + pool triple that ran as one launch
    (FeatureExtractor._fwd_pooled): the map was never stored; what is kept is the pooled map and one route byte per pooled element
    (bits 0-1: the window position the pool picked, bit 2: pooled value > 0)."""
    __slots__ = ("route", "pooled")

    def __init__(self, route, pooled):
        self.route, self.pooled = route, pooled

    def dense(self):
        """torch stand-in [N, H, W, C] for inspection (debug / tests only, like View.dense): the pooled value at the position the pool
        picked, -inf at the three positions it did not -- their values do not exist.  `> 0` is the ReLU branch at every position a
        gradient can reach, and F.max_pool2d(..., return_indices=True) finds the winners."""
        p = self.pooled.dense()
        N, Hp, Wp, Cc = p.shape
        arg = self.route & 3
        out = torch.full((N, Hp, 2, Wp, 2, Cc), float("-inf"), dtype=p.dtype, device=p.device)
        for k in range(4):
            out[:, :, k >> 1, :, k & 1] = torch.where(arg == k, p, out[:, :, k >> 1, :, k & 1])
        return out.reshape(N, 2 * Hp, 2 * Wp, Cc)


class FeatureExtractor(HipNet):
    def __init__(self, listen_list=None, net="vgg19", use_input_norm=True, z_norm=False, requires_grad=False,
                 remove_pooling=False, pooling_stride=2, change_padding=False, load_path=None, allow_random_init=False):
        super().__init__()
        for opt_name, on in (("remove_pooling", remove_pooling), ("change_padding", change_padding), ("requires_grad", requires_grad),
                             ("z_norm", z_norm)):
            if on:
                raise NotImplementedError("FeatureExtractor option '%s' is not implemented by the HIP engine" % opt_name)
        if net not in VGG_CFG or pooling_stride != 2:
            raise NotImplementedError("FeatureExtractor net=%r / pooling_stride=%r is not implemented by the HIP engine" % (net, pooling_stride))
        listen_list = list(listen_list or ["conv5_4"])
        names = vgg_layer_names(net)
        unknown = [v for v in listen_list if v not in names]
        if unknown:
            raise ValueError("FeatureExtractor(%s): unknown layer name(s) %s" % (net, ", ".join(map(str, unknown))))
        self.listen_list = set(listen_list)
        self.use_input_norm = use_input_norm
        last = max(names.index(v) for v in listen_list)       # truncated after the last listened layer (perceptual.py:129-144)
        self.names = names[:last + 1]
        self.taps = [n for n in self.names if n in self.listen_list]      # network order
        # one conv tap that is also the last layer: the single-output node and launch sequence this class always had
        self._single = len(self.taps) == 1 and self.taps[0].startswith("conv")
        self.listen = self.taps[0] if self._single else None
        layers, c, chans = nn.ModuleDict(), 3, iter([v for v in VGG_CFG[net] if v != "M"])
        for n in self.names:
            if n.startswith("conv"):
                v = next(chans)
                layers[n] = B.Conv2dHIP(c, v, 3, 1)
                c = v
            else:
                layers[n] = B.Marker(n)
        self.feature_net = layers            # keys feature_net.convX_Y.{weight,bias} as in the reference
        self.out_channels = c
        if use_input_norm:
            self.register_buffer("mean", torch.tensor([[[0.485]], [[0.456]], [[0.406]]]))
            self.register_buffer("std", torch.tensor([[[0.229]], [[0.224]], [[0.225]]]))
        self.weights_source = self._load_pretrained(net, load_path, allow_random_init)
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self._init_engine()
        self._norm = None

    def _load_pretrained(self, net, load_path, allow_random_init):
        """perceptual.py:134-144: a local torchvision state_dict, else torchvision's ImageNet weights; never a
        silent random init."""
        if load_path and os.path.exists(load_path):
            self.load_torchvision_state(torch.load(load_path, map_location="cpu", weights_only=False))
            return load_path
        why = "pretrained_path %r does not exist" % load_path if load_path else "no perceptual_opt.pretrained_path given"
        try:
            from torchvision.models import vgg as tv_vgg          # optional: not installed on the build image
            self.load_torchvision_state(getattr(tv_vgg, net)(pretrained=True).state_dict())
            return "torchvision:%s" % net
        except Exception as e:                                    # no torchvision / no network / no cached weights
            why += "; torchvision pretrained weights unavailable (%s: %s)" % (type(e).__name__, e)
        # the file torchvision's `pretrained=True` would have cached (torch.hub checkpoints dir, $TORCH_HOME): usable without
        # torchvision itself -- an offline box that carries the cached weights runs the reference's recipe unmodified
        cached = os.path.join(torch.hub.get_dir(), "checkpoints", TORCHVISION_FILES.get(net, ""))
        if os.path.isfile(cached):
            self.load_torchvision_state(torch.load(cached, map_location="cpu", weights_only=False))
            return cached
        why += "; no cached %s" % cached
        if not allow_random_init:
            from ....hip import HipEngineError
            raise HipEngineError("FeatureExtractor(%s): %s. A perceptual loss on randomly initialised features is refused; "
                                 "set train.perceptual_opt.pretrained_path to a torchvision %s state_dict, or opt in with "
                                 "train.perceptual_allow_random_init: true (benchmarks / parity tests that load their own "
                                 "weights)" % (net, why, net))
        logger.warning("FeatureExtractor(%s): %s -- weights left at their random init (allow_random_init)", net, why)
        return "random-init"

    def load_torchvision_state(self, sd):
        """Accept a torchvision vggNN state_dict (features.<i>.weight/bias): torchvision's `features`
        indices run over the same conv / relu / pool sequence as self.names."""
        own = self.state_dict()
        for i, n in enumerate(self.names):
            if n.startswith("conv"):
                own["feature_net.%s.weight" % n].copy_(sd["features.%d.weight" % i])
                own["feature_net.%s.bias" % n].copy_(sd["features.%d.bias" % i])

    def _build_ops(self, packer):
        self._ops = {n: ConvOp(self.feature_net[n], packer) for n in self.names if n.startswith("conv")}

    def _norm_consts(self, dev):
        """(x - mean)/std as x*scale + shift; six host-side constants uploaded once."""
        if self._norm is None or self._norm[0].device != dev:
            if self.use_input_norm:
                mean = [float(v) for v in self.mean.reshape(3).cpu().tolist()]
                std = [float(v) for v in self.std.reshape(3).cpu().tolist()]
                scale = torch.tensor([1.0 / s for s in std], dtype=torch.float32).to(dev)
                shift = torch.tensor([-m / s for m, s in zip(mean, std)], dtype=torch.float32).to(dev)
            else:
                scale = torch.ones(3).to(dev)
                shift = torch.zeros(3).to(dev)
            self._norm = (scale, shift)
        return self._norm

    def _fwd_pooled(self, i, cur, save):
        """names[i] = convX_Y followed by reluX_Y and poolX with no tap on the conv or the relu: the three layers as ONE launch that
        stores the pooled map only (ops.conv_pool2) -> the two tape entries (convX_Y, cur, away) and (poolX, away,
        pooled view); away: a PooledAway in the place of the full-resolution map, with the arg-max / sign bytes the backward routes
        by (None when nothing is saved: no full-resolution tensor and no bytes exist then).  None: not such a triple, or the launch
        is declined -- nothing ran, the caller keeps its launches."""
        names = self.names
        n = names[i]
        if (i + 2 >= len(names) or not names[i + 2].startswith("pool") or n in self.listen_list or names[i + 1] in self.listen_list
                or not ops.pool_fold_on() or cur.H % 2 or cur.W % 2):
            return None
        shape = (cur.N, cur.H // 2, cur.W // 2, self.feature_net[n].out_channels)
        dev = cur.buf.device
        y = View(new_act(*shape, dev))
        route = torch.empty(shape, dtype=torch.uint8, device=dev) if save else None
        if not self._ops[n].fwd_pool2(cur, y, route=route, act=ops.ACT_RELU):
            return None
        away = PooledAway(route, y) if save else None
        return [(n, cur, away), (names[i + 2], away, y)]

    @staticmethod
    def _pool_bwd(g, xin, y):
        """Gradient of a pool's input (with ReLU' of the pooled activation) from the tape entry (poolX, xin, y): xin is the
        full-resolution activation, or the PooledAway of a pooled convolution store."""
        gx = View(new_act(y.N, 2 * y.H, 2 * y.W, y.C, y.buf.device))
        if isinstance(xin, View):
            ops.maxpool2_bwd(g, xin, gx)                                  # routes + ReLU' of the pooled activation
        else:
            ops.unpool2_bwd(g, xin.route, gx)                             # the same, from the bytes
        return gx

    def engine_forward(self, x, save):
        N, Cc, H, W = x.shape
        if Cc != 3:
            raise ValueError("FeatureExtractor expects RGB input")
        dev = x.device
        scale, shift = self._norm_consts(dev)
        x4 = View(new_act(N, H, W, 4, dev))
        ops.nchw_to_nhwc(x, x4, Cpad=4, scale=scale, shift=shift)
        cur, tape, folded = x4, [], None
        for i, n in enumerate(self.names):
            if n.startswith("conv"):
                entries = self._fwd_pooled(i, cur, save)
                if entries is not None:                                   # conv + ReLU + the pool behind them: one launch
                    tape += entries
                    cur, folded = entries[1][2], entries[1][0]
                    continue
                y = View(new_act(N, cur.H, cur.W, self.feature_net[n].out_channels, dev))
                if n == self.listen:
                    self._ops[n].fwd(cur, y)                              # listened pre-ReLU
                else:
                    self._ops[n].fwd(cur, y, act=ops.ACT_RELU)
                tape.append((n, cur, y))
                cur = y
            elif n.startswith("pool") and n != folded:
                y = View(new_act(N, cur.H // 2, cur.W // 2, cur.C, dev))
                ops.maxpool2_fwd(cur, y)
                tape.append((n, cur, y))
                cur = y
        # logical NCHW tensor over the NHWC storage (channels_last strides); L1 is layout agnostic
        out = cur.buf.permute(0, 3, 1, 2)
        return out, (dict(tape=tape, in_shape=(N, H, W)) if save else None)

    def engine_backward(self, sv, gout, need_input_grad, need_param_grad):
        if not need_input_grad:
            return None
        tape = sv["tape"]
        N, H, W = sv["in_shape"]
        dev = gout.device
        g_nhwc = gout.permute(0, 2, 3, 1)
        if not g_nhwc.is_contiguous():
            g_nhwc = g_nhwc.contiguous()
        g = View(g_nhwc)
        for i in range(len(tape) - 1, -1, -1):
            n, xin, y = tape[i]
            if n.startswith("pool"):
                gx = self._pool_bwd(g, xin, y)
            else:
                gx = View(new_act(N, xin.H, xin.W, xin.C, dev))
                prev = tape[i - 1][0] if i > 0 else None
                if prev is not None and prev.startswith("conv"):
                    self._ops[n].dgrad(g, gx, mask=xin, m_slope=0.0)      # ReLU' of the producing conv
                else:
                    self._ops[n].dgrad(g, gx)                             # input image / pooled map: no activation
            g = gx
        scale, _ = self._norm_consts(dev)
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
        ops.nhwc_to_nchw(View(g.buf, 0, 3), out, scale=scale)
        return out

    # ---- any number of taps -------------------------------------------------------------------------------------------
    def engine_forward_taps(self, x, save):
        """The sweep of engine_forward with a tap at every listened layer.  tape: (name, input view, output view the next layer reads)
        per conv / pool; feats: name -> view."""
        N, Cc, H, W = x.shape
        if Cc != 3:
            raise ValueError("FeatureExtractor expects RGB input")
        dev = x.device
        scale, shift = self._norm_consts(dev)
        x4 = View(new_act(N, H, W, 4, dev))
        ops.nchw_to_nhwc(x, x4, Cpad=4, scale=scale, shift=shift)
        cur, tape, feats, folded = x4, [], {}, None
        for i, n in enumerate(self.names):
            if n.startswith("conv"):
                entries = self._fwd_pooled(i, cur, save)
                if entries is not None:                                   # conv + ReLU + the pool behind them: one launch
                    tape += entries
                    cur, folded = entries[1][2], entries[1][0]
                    continue
                y = View(new_act(N, cur.H, cur.W, self.feature_net[n].out_channels, dev))
                if n not in self.listen_list:
                    self._ops[n].fwd(cur, y, act=ops.ACT_RELU)
                else:
                    self._ops[n].fwd(cur, y)                              # listened pre-ReLU
                    feats[n] = y
                    if i + 1 < len(self.names):                           # the network goes on: relu(map) in one elementwise pass
                        post = View(new_act(N, y.H, y.W, y.C, dev))
                        ops.mask_copy(post, y, y, mslope=0.0)             # y * (y > 0)
                        y = post
                tape.append((n, cur, y))
                cur = y
            elif n.startswith("pool"):
                if n != folded:
                    y = View(new_act(N, cur.H // 2, cur.W // 2, cur.C, dev))
                    ops.maxpool2_fwd(cur, y)
                    tape.append((n, cur, y))
                    cur = y
                if n in self.listen_list:                                 # (a folded pool's tap is the tensor the launch stored)
                    feats[n] = cur
            elif n in self.listen_list:                                   # reluX_Y: the post-ReLU map the next layer reads
                feats[n] = cur
        outs = tuple(feats[n].buf.permute(0, 3, 1, 2) for n in self.taps)
        return outs, (dict(tape=tape, in_shape=(N, H, W)) if save else None)

    @staticmethod
    def _grad_view(g):
        g_nhwc = g.permute(0, 2, 3, 1)
        return View(g_nhwc if g_nhwc.is_contiguous() else g_nhwc.contiguous())

    def _inject(self, entry, tg, g):
        """Add the tap gradients of `entry`'s output maps to the running gradient g (None: nothing arrived from above yet), in the
        running form: with respect to the PRE-activation map for a conv (the ReLU mask of the layer above already applied to what
        came through it), to the pooled map for a pool.  Tap gradients are never written to."""
        n, xin, y = entry
        if not isinstance(y, View):                                       # a conv folded with its pool (_fwd_pooled): no tap listens on it
            return g
        dev = y.buf.device

        def add(g, t):
            if g is None:
                return t
            if any(g is v for v in tg.values()):                          # still a caller's tensor: sum into a fresh buffer
                s = View(new_act(y.N, y.H, y.W, y.C, dev))
                ops.add2(s, g, t)
                return s
            ops.axpby(g, t, 1.0, 1.0)
            return g

        if n.startswith("pool"):
            return add(g, tg[n]) if tg.get(n) is not None else g
        tr = tg.get("relu" + n[4:])
        if tr is not None:                                                # before the ReLU's derivative: mask it, then add
            m = View(new_act(y.N, y.H, y.W, y.C, dev))
            ops.mask_copy(m, tr, y, mslope=0.0)                           # y is the post-ReLU map here: same sign pattern as the pre-ReLU one
            g = m if g is None else add(g, m)
        if tg.get(n) is not None:                                         # conv tap: after the mask
            g = add(g, tg[n])
        return g

    def engine_backward_taps(self, sv, gouts):
        tape = sv["tape"]
        N, H, W = sv["in_shape"]
        tg = {n: self._grad_view(g) for n, g in zip(self.taps, gouts) if g is not None}
        dev = tape[0][1].buf.device
        g = self._inject(tape[-1], tg, None)
        for i in range(len(tape) - 1, -1, -1):
            n, xin, y = tape[i]
            if g is not None:
                if n.startswith("pool"):
                    gx = self._pool_bwd(g, xin, y)
                else:
                    gx = View(new_act(N, xin.H, xin.W, xin.C, dev))
                    prev = tape[i - 1][0] if i > 0 else None
                    if prev is not None and prev.startswith("conv"):
                        self._ops[n].dgrad(g, gx, mask=xin, m_slope=0.0)  # ReLU' of the producing conv
                    else:
                        self._ops[n].dgrad(g, gx)                         # input image / pooled map: no activation
                g = gx
            if i > 0:
                g = self._inject(tape[i - 1], tg, g)
        out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)
        if g is None:
            return out.zero_()
        scale, _ = self._norm_consts(dev)
        ops.nhwc_to_nchw(View(g.buf, 0, 3), out, scale=scale)
        return out

    def forward(self, x):
        if self._single:
            return {self.listen: super().forward(x)}
        x = x.contiguous()
        self._prepare(x)
        feats = _TapsFn.apply(self, x, *self.parameters())
        return dict(zip(self.taps, feats))


class _TapsFn(torch.autograd.Function):
    """The multi-tap extractor as ONE autograd node with one output per listened layer (the frozen parameters are listed as inputs
    like in engine._NetFn; they get no gradient)."""

    @staticmethod
    def forward(ctx, net, x, *params):
        ctx.set_materialize_grads(False)                  # a tap no loss term reads arrives as None and is skipped
        outs, saved = net.engine_forward_taps(x, save=ctx.needs_input_grad[1])
        ctx.net, ctx.saved = net, saved
        return outs

    @staticmethod
    def backward(ctx, *gouts):
        saved, ctx.saved = ctx.saved, None
        if saved is None:
            raise RuntimeError("HIP engine: backward through a forward that saved no activations")
        gx = ctx.net.engine_backward_taps(saved, gouts) if ctx.needs_input_grad[1] else None
        return (None, gx) + (None,) * (len(ctx.needs_input_grad) - 2)
