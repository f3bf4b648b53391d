"""PNetLin for net='squeeze', version '0.1', spatial=False (codes/models/modules/LPIPS/networks_basic.py:32-120,
pretrained_networks.py:6-55), on the MI355X engine.

The torch modules below only hold the parameters, under the reference's state_dict keys (scaling_layer.*, net.sliceK.N.*,
lin{l}.model.1.weight); nothing here computes with torch.  The forward pass runs the image pairs as one 2N batch:
  tnr_lpips_stem            ScalingLayer + features[0:2] (conv 3x3 s2 + ReLU)                      -> relu1 (64)
  tnr_maxpool3s2_ceil_fwd   features[2], [5], [8] (MaxPool2d(3, 2, ceil_mode=True))
  tnr_conv_forward          every Fire: squeeze 1x1 + ReLU, expand1x1 / expand3x3 (pad 1) + ReLU written into the two channel
                            halves of one buffer (the torch.cat of torchvision's Fire never exists)
  tnr_lpips_head            per tapped layer, right after it is produced; tnr_lpips_finalize once per chunk.
The convolutions always use the process's fp32 arithmetic (ops.FP32_MMA), never the bf16 operands of use_amp: the reference computes
this metric in fp32.
"""
import ctypes as C

import torch
import torch.nn as nn

from .... import hip, ops
from ....ops import View, new_act

# torchvision squeezenet1_1().features: index -> Fire(inplanes, squeeze, expand1x1, expand3x3); 0 = conv 3x3 s2, 2 / 5 / 8 = pools
FIRE = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128),
        9: (256, 48, 192, 192), 10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}
POOLS = (2, 5, 8)
# pretrained_networks.py:21-34: features indices of slice1..slice7; the LPIPS taps relu1..relu7 are the slice outputs
SLICES = [(0, 1), (2, 3, 4), (5, 6, 7), (8, 9), (10,), (11,), (12,)]
CHNS = [64, 128, 256, 384, 384, 512, 512]
SHIFT = [-.030, -.088, -.188]
SCALE = [.458, .448, .450]
# pairs per chunk: relu1 of a chunk (2 P images x 64 channels) stays at or below this many elements (every later buffer is smaller);
# tnr_conv_forward addresses a buffer with 32-bit offsets (< 2^31 elements)
CHUNK_ELEMS = 1 << 30


class Fire(nn.Module):
    """torchvision.models.squeezenet.Fire: parameter names squeeze / expand1x1 / expand3x3."""

    def __init__(self, inplanes, squeeze, e1, e3):
        super().__init__()
        self.squeeze = nn.Conv2d(inplanes, squeeze, 1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze, e1, 1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze, e3, 3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)


def squeezenet_features():
    """The layer list of torchvision's squeezenet1_1().features (public architecture)."""
    layers = []
    for i in range(13):
        if i == 0:
            layers.append(nn.Conv2d(3, 64, 3, stride=2))
        elif i == 1:
            layers.append(nn.ReLU(inplace=True))
        elif i in POOLS:
            layers.append(nn.MaxPool2d(3, 2, ceil_mode=True))
        else:
            layers.append(Fire(*FIRE[i]))
    return layers


class SqueezeSlices(nn.Module):
    """pretrained_networks.squeezenet: slice1..slice7 over features[0..12] (keys net.sliceK.N.*)."""

    def __init__(self):
        super().__init__()
        feats = squeezenet_features()
        for k, idx in enumerate(SLICES):
            s = nn.Sequential()
            for i in idx:
                s.add_module(str(i), feats[i])
            setattr(self, "slice%d" % (k + 1), s)

    def layer(self, i):
        for k, idx in enumerate(SLICES):
            if i in idx:
                return getattr(self, "slice%d" % (k + 1))[idx.index(i)]
        raise IndexError(i)


def torchvision_to_slices(sd):
    """A torchvision squeezenet1_1 state_dict (features.N.*, classifier.* ignored) -> {net.sliceK.N.*}."""
    out = {}
    for k, idx in enumerate(SLICES):
        for i in idx:
            pre = "features.%d." % i
            for key, v in sd.items():
                if key.startswith(pre):
                    out["net.slice%d.%d.%s" % (k + 1, i, key[len(pre):])] = v
    return out


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(SCALE)[None, :, None, None])


class NetLinLayer(nn.Module):
    """Dropout (identity in eval) + 1x1 conv without bias: key model.1.weight."""

    def __init__(self, chn_in, chn_out=1):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(chn_in, chn_out, 1, stride=1, padding=0, bias=False))


class PNetLin(nn.Module):
    def __init__(self):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.net = SqueezeSlices()
        self.chns = list(CHNS)
        self.L = len(CHNS)
        for l, c in enumerate(CHNS):
            setattr(self, "lin%d" % l, NetLinLayer(c))
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        self._engine = None

    # ------------------------------------------------------------------------------------------------------------------------
    def _prepare(self, dev):
        """Parameters on `dev`, packed for tnr_conv_forward; re-packed whenever a parameter changed (load_state_dict)."""
        if any(t.device != dev for t in list(self.parameters()) + list(self.buffers())):
            self.to(dev)
            self._engine = None
        params = list(self.parameters()) + list(self.buffers())
        key = tuple((t.data_ptr(), t._version) for t in params)
        if self._engine is not None and self._engine["key"] == key:
            return self._engine
        if self._engine is None or self._engine["ptrs"] != tuple(t.data_ptr() for t in params):
            packer = ops.WeightPacker(dev)
            fires = {}
            for i in FIRE:
                f = self.net.layer(i)
                fires[i] = (packer.add(f.squeeze.weight, ops.PACK_COL_FWD), packer.add(f.expand1x1.weight, ops.PACK_COL_FWD),
                            packer.add(f.expand3x3.weight, ops.PACK_FWD))
            self._engine = dict(packer=packer, fires=fires)
        eng = self._engine
        eng["packer"].run()
        conv0 = self.net.layer(0)
        eng["stem"] = (conv0.weight.contiguous(), conv0.bias.contiguous(), self.scaling_layer.shift.reshape(3).contiguous(),
                       self.scaling_layer.scale.reshape(3).contiguous())
        eng["lin"] = [getattr(self, "lin%d" % l).model[1].weight.reshape(-1).contiguous() for l in range(self.L)]
        eng["ptrs"] = tuple(t.data_ptr() for t in params)
        eng["key"] = tuple((t.data_ptr(), t._version) for t in params)
        return eng

    def _fire(self, eng, i, x):
        sq, e1, e3 = FIRE[i][1:]
        f = self.net.layer(i)
        i_sq, i_e1, i_e3 = eng["fires"][i]
        pk = eng["packer"]
        s = View(new_act(x.N, x.H, x.W, sq, x.buf.device))
        ops.conv(x, pk.get(i_sq), s, mode=ops.CONV_1x1, bias=f.squeeze.bias, act=ops.ACT_RELU)
        out = new_act(x.N, x.H, x.W, e1 + e3, x.buf.device)
        ops.conv(s, pk.get(i_e1), View(out, 0, e1), mode=ops.CONV_1x1, bias=f.expand1x1.bias, act=ops.ACT_RELU)
        ops.conv(s, pk.get(i_e3), View(out, e1, e3), mode=ops.CONV_3x3, bias=f.expand3x3.bias, act=ops.ACT_RELU)
        return View(out)

    @staticmethod
    def _pool(x):
        lib = hip.load()
        ho, wo = hip.c_i(), hip.c_i()
        hip.check(lib.tnr_maxpool3s2_ceil_dims(x.H, x.W, C.byref(ho), C.byref(wo)), "maxpool3s2_ceil_dims")
        y = View(new_act(x.N, ho.value, wo.value, x.C, x.buf.device))
        hip.check(lib.tnr_maxpool3s2_ceil_fwd(x.c(), y.c(), x.N, x.H, x.W, x.C, hip.stream()), "maxpool3s2_ceil_fwd")
        return y

    def _head(self, eng, l, x, P, ws):
        f0, f1 = View(x.buf[:P]), View(x.buf[P:])
        hip.check(hip.load().tnr_lpips_head(f0.c(), f1.c(), P, x.H, x.W, x.C, eng["lin"][l].data_ptr(), l, self.L, ws.data_ptr(),
                                            ws.numel() * 8, hip.stream()), "lpips_head")

    def engine_distance(self, a, b, src_kind, crop=0, normalize=False):
        """LPIPS of the N pairs (a[n], b[n]) -> (total [N], per_layer [N, L]) fp64 device tensors.  src_kind 0: uint8 NHWC images,
        cropped by `crop` per side; 1: fp32 NCHW in [-1, 1] (normalize: [0, 1] inputs)."""
        hip.require_device(a)
        dev = a.device
        lib = hip.load()
        N = a.shape[0]
        H, W = (a.shape[1], a.shape[2]) if src_kind == 0 else (a.shape[2], a.shape[3])
        ho, wo = hip.c_i(), hip.c_i()
        hip.check(lib.tnr_lpips_stem_dims(H, W, int(crop), C.byref(ho), C.byref(wo)), "lpips_stem_dims")
        Ho, Wo = ho.value, wo.value
        per_pair = 2 * 64 * Ho * Wo
        if per_pair >= 1 << 31:
            raise ValueError("LPIPS: a %dx%d image is above the engine's 2^31-element activation limit" % (H, W))
        P = max(1, min(N, CHUNK_ELEMS // per_pair))
        total = torch.empty(N, dtype=torch.float64, device=dev)
        per_layer = torch.empty((N, self.L), dtype=torch.float64, device=dev)
        prev, ops.MMA = ops.MMA, ops.FP32_MMA          # fp32-class arithmetic whatever use_amp says (restored on exit)
        try:
            eng = self._prepare(dev)
            w0, b0, shift, scale = eng["stem"]
            ws = ops.WS.get("lpips", lib.tnr_lpips_workspace_bytes(P, self.L), dev)
            for n0 in range(0, N, P):
                p = min(P, N - n0)
                y = View(new_act(2 * p, Ho, Wo, 64, dev))
                hip.check(lib.tnr_lpips_stem(a[n0:n0 + p].data_ptr(), b[n0:n0 + p].data_ptr(), src_kind, p, H, W, 3, int(crop),
                                             int(bool(normalize)), shift.data_ptr(), scale.data_ptr(), w0.data_ptr(), b0.data_ptr(),
                                             y.c(), hip.stream()), "lpips_stem")
                self._head(eng, 0, y, p, ws)
                x = y
                for l, idx in enumerate(SLICES[1:], start=1):
                    for i in idx:
                        x = self._pool(x) if i in POOLS else self._fire(eng, i, x)
                    self._head(eng, l, x, p, ws)
                hip.check(lib.tnr_lpips_finalize(p, self.L, ws.data_ptr(), ws.numel() * 8, total[n0:].data_ptr(),
                                                 per_layer[n0:].data_ptr(), hip.stream()), "lpips_finalize")
        finally:
            ops.MMA = prev
        return total, per_layer
