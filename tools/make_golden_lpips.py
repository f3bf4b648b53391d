"""tests/golden/lpips_squeeze.pt from the REFERENCE's own LPIPS metric (utils/metrics.py MetricsDict('lpips') -> calculate_lpips ->
PerceptualLoss(net-lin, squeeze, v0.1) -> PNetLin), run on the CPU where the reference tree exists (never on a GPU machine):

    python tools/make_golden_lpips.py

torchvision is not installed there (oracle/stubs/torchvision raises for squeezenet1_1), and its pretrained backbone cannot be
downloaded: for this run only, the stub's squeezenet1_1 is replaced in memory by the public SqueezeNet 1.1 layer table below with
weights from oracle.detrand.fill_state_dict_(seed), so the 5 MB backbone is neither needed nor committed.  The linear heads are the
reference's own lpips_weights/v0.1/squeeze.pth (loaded by the reference itself; the fixture keeps a copy, 10.8 KB of data).
Image sizes are picked so that ceil-mode pooling matters (a 66 x 66 image after the crop: conv1 32 x 32, pool1 16 x 16 where floor
mode gives 15 x 15).
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "lpips_squeeze.pt")
SEED = 4242
GAIN = 1.0
CROP = 4
# (name, H, W before the crop, kind): "noisy" = b is a with bounded noise, "same" = b is a, "pm1" = b is a with +-1 in a few pixels
PAIRS = [("even66", 74, 74, "noisy"), ("odd35x50", 43, 58, "noisy"), ("sq128", 136, 136, "noisy"), ("same", 40, 40, "same"),
         ("pm1", 74, 74, "pm1")]
FIRE = {3: (64, 16, 64, 64), 4: (128, 16, 64, 64), 6: (128, 32, 128, 128), 7: (256, 32, 128, 128),
        9: (256, 48, 192, 192), 10: (384, 48, 192, 192), 11: (384, 64, 256, 256), 12: (512, 64, 256, 256)}


class Fire(nn.Module):
    def __init__(self, inplanes, squeeze, e1, e3):
        super().__init__()
        self.squeeze = nn.Conv2d(inplanes, squeeze, 1)
        self.squeeze_activation = nn.ReLU(inplace=True)
        self.expand1x1 = nn.Conv2d(squeeze, e1, 1)
        self.expand1x1_activation = nn.ReLU(inplace=True)
        self.expand3x3 = nn.Conv2d(squeeze, e3, 3, padding=1)
        self.expand3x3_activation = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.squeeze_activation(self.squeeze(x))
        return torch.cat([self.expand1x1_activation(self.expand1x1(x)), self.expand3x3_activation(self.expand3x3(x))], 1)


class SqueezeNet11(nn.Module):
    """torchvision.models.squeezenet1_1 `features` (the classifier is not used by LPIPS)."""

    def __init__(self):
        super().__init__()
        layers = []
        for i in range(13):
            if i == 0:
                layers.append(nn.Conv2d(3, 64, kernel_size=3, stride=2))
            elif i == 1:
                layers.append(nn.ReLU(inplace=True))
            elif i in (2, 5, 8):
                layers.append(nn.MaxPool2d(kernel_size=3, stride=2, ceil_mode=True))
            else:
                layers.append(Fire(*FIRE[i]))
        self.features = nn.Sequential(*layers)


def seeded_backbone_state(seed=SEED, gain=GAIN):
    """The torchvision-keyed (features.N.*) backbone state_dict every consumer of the fixture rebuilds from (seed, gain)."""
    sd = {k: v.detach().clone() for k, v in SqueezeNet11().state_dict().items()}
    return detrand.fill_state_dict_(sd, seed, gain=gain)


def image_pairs():
    out = []
    for i, (name, H, W, kind) in enumerate(PAIRS):
        a = (detrand.uniform01(H * W * 3, 900 + i) * 256).floor().clamp(0, 255).to(torch.uint8).reshape(H, W, 3)
        if kind == "same":
            b = a.clone()
        elif kind == "pm1":
            b = a.clone().to(torch.int16)
            for j in range(12):                          # 12 pixels of one channel each, +-1, away from 0 / 255 saturation
                y, x, c = (7 * j + 20) % (H - 2 * CROP) + CROP, (11 * j + 13) % (W - 2 * CROP) + CROP, j % 3
                b[y, x, c] += 1 if j % 2 == 0 else -1
            b = b.clamp(0, 255).to(torch.uint8)
        else:
            noise = (detrand.uniform01(H * W * 3, 950 + i) * 41).floor().to(torch.int16).reshape(H, W, 3) - 20
            b = (a.to(torch.int16) + noise).clamp(0, 255).to(torch.uint8)
        out.append((name, a, b))
    return out


def build_fixture():
    tv_sd = seeded_backbone_state()
    with R.reference_env():
        import torchvision.models as tvm
        saved = tvm.squeezenet1_1

        def squeezenet1_1(pretrained=False, **kw):
            net = SqueezeNet11()
            net.load_state_dict(tv_sd)
            return net

        tvm.squeezenet1_1 = squeezenet1_1
        try:
            from models.modules.LPIPS import networks_basic as ref_nb, perceptual_loss as ref_pl
            from utils.metrics import MetricsDict
            md = MetricsDict("lpips")
            pnet = md.lpips_model.model.net
            pnet_keys = [(k, tuple(v.shape)) for k, v in pnet.state_dict().items()]
            lin = {k: v.detach().clone() for k, v in pnet.state_dict().items() if k.startswith("lin")}
            pairs = []
            for name, a, b in image_pairs():
                an, bn = a.numpy(), b.numpy()
                calc = md.calculate_metrics(an, bn, crop_size=CROP)
                c1, c2 = an[CROP:-CROP, CROP:-CROP, ...], bn[CROP:-CROP, CROP:-CROP, ...]
                # PNetLin.forward sums the layers in place into res[0] (`val = res[0]; val += res[l]`): the per-layer values are
                # recorded as its spatial_average hands them out (the totals come from the unpatched MetricsDict call above)
                avg0, rec = ref_nb.spatial_average, []

                def recording(t, keepdim=True):
                    r = avg0(t, keepdim=keepdim)
                    rec.append(float(r))
                    return r

                ref_nb.spatial_average = recording
                try:
                    with torch.no_grad():
                        val, res = pnet.forward(ref_pl.im2tensor(c1), ref_pl.im2tensor(c2), retPerLayer=True)
                finally:
                    ref_nb.spatial_average = avg0
                per_layer = rec
                pairs.append(dict(name=name, img1=a, img2=b, crop=CROP, total=float(calc["lpips"]), per_layer=per_layer,
                                  total_direct=float(val)))
            avg = md.get_averages()["lpips"]
        finally:
            tvm.squeezenet1_1 = saved
    return dict(seed=SEED, gain=GAIN, tv_keys=[(k, tuple(v.shape)) for k, v in tv_sd.items()], lin=lin, pnet_keys=pnet_keys,
                pairs=pairs, average=avg)


TAPS = [1, 4, 7, 9, 10, 11, 12]          # features index after which relu1..relu7 are taken


def restate(tv_sd, lin, a, b, crop=CROP, dtype=torch.float64, ceil_mode=True, drop_layer=None):
    """A torch restatement of the metric (CPU, `dtype`): uint8 HWC images a, b -> (total, [7 per-layer values]).  ceil_mode /
    drop_layer exist so that tests can show they would see those two mistakes."""
    net = SqueezeNet11()
    net.load_state_dict(tv_sd)
    net = net.to(dtype).eval()
    for m in net.features:
        if isinstance(m, nn.MaxPool2d):
            m.ceil_mode = ceil_mode
    shift = torch.tensor([-.030, -.088, -.188], dtype=torch.float32).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], dtype=torch.float32).view(1, 3, 1, 1)

    def feats(img):
        img = img.numpy() if torch.is_tensor(img) else img
        img = img[crop:img.shape[0] - crop, crop:img.shape[1] - crop, :]
        x = torch.from_numpy((img / 127.5 - 1.0).astype(np.float32)).permute(2, 0, 1)[None].contiguous()
        h, out = ((x - shift) / scale).to(dtype), []
        for i, m in enumerate(net.features):
            h = m(h)
            if i in TAPS:
                out.append(h)
        return out

    with torch.no_grad():
        per_layer = []
        for l, (f0, f1) in enumerate(zip(feats(a), feats(b))):
            n0 = f0 / (f0.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            n1 = f1 / (f1.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
            w = lin["lin%d.model.1.weight" % l].to(dtype).view(1, -1, 1, 1)
            per_layer.append(float(((n0 - n1) ** 2 * w).sum(1).mean()))
    total = sum(v for l, v in enumerate(per_layer) if l != drop_layer)
    return total, per_layer


def main():
    fx = build_fixture()
    torch.save(fx, OUT)
    print("wrote", OUT, {p["name"]: round(p["total"], 6) for p in fx["pairs"]}, "average %.6f" % fx["average"])


if __name__ == "__main__":
    main()
