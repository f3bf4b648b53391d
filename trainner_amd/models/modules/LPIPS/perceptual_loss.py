"""PerceptualLoss / LPIPS metric (codes/models/modules/LPIPS/perceptual_loss.py:13-45, dist_model.py:29-80) for model='net-lin',
net='squeeze', version='0.1', spatial=False -- the configuration the reference's validation uses (utils/metrics.py:37) -- on the
MI355X engine (networks_basic.PNetLin; kernels in csrc/lpips.hip).

Weights (never a silent random init):
  backbone      `pnet_path`, else the file torchvision's squeezenet1_1(pretrained=True) caches:
                <torch.hub.get_dir()>/checkpoints/squeezenet1_1-b8a52dc0.pth (keys features.N.* -> net.sliceK.N.*)
  linear heads  `model_path`, else $TNR_LPIPS_WEIGHTS/v0.1/squeeze.pth ($TNR_LPIPS_WEIGHTS laid out like the reference's
                models/modules/LPIPS/lpips_weights/), loaded with the reference's strict=False
If either is missing the constructor raises LPIPSWeightsUnavailable (a NotImplementedError) naming both paths it tried;
`allow_random_init=True` (tests, tools) constructs the model anyway so that the caller can load its own weights.
"""
import logging
import os

import numpy as np
import torch

from .networks_basic import PNetLin, torchvision_to_slices

logger = logging.getLogger("base")

TORCHVISION_FILE = "squeezenet1_1-b8a52dc0.pth"
WEIGHTS_ENV = "TNR_LPIPS_WEIGHTS"


class LPIPSWeightsUnavailable(NotImplementedError):
    """The pretrained SqueezeNet backbone or the LPIPS linear heads are not on this machine."""


def backbone_path(pnet_path=None):
    return pnet_path or os.path.join(torch.hub.get_dir(), "checkpoints", TORCHVISION_FILE)


def heads_path(model_path=None, version="0.1", net="squeeze"):
    if model_path:
        return model_path
    root = os.environ.get(WEIGHTS_ENV)
    return os.path.join(root, "v%s" % version, "%s.pth" % net) if root else None


class PerceptualLoss(PNetLin):
    """state_dict = the reference PNetLin's (scaling_layer.*, net.sliceK.N.*, lin{l}.model.1.weight)."""

    def __init__(self, model="net-lin", net="squeeze", colorspace="rgb", spatial=False, use_gpu=True, gpu_ids=None, model_path=None,
                 pnet_path=None, allow_random_init=False, version="0.1"):
        if model != "net-lin":
            raise NotImplementedError("LPIPS model=%r is not implemented by the HIP engine (only 'net-lin')" % (model,))
        if net != "squeeze":
            raise NotImplementedError("LPIPS net=%r is not implemented by the HIP engine (only 'squeeze', the validation metric's)" % (net,))
        if spatial:
            raise NotImplementedError("LPIPS spatial=True is not implemented by the HIP engine (only the spatial mean)")
        if str(version) != "0.1":
            raise NotImplementedError("LPIPS version=%r is not implemented by the HIP engine (only '0.1')" % (version,))
        super().__init__()
        self.use_gpu, self.gpu_ids, self.spatial, self.colorspace = use_gpu, gpu_ids or [0], spatial, colorspace
        self.weights_source = self._load_pretrained(model_path, pnet_path, allow_random_init)

    def _load_pretrained(self, model_path, pnet_path, allow_random_init):
        bpath, lpath = backbone_path(pnet_path), heads_path(model_path)
        have_b, have_l = os.path.isfile(bpath), bool(lpath) and os.path.isfile(lpath)
        if not (have_b and have_l) and not allow_random_init:
            lmsg = lpath if lpath else "$%s/v0.1/squeeze.pth ($%s is not set)" % (WEIGHTS_ENV, WEIGHTS_ENV)
            raise LPIPSWeightsUnavailable(
                "LPIPS(net-lin, squeeze, v0.1) needs two pretrained files: the torchvision SqueezeNet 1.1 backbone at %s (%s) and the "
                "linear heads at %s (%s). Copy torchvision's %s into <torch hub dir>/checkpoints (or pass pnet_path) and point $%s at "
                "a directory laid out like the reference's models/modules/LPIPS/lpips_weights (or pass model_path)."
                % (bpath, "found" if have_b else "missing", lmsg, "found" if have_l else "missing", TORCHVISION_FILE, WEIGHTS_ENV))
        src = {}
        if have_b:
            self.load_torchvision_state(torch.load(bpath, map_location="cpu", weights_only=False))
            src["net"] = bpath
        else:
            src["net"] = "random-init"
        if have_l:
            self.load_heads(torch.load(lpath, map_location="cpu", weights_only=False))
            src["lin"] = lpath
        else:
            src["lin"] = "random-init"
        if "random-init" in src.values():
            logger.warning("LPIPS: weights left at their random init (allow_random_init): %s", src)
        return src

    def load_torchvision_state(self, sd):
        """A torchvision squeezenet1_1 state_dict (features.N.*) into net.sliceK.N.*; every backbone parameter must be present."""
        mapped = torchvision_to_slices(sd)
        own = self.state_dict()
        want = [k for k in own if k.startswith("net.")]
        missing = [k for k in want if k not in mapped]
        if missing:
            raise KeyError("not a torchvision squeezenet1_1 state_dict: missing %s" % missing[:4])
        with torch.no_grad():
            for k in want:
                own[k].copy_(mapped[k])

    def load_heads(self, sd):
        """The reference's lpips_weights/v0.1/squeeze.pth (lin{l}.model.1.weight), with the reference's strict=False load
        (dist_model.py:71)."""
        if not any(k.startswith("lin") for k in sd):
            raise KeyError("no lin{l}.model.1.weight key in the LPIPS head file")
        self.load_state_dict(sd, strict=False)

    # ------------------------------------------------------------------------------------------------------------------------
    def distance_u8(self, img0, img1, crop=0, per_layer=False):
        """LPIPS of uint8 RGB images (HWC or NHWC, tensors or numpy arrays; the reference's im2tensor scaling) cropped by `crop`
        pixels per side -> float64 cpu tensor [N] (and [N, 7] per layer if per_layer)."""
        from ....utils.metrics import _as_batch_u8
        a, b = _as_batch_u8(img0), _as_batch_u8(img1)
        if a.shape != b.shape:
            raise ValueError("Input images must have the same dimensions.")
        if a.shape[3] != 3:
            raise ValueError("LPIPS takes 3-channel images, got %d channels" % a.shape[3])
        total, layers = self.engine_distance(a, b, 0, crop=crop)
        return (total.cpu(), layers.cpu()) if per_layer else total.cpu()

    def forward(self, pred, target, normalize=False):
        """perceptual_loss.py:27-45: pred / target NCHW float [N, 3, H, W] in [-1, 1] ([0, 1] if normalize) -> per-image distances,
        float64 [N] on the device (the reference returns the same values in fp32; its spatial mean keeps image 0 only)."""
        from .... import hip
        for t in (pred, target):
            hip.require_device(t)
            if t.dim() != 4 or t.shape[1] != 3 or t.shape != pred.shape:
                raise ValueError("PerceptualLoss expects two NCHW RGB tensors of one shape")
        a = target.detach().to(torch.float32).contiguous()
        b = pred.detach().to(torch.float32).contiguous()
        return self.engine_distance(a, b, 1, normalize=normalize)[0]


def im2tensor(image, cent=1.0, factor=255.0 / 2.0):
    """perceptual_loss.py:148-151 (CPU helper for tests and tools): uint8 HWC -> float32 [1, C, H, W] in [-1, 1]."""
    return torch.Tensor((image / factor - cent)[:, :, :, np.newaxis].transpose((3, 2, 0, 1)))
