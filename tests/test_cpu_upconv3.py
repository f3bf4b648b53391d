"""`scale: 3` off the device: the option parse, RRDBNet's x3 state_dict (the reference's keys and shapes), the refusals by name, and the
border proof of the fold: conv_transpose2d over ops.upconv3_fold_weights(w), stride 3, padding 1, IS nearest x3 + the zero-padded 3x3 layer."""
import pytest
import torch
import torch.nn.functional as F

from trainner_amd import ops
from trainner_amd.options import defaults

X3_KEYS = {"model.0": (32, 3, 3, 3), "model.1.sub.1": (32, 32, 3, 3), "model.3": (32, 32, 3, 3), "model.5": (32, 32, 3, 3), "model.7": (3, 32, 3, 3)}


def test_scale3_parses_and_builds_the_reference_state_dict():
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    opt = defaults.get_network_defaults({"scale": 3, "datasets": {"train": {"crop_size": 96}}, "network_G": {"type": "esrgan", "nb": 1, "nf": 32}}, True)
    assert opt["network_G"]["upscale"] == 3
    sd = RRDBNet(3, 3, 32, 1, upscale=3).state_dict()
    heads = {k.rsplit(".", 1)[0] for k in sd if ".RDB" not in k}
    assert heads == set(X3_KEYS) and len([k for k in sd if ".RDB" in k]) == 30
    for k, shape in X3_KEYS.items():
        assert tuple(sd[k + ".weight"].shape) == shape and tuple(sd[k + ".bias"].shape) == shape[:1], k


def test_refusals_are_named():
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    from trainner_amd.models.modules.architectures.SRResNet_arch import SRResNet
    with pytest.raises(NotImplementedError, match=r"upscale 3 with upsample_mode \[pixelshuffle\]"):
        RRDBNet(3, 3, 32, 1, upscale=3, upsample_mode="pixelshuffle")
    with pytest.raises(NotImplementedError, match="use_unshuffle with a scale-3 network"):
        RRDBNet(12, 3, 32, 1, upscale=3)
    with pytest.raises(NotImplementedError, match="built for nf 32 and 64"):
        RRDBNet(3, 3, 96, 1, upscale=3)
    with pytest.raises(NotImplementedError, match="SRResNet upscale 3"):
        SRResNet(3, 3, 64, 1, upscale=3)


@pytest.mark.parametrize("hw", [(1, 1), (4, 5)])
def test_fold_is_the_layer_borders_included(hw):
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(2, 4, *hw, dtype=torch.double, generator=g), torch.randn(6, 4, 3, 3, dtype=torch.double, generator=g)
    want = F.conv2d(F.interpolate(x, scale_factor=3, mode="nearest"), w, padding=1)
    got = F.conv_transpose2d(x, ops.upconv3_fold_weights(w).transpose(0, 1), stride=3, padding=1)
    assert got.shape == want.shape and float((got - want).abs().max()) < 1e-12
