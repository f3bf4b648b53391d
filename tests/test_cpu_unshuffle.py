"""`use_unshuffle` / `unshuffle_scale` off the device: the option handling (against the live reference's where the build container has
it), BaseModel.setup_unshuffle, the state_dict shapes of the unshuffle nets and the refusals, by name."""
import logging
import types

import pytest
import torch

from oracle import ref_harness as R
from trainner_amd.options import defaults


def opt_with(top=None, net=None, scale=2):
    o = {"scale": scale, "datasets": {"train": {"crop_size": 64}}, "network_G": dict({"type": "esrgan", "nb": 1, "nf": 32}, **(net or {}))}
    o.update(top or {})
    return o


# (top-level keys, network_G keys) -> (unshuffle_scale, in_nc)
OPTION_CASES = {
    "switch+scale": (dict(use_unshuffle=True, unshuffle_scale=2), dict(scale=4), 2, 12),
    "explicit-net-scale": (dict(use_unshuffle=True), dict(scale=4, unshuffle_scale=4), 4, 48),
    "inferred": (dict(use_unshuffle=True), dict(scale=4), 2, 12),
    "net-switch-inferred-x1": (dict(scale=1), dict(unshuffle=True, scale=4), 4, 48),
    "not-inferable": (dict(use_unshuffle=True), dict(), None, 3),
}


@pytest.mark.parametrize("name", list(OPTION_CASES))
def test_options(name):
    top, net, want_s, want_nc = OPTION_CASES[name]
    opt = defaults.get_network_defaults(opt_with(top, net), True)
    assert opt["unshuffle_scale"] == want_s and opt["network_G"]["in_nc"] == want_nc
    assert opt["network_G"]["upscale"] == net.get("scale", opt["scale"]) and "unshuffle_scale" not in opt["network_G"]
    if R.reference_available():
        with R.reference_env():
            import options.defaults as ref_defaults
            ref = ref_defaults.get_network_defaults(opt_with(top, net), True)
        assert ref["unshuffle_scale"] == opt["unshuffle_scale"] and ref["network_G"] == opt["network_G"]


def test_absent_keys_leave_the_parse_unchanged():
    plain = defaults.get_network_defaults(opt_with(), True)
    want = dict(opt_with(), network_G=defaults.get_network_G_config(opt_with()["network_G"], 2, 64))
    assert plain == want and "unshuffle_scale" not in plain and plain["network_G"]["in_nc"] == 3
    for top in (dict(use_unshuffle=False), dict(unshuffle_scale=2), dict(use_unshuffle=False, unshuffle_scale=2)):      # no switch: nothing moves
        assert defaults.get_network_defaults(opt_with(top), True) == dict(want, **top)


def test_setup_unshuffle_and_refusals(caplog):
    from trainner_amd.models.base_model import BaseModel
    from trainner_amd.models.modules.architectures import block as B
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    nets = {s: RRDBNet(3 * s * s, 3, 32, 1, upscale=4) for s in (2, 4)}
    for s, net in nets.items():
        assert tuple(net.state_dict()["model.0.weight"].shape) == (32, 3 * s * s, 3, 3) and net.unshuffle == s
    stub = lambda **opt: types.SimpleNamespace(opt=opt, netG=nets[2], unshuffle=None)
    m = stub(use_unshuffle=True, unshuffle_scale=2)
    with caplog.at_level(logging.INFO, logger="base"):
        BaseModel.setup_unshuffle(m)
    assert isinstance(m.unshuffle, B.SpaceToDepth) and m.unshuffle.bs == 2 and "Pixel Unshuffle wrapper enabled. Scale: 2" in caplog.text
    for opt in (dict(use_unshuffle=True), dict(unshuffle_scale=2), dict(use_unshuffle=False, unshuffle_scale=2)):
        m = stub(**opt)
        BaseModel.setup_unshuffle(m)
        assert m.unshuffle is None
    h = B.SpaceToDepth(2)(torch.zeros(1, 3, 8, 12))
    assert isinstance(h, B.Unshuffled) and h.bs == 2 and h.image.shape == (1, 3, 8, 12)
    # refusals, by name
    with pytest.raises(NotImplementedError, match="grayscale"):
        RRDBNet(16, 1, 32, 1)
    with pytest.raises(NotImplementedError, match="grayscale"):
        BaseModel.setup_unshuffle(types.SimpleNamespace(opt=dict(use_unshuffle=True, unshuffle_scale=2), netG=RRDBNet(4, 1, 32, 1), unshuffle=None))
    with pytest.raises(NotImplementedError, match="in_nc 24"):
        RRDBNet(24, 3, 32, 1)
    with pytest.raises(ValueError, match="plain tensor of 12 channels"):
        nets[2](torch.zeros(1, 12, 8, 8))
    with pytest.raises(ValueError, match="pixel unshuffle of 4"):
        nets[2](B.SpaceToDepth(4)(torch.zeros(1, 3, 8, 8)))
    with pytest.raises(AssertionError, match=r"\(9, 8, 2\)"):
        B.SpaceToDepth(2)(torch.zeros(1, 3, 9, 8))
