"""upsample_mode "upconv" of the image-to-image generators, host side: both construct with the up-conv layers under the expected keys, an
unknown mode still raises, a Pix2Pix and a CycleGAN recipe with `network_G: {upsample_mode: upconv}` reach the constructor through
networks.define_G, and (where the reference checkout is present) the state_dict keys and shapes are the reference's for the same arguments."""
import importlib
import sys

import pytest

from oracle import ref_harness as R

ARGS = {"ResNet_arch.ResnetGenerator": dict(input_nc=3, output_nc=3, ngf=16, norm_type="instance", n_blocks=2),
        "UNet_arch.UnetGenerator": dict(input_nc=3, output_nc=3, num_downs=6, ngf=8, norm_type="batch")}
# Sequential(Upsample, Conv2d): the parameters under child 1 of what was the transposed convolution -> [Cout, Cin, 3, 3]
UP_KEYS = {"ResNet_arch.ResnetGenerator": {"model.12.1.weight": (32, 64, 3, 3), "model.15.1.weight": (16, 32, 3, 3)},
           "UNet_arch.UnetGenerator": {"model.model.3.1.weight": (3, 16, 3, 3), "model.model.1.model.5.1.weight": (8, 32, 3, 3),
                                       "model.model.1.model.3.model.3.model.3.model.3.model.3.1.weight": (64, 64, 3, 3)}}


def engine_class(name):
    mod, cls = name.split(".")
    return getattr(importlib.import_module("trainner_amd.models.modules.architectures." + mod), cls)


@pytest.mark.parametrize("name", list(ARGS))
def test_constructs_and_unknown_mode_raises(name):
    sd = engine_class(name)(upsample_mode="upconv", **ARGS[name]).state_dict()
    for k, shape in UP_KEYS[name].items():
        assert k in sd and tuple(sd[k].shape) == shape, k
    with pytest.raises(NotImplementedError):
        engine_class(name)(upsample_mode="pixelshuffle", **ARGS[name])


@pytest.mark.parametrize("model,which_G,key", [("pix2pix", "unet_128", "model.model.3.1.weight"), ("cyclegan", "resnet_net", "model.12.1.weight")])
def test_recipe_option_reaches_the_generator(model, which_G, key, tmp_path):
    from trainner_amd.models import networks
    from trainner_amd.options import options
    yml = R.i2i_yaml(name="upconv_" + model, model=model, which_G=which_G, out_root=str(tmp_path), crop=128)
    with open(yml) as fh:
        txt = fh.read()
    assert "network_G:\n" in txt
    with open(yml, "w") as fh:
        fh.write(txt.replace("network_G:\n", "network_G:\n  upsample_mode: upconv\n"))
    opt = options.parse(yml, is_train=True)
    assert opt["network_G"]["upsample_mode"] == "upconv"
    net = networks.define_G(opt)                     # (what pix2pix_model.py / cyclegan_model.py call)
    assert key in net.state_dict() and not any("ConvTranspose" in type(m).__name__ for m in net.modules())


@pytest.mark.skipif(not R.reference_available(), reason="reference checkout not present")
@pytest.mark.parametrize("name", list(ARGS))
def test_state_dict_is_the_references(name):
    got = {k: tuple(v.shape) for k, v in engine_class(name)(upsample_mode="upconv", **ARGS[name]).state_dict().items()}
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data")]:
            del sys.modules[m]
        mod, cls = name.split(".")
        ref = getattr(importlib.import_module("models.modules.architectures." + mod), cls)(upsample_mode="upconv", **ARGS[name])
    want = {k: tuple(v.shape) for k, v in ref.state_dict().items()}
    assert list(got) == list(want) and got == want
