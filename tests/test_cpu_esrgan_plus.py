"""ESRGAN+ residual paths (network_G `plus: true`), host side (-m "not gpu"): the reference's state_dict layout, the new-arch key map,
the option and the factory."""
import torch

from oracle import ref_harness


def test_state_dict_layout_and_key_maps():
    from trainner_amd.models import networks
    from trainner_amd.models.modules.architectures.RRDBNet_arch import RRDBNet
    sd = RRDBNet(3, 3, 64, 2, plus=True).state_dict()
    keys = list(sd)
    for b in range(2):
        for r in (1, 2, 3):
            pre = "model.1.sub.%d.RDB%d." % (b, r)
            mine = [k for k in keys if k.startswith(pre)]
            assert mine[0] == pre + "conv1x1.weight" and mine[1] == pre + "conv1.0.weight" and len(mine) == 11      # first; no conv1x1.bias
            assert keys.index(mine[-1]) - keys.index(mine[0]) == 10                                                   # one contiguous run
            assert tuple(sd[mine[0]].shape) == (32, 64, 1, 1)
    assert len(keys) == len(RRDBNet(3, 3, 64, 2).state_dict()) + 6
    new = networks.mod2normal(networks.normal2mod(sd))
    assert "RRDB_trunk.1.RDB3.conv1x1.weight" in networks.normal2mod(sd)
    assert list(new) == keys and all(new[k] is sd[k] for k in keys)


def test_option_reaches_the_factory(tmp_path, monkeypatch):
    import emul_backend
    from trainner_amd.models import networks
    from trainner_amd.options import options
    emul_backend.install(monkeypatch)
    yml = ref_harness.esrgan_yaml(name="plus", out_root=str(tmp_path), nb=1, crop=64)
    txt = open(yml).read().replace("  type: esrgan\n", "  which_model_G: esrgan\n  plus: true\n")
    open(yml, "w").write(txt)
    opt = options.parse(yml, is_train=True)
    assert opt["network_G"]["plus"] is True and opt["network_G"]["type"] == "rrdb_net"
    net = networks.define_G(opt)
    assert net.plus and tuple(net.model[1].sub[0].RDB2.conv1x1.weight.shape) == (32, 64, 1, 1)
    w = net.model[1].sub[0].RDB1.conv1x1.weight
    assert float(w.detach().std()) < 0.1 * (2.0 / 64) ** 0.5 * 1.5          # the kaiming x 0.1 rule reached it (std 0.1 sqrt(2 / fan_in))
    assert isinstance(w, torch.nn.Parameter) and net.model[1].sub[0].RDB1.conv1x1.bias is None
