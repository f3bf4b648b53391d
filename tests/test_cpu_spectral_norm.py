"""Spectral normalisation without a device (-m "not gpu"): the restatement (tests/sn_restate.py) against the reference-generated golden
and by hand, the holder's keys, the options extension, the memo staying off and the per-forward weight generations through the
torch-CPU stand-in of the C ABI (tests/emul_backend.py; the two new entry points ops.sn_forward / ops.sn_backward are restated here on
top of it), and, where the reference's checkout is present, the same-seed initial state and checkpoint interchange with the live
reference."""
import os
import random
import re

import numpy as np
import pytest
import torch

import emul_backend
import sn_restate as X
import test_gpu_i2i as TI
import test_gpu_spectral_norm as G
import test_gpu_step as TS
from oracle import fixtures as FX, ref_harness as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = {"tnr_sn_job_words", "tnr_sn_forward", "tnr_sn_backward"}


# ------------------------------------------------------------------------------------------------ the stand-in's two new entry points
def emul_sn_forward(table, iterate, eps=X.EPS):
    with torch.no_grad():
        for L in table.layers:
            rows = L["w"].shape[0]
            wn, u, v, s = X.forward(L["w"].detach().reshape(rows, -1), L["u"], L["v"], training=bool(iterate), eps=eps)
            L["u"].copy_(u)
            L["v"].copy_(v)
            L["ru"].copy_(u)
            L["rv"].copy_(v)
            L["sig"].copy_(s.reshape(1))
            L["wn"].copy_(wn.view_as(L["wn"]))


def emul_sn_backward(table):
    with torch.no_grad():
        for L in table.layers:
            rows = L["w"].shape[0]
            d = X.grad_correction(L["g"].reshape(rows, -1), L["wn"].reshape(rows, -1), L["ru"], L["rv"], L["sig"][0])
            L["dw"].add_(d.view_as(L["dw"]))


@pytest.fixture
def emulated(monkeypatch):
    from trainner_amd import ops
    emul_backend.install(monkeypatch)
    monkeypatch.setattr(ops, "sn_forward", emul_sn_forward)
    monkeypatch.setattr(ops, "sn_backward", emul_sn_backward)
    for mod in (G, TS, TI):
        monkeypatch.setattr(mod, "DEV", "cpu")
    torch.set_num_threads(8)


# ------------------------------------------------------------------------------------------------ restatement
def test_formulas_by_hand_on_a_2x3_matrix():
    W = torch.tensor([[3.0, 0.0, 4.0], [0.0, 2.0, 0.0]], dtype=torch.float64)
    u0, v0 = torch.tensor([1.0, 0.0], dtype=torch.float64), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    # W^T u0 = (3, 0, 4): v = (0.6, 0, 0.8); W v = (5, 0): u = (1, 0); sigma = u . W v = 5
    Wn, u, v, s = X.forward(W, u0, v0)
    assert torch.allclose(v, torch.tensor([0.6, 0.0, 0.8], dtype=torch.float64), atol=1e-15)
    assert torch.equal(u, torch.tensor([1.0, 0.0], dtype=torch.float64)) and abs(float(s) - 5.0) < 1e-15
    assert torch.allclose(Wn, W / 5.0, atol=1e-16)
    # eval: no iteration, sigma from the stored vectors: u0 . W v0 = (3, 0, 4) . (0, 1, 0) = 0 ... with u0 = (0, 1): 2
    _, ue, ve, se = X.forward(W, torch.tensor([0.0, 1.0], dtype=torch.float64), v0, training=False)
    assert float(se) == 2.0 and torch.equal(ve, v0)
    # G = ones: <G, Wn> = 9 / 5; u v^T = [[0.6, 0, 0.8], [0, 0, 0]]; (G - 1.8 u v^T) / 5
    d = X.grad_correction(torch.ones(2, 3, dtype=torch.float64), Wn, u, v, s)
    want = torch.tensor([[(1 - 1.8 * 0.6) / 5, 0.2, (1 - 1.8 * 0.8) / 5], [0.2, 0.2, 0.2]], dtype=torch.float64)
    assert torch.allclose(d, want, atol=1e-15)
    # a zero matrix: the norms are clamped at eps, nothing divides by zero in the iteration
    uz, vz = X.iterate(torch.zeros(2, 3, dtype=torch.float64), u0, v0)
    assert float(uz.abs().max()) == 0 and float(vz.abs().max()) == 0


def test_restatement_is_autograd_of_the_forward():
    """grad_correction == torch's own derivative of W / sigma(W) with u and v held constant."""
    W, u, v, Gd = X.matrix_case(2)
    W = W.clone().requires_grad_(True)
    Wn, u1, v1, s = X.forward(W.detach(), u, v)
    (W / X.sigma(W, u1, v1)).backward(Gd)
    d = X.grad_correction(Gd, Wn, u1, v1, s)
    assert float((W.grad - d).abs().max()) <= 1e-12 * float(d.abs().max())


def test_restatement_against_the_golden():
    """The fp32 restatement stays within the yardstick the golden records for the reference's fp32 modules: 2 x e32 + 2e-7 x scale."""
    g = G.golden()["matrices"]
    assert len(g) == len(X.MATRICES)
    for i in range(len(X.MATRICES) - 1):          # (the 512 x 4096 matrix: on the device only)
        r64, r32 = G.matrix_reference(i), X.matrix_run(i, torch.float32)
        for k in ("u", "v", "sigma", "wn", "grad"):
            e = float((r32[k].double() - r64[k]).abs().max())
            sc = float(r64[k].abs().max())
            assert abs(sc - g[i][k]["scale"]) <= 1e-12 * sc, (i, k)
            assert e <= 2.0 * g[i][k]["e32"] + 2e-7 * sc, (i, k, e, g[i][k])


def test_exports_declared_and_bound():
    from trainner_amd import hip
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        declared = set(re.findall(r"\b(tnr_[a-z0-9_]+)\s*\(", fh.read()))
    assert NEW_EXPORTS <= declared and NEW_EXPORTS <= set(hip.EXPORTS)
    assert hip.load().tnr_sn_job_words() == 16


# ------------------------------------------------------------------------------------------------ holder, keys, options
def test_key_lists_are_the_reference_s():
    from trainner_amd.models.modules.architectures import discriminators as D
    for name, (kw, _) in X.NETS.items():
        cls = D.NLayerDiscriminator if name == "patchgan" else D.UNetDiscriminator
        net = cls(**kw)
        keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        assert keys == G.golden()["nets"][name]["keys"]
        assert [k for k, _ in net.named_parameters()] == [k for k, _ in keys if not (k.endswith("_u") or k.endswith("_v"))]
        assert not any(k.endswith(".weight") for k, _ in keys if not k.startswith("conv9"))
    for fx, n in ((G.golden()["steps"]["pix2pix_sn"], "D"),):
        net = D.NLayerDiscriminator(**{k: v for k, v in fx["network_D"].items() if k not in ("type", "strict")})
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["keys"][n]
    # what the constructors refused before besides spectral norm stays refused
    for kw in (dict(use_sigmoid=True), dict(get_feats=True), dict(patch=False), dict(norm_layer=torch.nn.InstanceNorm2d)):
        with pytest.raises(NotImplementedError):
            D.NLayerDiscriminator(3, use_spectral_norm=True, **kw)
    with pytest.raises(NotImplementedError):
        D.UNetDiscriminator(5, spectral_norm=True)


def test_init_weights_selects_the_wrapped_layers_and_writes_weight_orig():
    from trainner_amd.models import networks
    from trainner_amd.models.modules.architectures import block as B, discriminators as D
    torch.manual_seed(3)
    net = D.UNetDiscriminator(3, nf=8, spectral_norm=True)
    before = net.conv1.weight_orig.detach().clone()
    assert isinstance(net.conv1, B.SpectralNormConv2dHIP) and "Conv" in type(net.conv1).__name__
    assert abs(float(net.conv1.weight_u.norm()) - 1.0) < 1e-6 and abs(float(net.conv1.weight_v.norm()) - 1.0) < 1e-6
    networks.init_weights(net, init_type="kaiming", scale=0.1)
    assert not torch.equal(net.conv1.weight_orig, before)          # `m.weight` aliases weight_orig until an engine binds it
    assert float(net.conv0.bias.detach().abs().max()) == 0.0


def _parse(tmp_path, d_lines, name):
    from trainner_amd.options import options
    yml = R.esrgan_yaml(name=name, out_root=str(tmp_path / name), gpu_ids="[0]", nb=1, batch=2, crop=64, d_nf=16, d_type="unet")
    txt = open(yml).read().replace("network_D:\n  type: unet\n  nf: 16\n", "network_D:\n  type: unet\n  nf: 16\n" + d_lines)
    open(yml, "w").write(txt)
    return options.parse(yml, is_train=True)


def test_options_forward_the_unet_key_only_when_given(tmp_path):
    plain = _parse(tmp_path, "", "plain")
    assert "spectral_norm" not in plain["network_D"]
    assert dict(plain["network_D"]) == FX.load("esrgan_nb1_unet")["network_D"]        # exactly what the reference parses
    on = _parse(tmp_path, "  spectral_norm: true\n", "sn_on")
    off = _parse(tmp_path, "  spectral_norm: false\n", "sn_off")
    assert on["network_D"]["spectral_norm"] is True and off["network_D"]["spectral_norm"] is False
    assert {k: v for k, v in on["network_D"].items() if k != "spectral_norm"} == dict(plain["network_D"])
    assert dict(on["network_D"]) == G.golden()["steps"]["esrgan_unet_sn"]["network_D"]
    # PatchGAN: the reference's parser forwards the key itself
    fx = G.golden()["steps"]["pix2pix_sn"]
    from trainner_amd.options import options
    yml = G.add_key_to_network_D(R.i2i_yaml(name="p2p", out_root=str(tmp_path / "p2p"), gpu_ids="[0]", **fx["spec"]["yaml"]))
    assert dict(options.parse(yml, is_train=True)["network_D"]) == fx["network_D"]


# ------------------------------------------------------------------------------------------------ engine host logic on the stand-in
def _loose_yardstick(monkeypatch):
    """The stand-in computes with torch's fp32 CPU operators in another order than the reference's modules: its figures are printed
    and bounded at 20 x the device's yardstick (the device test holds the yardstick itself)."""
    def y(what, got, ref64, ref32):
        scale = float(ref64.abs().max())
        e, e32 = float((got.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
        assert e <= 20.0 * (2.0 * e32 + 2e-7 * scale), (what, e, e32, scale)
        return e, e32
    monkeypatch.setattr(G, "yardstick", y)


@pytest.mark.parametrize("name", list(X.NETS))
def test_network_sequence_on_the_stand_in(name, emulated, monkeypatch):
    _loose_yardstick(monkeypatch)
    net, fx, _ = G.run_sequence(name)
    assert net._sn is not None and net._sn.gen >= 3          # two training generations and the eval one


@pytest.mark.parametrize("name", list(X.NETS))
def test_network_sequence_tells_the_generations_apart_on_the_stand_in(name, emulated):
    G.test_network_sequence_fails_with_the_second_forward_s_weights(name)


def test_memo_stays_off_and_every_training_forward_iterates(emulated):
    net, fx = G.build_net("unet")
    net.memoize = True                                       # what the SR model sets on its discriminator
    x = X.net_inputs("unet")[0].float()
    with torch.no_grad():
        y1 = net(x)
        u1 = net.conv3.weight_u.clone()
        y2 = net(x)                                          # same tensor, same parameters: not a repeat
    assert net._memo == {}
    assert not torch.equal(u1, net.conv3.weight_u) and not torch.equal(y1, y2)
    net.eval()
    with torch.no_grad():
        y3, u3 = net(x), net.conv3.weight_u.clone()
        y4 = net(x)
    assert torch.equal(y3, y4) and torch.equal(u3, net.conv3.weight_u)
    from trainner_amd.models.modules.architectures import discriminators as D
    plain = D.UNetDiscriminator(3, nf=16).train()
    plain.memoize = True
    with torch.no_grad():
        plain(x)
    assert len(plain._memo) == 1                             # the memo itself is as it was


def test_freeze_prefixes_match_weight_orig(emulated):
    from trainner_amd.models.base_model import BaseModel
    net, _ = G.build_net("patchgan")
    BaseModel.requires_grad(None, net, False, target_layer=0, net_type="D")
    frozen = [k for k, p in net.named_parameters() if not p.requires_grad]
    assert frozen == ["model.0.bias", "model.0.weight_orig"]
    fp = net.flat_params()                                   # FlatParams carries weight_orig like any parameter
    assert all(p._tnr_flat[0] is fp for p in net.parameters()) and sum(n for _, _, n in fp.offsets) == sum(p.numel() for p in net.parameters())


def test_state_dict_round_trip_through_a_file(emulated, tmp_path):
    a, _ = G.build_net("patchgan")
    x = X.net_inputs("patchgan")[0].float()
    with torch.no_grad():
        a(x)
    path = str(tmp_path / "d.pth")
    torch.save(a.state_dict(), path)
    from trainner_amd.models.modules.architectures import discriminators as D
    b = D.NLayerDiscriminator(**X.NETS["patchgan"][0])
    b.load_state_dict(torch.load(path), strict=True)
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k
    a.eval(), b.eval()
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


def test_pix2pix_step_on_the_stand_in(emulated, tmp_path):
    G.test_pix2pix_step_with_spectral_norm_matches_reference_golden(tmp_path)


def test_sr_step_on_the_stand_in(emulated, tmp_path):
    G.test_sr_step_with_spectral_norm_unet_matches_reference_golden(tmp_path)


# ------------------------------------------------------------------------------------------------ the live reference (build container)
needs_reference = pytest.mark.skipif(not R.reference_available(), reason="the reference's checkout is not present")


def _reference_discriminators():
    import sys
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        from models import networks as RN
        from models.modules.architectures import discriminators as RD
    return RD, RN


def _seed(s):
    random.seed(s)
    np.random.seed(s)
    torch.manual_seed(s)


@needs_reference
@pytest.mark.parametrize("name", list(X.NETS))
def test_same_seed_initial_state_is_the_live_reference_s(name):
    """Construction draws (weight, bias, u, v per layer) and networks.init_weights (which writes through `m.weight` into weight_orig's
    storage on both sides) leave the same weight_orig, weight_u, weight_v and biases, bit for bit."""
    from trainner_amd.models import networks as EN
    from trainner_amd.models.modules.architectures import discriminators as ED
    RD, RN = _reference_discriminators()
    kw = X.NETS[name][0]
    _seed(7)
    ref = (RD.NLayerDiscriminator if name == "patchgan" else RD.UNetDiscriminator)(**kw)
    with R.reference_env():
        RN.init_weights(ref, init_type="kaiming", scale=0.1)
    _seed(7)
    eng = (ED.NLayerDiscriminator if name == "patchgan" else ED.UNetDiscriminator)(**kw)
    EN.init_weights(eng, init_type="kaiming", scale=0.1)
    a, b = eng.state_dict(), ref.state_dict()
    assert list(a) == list(b)
    for k in b:
        assert torch.equal(a[k], b[k]), k
    assert any(k.endswith("weight_orig") for k in a) and float(a[[k for k in a if k.endswith("weight_orig")][0]].std()) > 0


@needs_reference
@pytest.mark.parametrize("name", list(X.NETS))
def test_checkpoints_interchange_with_the_live_reference(name, emulated, tmp_path):
    """A file the reference wrote loads into the engine and the other way round (strict; torch's load pre-hook of the wrapped layers
    takes the three keys without version metadata), and both then compute the same eval forward."""
    from trainner_amd.models.modules.architectures import discriminators as ED
    RD, _ = _reference_discriminators()
    kw = X.NETS[name][0]
    x = X.net_inputs(name)[0].float()
    mk_r = lambda: (RD.NLayerDiscriminator if name == "patchgan" else RD.UNetDiscriminator)(**kw)
    mk_e = lambda: (ED.NLayerDiscriminator if name == "patchgan" else ED.UNetDiscriminator)(**kw)
    # reference -> engine
    _seed(11)
    ref = mk_r().train()
    with torch.no_grad():
        ref(x)                                               # one iteration: u, v away from their initial draws
    p1 = str(tmp_path / "ref.pth")
    torch.save(ref.state_dict(), p1)
    eng = mk_e()
    eng.load_state_dict(torch.load(p1), strict=True)
    ref.eval(), eng.eval()
    with torch.no_grad():
        d = float((eng(x) - ref(x)).abs().max())
    assert d <= 1e-5, d
    # engine -> reference: plain tensors, no _metadata version entry for the wrapped layers
    _seed(12)
    eng2 = mk_e().train()
    with torch.no_grad():
        eng2(x)
    p2 = str(tmp_path / "eng.pth")
    torch.save({k: v.clone() for k, v in eng2.state_dict().items()}, p2)
    ref2 = mk_r()
    ref2.load_state_dict(torch.load(p2), strict=True)
    ref2.eval(), eng2.eval()
    with torch.no_grad():
        d = float((eng2(x) - ref2(x)).abs().max())
    assert d <= 1e-5, d
