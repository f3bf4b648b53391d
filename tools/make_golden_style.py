"""tests/golden/style_loss.pt from the REFERENCE's own GramMatrix (codes/models/modules/loss.py:479-506), FeatureExtractor
(codes/models/modules/architectures/perceptual.py:73-214, over the seeded stub VGG of oracle/stubs) and PerceptualLoss
(codes/models/losses.py:220-340) and, for the step record, its own SRModel -- run on the CPU where the reference tree exists (never on
a GPU machine):

    python tools/make_golden_style.py

Everything is rebuilt from seeds; the file holds probes, the reference's own fp32-vs-fp64 deviations (`e32_*`: the yardsticks of the
GPU tests' tolerances) and scales, not full tensors.

(a) Gram cases GRAM_CASES (C, H, W, N): x uniform in [-1, 1), S (the gradient handed to the Gram matrix, NOT symmetric) likewise.
    G = reference GramMatrix(out_norm='ci')(x), dx = d sum(G * S) / dx, in fp64 and fp32.
(b) Extractor cases EXTRACTOR_CASES: the reference FeatureExtractor with taps TAPS on seeded weights; every tap and the input gradient of
    sum_k sum(fea_k * m_k), m_k seeded maps in [-1, 1).
(c) One PerceptualLoss record: both dictionaries, both weights, on the first extractor case's image pair.
(d) The step record: the harness's small ESRGAN config, two steps of the reference's SRModel with STEP_EXTRA in its train block.

`gram`, `gram_grad`, `extract` and `perceptual_terms` are fp64 restatements in plain torch; the tool asserts each equal to the reference
to 1e-12 (relative to the tensor's scale) before it writes the file, so the tests can compare the engine with the restatements' full
tensors where the reference does not exist.
"""
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import detrand  # noqa: E402
from oracle import ref_harness as R  # noqa: E402
from tools import make_golden_ssim as G  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "style_loss.pt")
GRAM_CASES = ((64, 1, 1, 1), (64, 5, 7, 2), (256, 9, 13, 1), (512, 4, 4, 2), (128, 16, 16, 2), (64, 96, 80, 1))
GRAM_SEED, MAP_SEED, IMG_SEED, VGG_FILL_SEED = 7301, 7411, 7523, 7607
EXTRACTOR_CASES = {"b2_32": (2, 3, 32, 32), "odd_40x24": (1, 3, 40, 24)}
TAPS = ("conv1_2", "relu2_2", "pool2", "conv3_4")
PERC_LAYERS = {"conv1_2": 0.1, "conv3_4": 1.0}
STYLE_LAYERS = {"relu2_2": 1.0, "pool2": 0.5}
STEP_YAML = dict(nb=1, batch=2, crop=64, d_nf=16, pixel_weight=1.0)
STEP_SEED, STEP_K = 463, 2
# With the seeded (not ImageNet) VGG, feature_weight 1 (the harness's value) and these three layers the perceptual term is about 2.8 and
# the unweighted style term about 0.01, the raw L1 pixel distance 0.47: pixel_weight 1 and style_weight 30 put the three at 0.47, 2.8
# and 0.29 -- both feature terms within two orders of magnitude of pix-l1 (asserted in step_record from the first step's values)
STYLE_WEIGHT = 30.0
STEP_EXTRA = ("  style_weight: %g\n  perceptual_opt:\n    perceptual_layers: {conv1_2: 0.1, conv3_4: 1, conv5_4: 1}\n"
              "    style_layers: {relu2_2: 1, relu4_2: 1}") % STYLE_WEIGHT

probe = G.probe


def seeded(shape, seed):
    n = 1
    for s in shape:
        n *= s
    return (detrand.uniform01(n, seed).double().reshape(shape) * 2 - 1).float()


def gram_inputs(case):
    """-> x [N, C, H, W], S [N, C, C], fp32."""
    C, H, W, N = case
    i = GRAM_CASES.index(case)
    return seeded((N, C, H, W), GRAM_SEED + i), seeded((N, C, C), GRAM_SEED + 100 + i)


def extractor_inputs(name):
    """-> x, y images in [0, 1), and the maps m_k of the linear functional are made by tap_maps(shapes)."""
    shape = EXTRACTOR_CASES[name]
    i = sorted(EXTRACTOR_CASES).index(name)
    return (seeded(shape, IMG_SEED + i) + 1) / 2, (seeded(shape, IMG_SEED + 50 + i) + 1) / 2


def tap_maps(feats):
    return {k: seeded(tuple(v.shape), MAP_SEED + i) for i, (k, v) in enumerate(feats.items())}


# ------------------------------------------------------------------------------------------------ restatement
def gram(x):
    N, C, H, W = x.shape
    m = x.reshape(N, C, H * W)
    return torch.einsum("nip,njp->nij", m, m) / (C * H * W)


def gram_grad(x, S):
    """d sum(gram(x) * S) / dx = (S + S^T) x / (C H W)."""
    N, C, H, W = x.shape
    return (torch.einsum("nij,njp->nip", S + S.transpose(1, 2), x.reshape(N, C, H * W)) / (C * H * W)).reshape(x.shape)


def extract(x, sd, taps, net="vgg19"):
    """The listened maps of the VGG `features` stack with the weights of state dict `sd` (keys feature_net.convX_Y.*), in x's dtype."""
    from trainner_amd.models.modules.architectures.perceptual import vgg_layer_names
    mean = torch.tensor([0.485, 0.456, 0.406]).to(x.dtype).view(1, 3, 1, 1)      # the module's fp32 buffers, widened
    std = torch.tensor([0.229, 0.224, 0.225]).to(x.dtype).view(1, 3, 1, 1)
    x = (x - mean) / std
    names = vgg_layer_names(net)
    out = {}
    for n in names[:max(names.index(t) for t in taps) + 1]:
        if n.startswith("conv"):
            x = F.conv2d(x, sd["feature_net.%s.weight" % n].to(x.dtype), sd["feature_net.%s.bias" % n].to(x.dtype), padding=1)
        elif n.startswith("relu"):
            x = F.relu(x)
        else:
            x = F.max_pool2d(x, 2, 2)
        if n in taps:
            out[n] = x
    return out


def perceptual_terms(fx, fy, w_l_p, w_l_s, perceptual_weight, style_weight):
    p = sum(F.l1_loss(fx[k], fy[k]) * w for k, w in w_l_p.items()) * perceptual_weight
    s = sum(F.l1_loss(gram(fx[k]), gram(fy[k])) * w for k, w in w_l_s.items()) * style_weight
    return p, s


def rel_close(a, b, tol=1e-12):
    return (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item())


# ------------------------------------------------------------------------------------------------ the reference
def _reference_modules():
    with R.reference_env():
        for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
            del sys.modules[m]
        from models import losses as RL
        from models.modules import loss as RML
        from models.modules.architectures import perceptual as RP
    return RL, RML, RP


def gram_cases(RML):
    out = {}
    gm = RML.GramMatrix(out_norm="ci")
    for case in GRAM_CASES:
        x, S = gram_inputs(case)
        res = {}
        for dt in (torch.float64, torch.float32):
            xx = x.detach().clone().to(dt).requires_grad_(True)
            g = gm(xx)
            (g * S.to(dt)).sum().backward()
            res[dt] = (g.detach(), xx.grad.detach())
        g64, d64 = res[torch.float64]
        assert rel_close(gram(x.double()), g64) and rel_close(gram_grad(x.double(), S.double()), d64), case
        rec = {"G": probe(g64), "dx": probe(d64), "G_absmax": g64.abs().max().item(), "dx_absmax": d64.abs().max().item(),
               "e32_G": (res[torch.float32][0].double() - g64).abs().max().item(),
               "e32_dx": (res[torch.float32][1].double() - d64).abs().max().item()}
        print("gram %-18s e32_G %.2e (max|G| %.3e)  e32_dx %.2e (max|dx| %.3e)" % (case, rec["e32_G"], rec["G_absmax"], rec["e32_dx"],
                                                                                  rec["dx_absmax"]))
        out[case] = rec
    return out


def reference_extractor(RP, taps):
    with R.reference_env():
        net = RP.FeatureExtractor(listen_list=list(taps), net="vgg19")
    detrand.fill_state_dict_({k: v for k, v in net.state_dict().items() if k.startswith("feature_net")}, VGG_FILL_SEED, gain=1.0, bias_amp=0.05)
    return net


def extractor_cases(RP):
    out = {}
    net = reference_extractor(RP, TAPS)
    keys = [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("feature_net")]
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    for name in EXTRACTOR_CASES:
        x, _ = extractor_inputs(name)
        res = {}
        for dt in (torch.float64, torch.float32):
            net.to(dt)
            xx = x.detach().clone().to(dt).requires_grad_(True)
            feats = net(xx)
            maps = tap_maps(feats)
            sum((feats[k] * maps[k].to(dt)).sum() for k in feats).backward()
            res[dt] = ({k: v.detach() for k, v in feats.items()}, xx.grad.detach())
        net.float()
        f64, d64 = res[torch.float64]
        assert list(f64) == list(TAPS)
        rx = x.double().requires_grad_(True)
        rf = extract(rx, sd, TAPS)
        sum((rf[k] * tap_maps(rf)[k].double()).sum() for k in rf).backward()
        assert all(rel_close(rf[k].detach(), f64[k]) for k in TAPS) and rel_close(rx.grad, d64), name
        rec = {"taps": {k: {"fea": probe(f64[k]), "shape": tuple(f64[k].shape), "absmax": f64[k].abs().max().item(),
                            "e32": (res[torch.float32][0][k].double() - f64[k]).abs().max().item()} for k in TAPS},
               "grad": probe(d64), "grad_absmax": d64.abs().max().item(), "e32_grad": (res[torch.float32][1].double() - d64).abs().max().item()}
        print("extract %-10s" % name, " ".join("%s e32 %.2e/%.2e" % (k, rec["taps"][k]["e32"], rec["taps"][k]["absmax"]) for k in TAPS),
              "grad e32 %.2e/%.2e" % (rec["e32_grad"], rec["grad_absmax"]))
        out[name] = rec
    return out, keys


def perceptual_record(RL, RP):
    import torch.nn as nn
    listen = list(dict(PERC_LAYERS, **STYLE_LAYERS))
    net = reference_extractor(RP, listen)
    opt = {"train": {"feature_weight": 1.0, "style_weight": 2.0,
                     "perceptual_opt": {"perceptual_layers": dict(PERC_LAYERS), "style_layers": dict(STYLE_LAYERS)}}}
    x, y = extractor_inputs("b2_32")
    res = {}
    for dt in (torch.float64, torch.float32):
        net.to(dt)
        pl = RL.PerceptualLoss(criterion=nn.L1Loss(), network=net, opt=opt)
        xx = x.detach().clone().to(dt).requires_grad_(True)
        p, s = pl(xx, y.to(dt))
        (p + s).backward()
        res[dt] = (p.item(), s.item(), xx.grad.detach())
    net.float()
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    rx = x.double().requires_grad_(True)
    rp, rs = perceptual_terms(extract(rx, sd, listen), extract(y.double(), sd, listen), PERC_LAYERS, STYLE_LAYERS, 1.0, 2.0)
    (rp + rs).backward()
    p64, s64, d64 = res[torch.float64]
    assert abs(rp.item() - p64) <= 1e-12 * max(1, abs(p64)) and abs(rs.item() - s64) <= 1e-12 * max(1, abs(s64)) and rel_close(rx.grad, d64)
    rec = {"opt": opt, "percep": p64, "style": s64, "grad": probe(d64), "grad_absmax": d64.abs().max().item(),
           "e32_percep": abs(res[torch.float32][0] - p64), "e32_style": abs(res[torch.float32][1] - s64),
           "e32_grad": (res[torch.float32][2].double() - d64).abs().max().item(),
           "keys": [(k, tuple(v.shape)) for k, v in net.state_dict().items() if k.startswith("feature_net")]}
    print("perceptual: percep %.6f (e32 %.2e) style %.6f (e32 %.2e) grad e32 %.2e/%.2e" % (p64, rec["e32_percep"], s64, rec["e32_style"],
                                                                                          rec["e32_grad"], rec["grad_absmax"]))
    return rec


def style_yaml(path, extra=STEP_EXTRA):
    """Add the lines of `extra` to the train block of a yaml written by oracle.ref_harness.esrgan_yaml."""
    with open(path) as fh:
        txt = fh.read()
    assert txt.count("\nlogger:") == 1
    with open(path, "w") as fh:
        fh.write(txt.replace("\nlogger:", "\n" + extra + "\nlogger:"))
    return path


def step_record():
    from oracle.make_golden import D_SEED, F_SEED, G_SEED, probe_state
    yml = style_yaml(R.esrgan_yaml(name="golden_style", **STEP_YAML))
    opt, model = R.build_reference_model(yml, seed=0)
    names = [l["name"] for l in model.generatorlosses.loss_list]
    assert names == ["pix-l1", "fea-vgg19-l1"], names
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    assert sorted(netF.listen_list) == ["conv1_2", "conv3_4", "conv5_4", "relu2_2", "relu4_2"]
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    logs, terms = [], None
    for s in range(1, STEP_K + 1):
        LR, HR = detrand.synthetic_pair(STEP_YAML["batch"], STEP_YAML["crop"], STEP_SEED + s)
        logs.append(R.reference_step(model, LR, HR, s))
        if s == 1:
            with R.reference_env(), torch.no_grad():
                pl = [l["function"] for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]
                p, st = pl(model.fake_H.detach(), model.real_H)
            terms = {"percep": p.item(), "style": st.item(), "pix": logs[0]["pix-l1"]}      # each with its weight
    print("step", [{k: round(v, 6) for k, v in l.items()} for l in logs], "terms after step 1:", terms)
    for k in ("percep", "style"):
        assert 1e-2 <= terms[k] / terms["pix"] <= 1e2, (k, terms)
    return {"name": "style_step", "spec": {"yaml": dict(STEP_YAML), "steps": STEP_K, "seed": STEP_SEED}, "extra": STEP_EXTRA,
            "loss_names": names, "terms_after_step1": terms,
            "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": STEP_SEED},
            "logs": logs, "fake_H": model.fake_H.detach().clone(),
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()],
            "d_keys": [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()], "torch": torch.__version__}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    RL, RML, RP = _reference_modules()
    ext, keys = extractor_cases(RP)
    fx = {"gram": gram_cases(RML), "extractor": ext, "extractor_keys": keys, "taps": TAPS, "perceptual": perceptual_record(RL, RP),
          "steps": {"style": step_record()}, "torch": torch.__version__}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    print("->", OUT, "%.1f KB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
