"""tests/golden/spectral_norm.pt from the REFERENCE's own spectrally normalised modules (block.add_spectral_norm = torch.nn.utils.
spectral_norm in its hook form; discriminators.NLayerDiscriminator / UNetDiscriminator; the Pix2Pix and SR models) -- run on the CPU
where the reference tree exists (never on a GPU machine):

    python tools/make_golden_spectral_norm.py

Recorded:
  * matrices: for every matrix of tests/sn_restate.py MATRICES, after ITERATIONS training forwards and the backward of a planted G, the
    reference's OWN fp32 deviation from its fp64 run for u, v, sigma, the scaled weight and weight_orig's gradient (e32, the yardstick
    of the GPU tests), with the fp64 scale (max |.|).  The fp64 values themselves are the restatement's, recomputed by the tests.
  * nets: for the two networks of sn_restate.NETS, the state-dict key / shape list and the fill seed of the initial state; two training
    forwards on different inputs followed by both backwards -- outputs, input gradients, u and v after each forward (whole tensors,
    fp64), samples of the weight_orig / bias gradients -- and one eval forward after an in-place weight change; every entry with the
    reference's fp32-vs-fp64 error and scale.
  * steps: two steps of Pix2Pix with `spectral_norm: true` on its PatchGAN (oracle/make_golden_i2i.py pix2pix_rn2_crop64's spec) and of
    the SR model with the spectrally normalised U-Net discriminator (oracle/make_golden.py esrgan_nb1_unet's spec; the reference's
    parser drops the key for `unet`, so it is set on the parsed options, which get_network passes to the constructor), in the layout of
    those tools' files.

Asserted before the file is written:
  * restatement == reference to 1e-12 of the tensor's scale in fp64, for every matrix and every recorded tensor of it
  * every yardstick is non-zero (but u of the one-row matrix, which is exactly +-1 in fp32 and fp64 alike)
  * a backward of the first forward run with the SECOND forward's weights misses the recorded input gradient by more than ten
    times the bound of the GPU test (the two weight generations are told apart)
  * the eval forward leaves u and v unchanged
"""
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in (ROOT, os.path.join(ROOT, "tests")):
    if d not in sys.path:
        sys.path.insert(0, d)

from oracle import detrand, fixtures as FX, ref_harness as R  # noqa: E402
from oracle.make_golden import CASES as SR_CASES, D_SEED, F_SEED, G_SEED, probe_state  # noqa: E402
from oracle.make_golden_i2i import CASES as I2I_CASES, POOL_SEED, SEEDS as I2I_SEEDS, ab_pair  # noqa: E402
import sn_restate as X  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "spectral_norm.pt")
NSAMPLE = 256
STEPS = 2


def _purge():
    for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
        del sys.modules[m]


def _reference_modules():
    with R.reference_env():
        _purge()
        from models.modules.architectures import block as RB, discriminators as RD
    return RB, RD


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def scale_of(t):
    return float(t.double().abs().max())


def sample(t):
    f = t.detach().double().reshape(-1)
    stride = max(1, f.numel() // NSAMPLE)
    return {"samples": f[::stride][:NSAMPLE].clone(), "stride": stride}


# ------------------------------------------------------------------------------------------------ matrices
def reference_matrix_run(RB, i, dtype):
    W, u, v, G = (t.to(dtype) for t in X.matrix_case(i))
    rows, K = W.shape
    m = RB.add_spectral_norm(torch.nn.Conv2d(K, rows, 1, bias=False).to(dtype), True)
    with torch.no_grad():
        m.weight_orig.copy_(W.view(rows, K, 1, 1))
        m.weight_u.copy_(u)
        m.weight_v.copy_(v)
    m.train()
    x = torch.ones(1, K, 1, 1, dtype=dtype)
    for _ in range(X.ITERATIONS):
        m(x)
    wn = m.weight                                   # the derived tensor of the last forward, with its graph
    wn.backward(G.view_as(wn))
    s = torch.dot(m.weight_u, m.weight_orig.detach().view(rows, K).mv(m.weight_v))
    return dict(u=m.weight_u.detach().clone(), v=m.weight_v.detach().clone(), sigma=s.reshape(1), wn=wn.detach().view(rows, K).clone(),
                grad=m.weight_orig.grad.view(rows, K).clone())


def matrices(RB):
    out = []
    for i, (rows, K) in enumerate(X.MATRICES):
        r64, r32, x64 = reference_matrix_run(RB, i, torch.float64), reference_matrix_run(RB, i, torch.float32), X.matrix_run(i, torch.float64)
        rec = {}
        for k in ("u", "v", "sigma", "wn", "grad"):
            sc = scale_of(r64[k])
            assert err(r64[k], x64[k]) <= 1e-12 * sc, (i, k, err(r64[k], x64[k]), sc)
            rec[k] = {"e32": err(r32[k], r64[k]), "scale": sc}
            if rows == 1 and k == "u":      # x / |x| of one element: exactly +-1 in every precision, the one yardstick that is zero
                assert abs(float(r64["u"][0])) == 1.0 and abs(float(r32["u"][0])) == 1.0 and rec[k]["e32"] == 0
            else:
                assert rec[k]["e32"] > 0, (i, k)
        out.append(rec)
        print("matrix %-12s" % ("%dx%d" % (rows, K)), " ".join("%s %.2e/%.2e" % (k, v["e32"], v["scale"]) for k, v in rec.items()))
    return out


# ------------------------------------------------------------------------------------------------ networks
def reference_net_run(RD, name, dtype, state):
    kw, _ = X.NETS[name]
    cls = RD.NLayerDiscriminator if name == "patchgan" else RD.UNetDiscriminator
    net = cls(**kw)
    net.load_state_dict(state)
    net = net.to(dtype).train()
    x1, x2, g1, g2 = (t.to(dtype) for t in X.net_inputs(name))
    x1.requires_grad_(True)
    x2.requires_grad_(True)
    sn = [(n, m) for n, m in net.named_modules() if hasattr(m, "weight_u")]
    rec = {}
    y1 = net(x1)
    rec["uv1"] = {n: (m.weight_u.clone(), m.weight_v.clone()) for n, m in sn}
    y2 = net(x2)
    rec["uv2"] = {n: (m.weight_u.clone(), m.weight_v.clone()) for n, m in sn}
    assert tuple(y1.shape) == tuple(g1.shape), (y1.shape, g1.shape)
    (y1 * g1).sum().backward()
    (y2 * g2).sum().backward()
    rec["y1"], rec["y2"], rec["gx1"], rec["gx2"] = y1.detach(), y2.detach(), x1.grad.clone(), x2.grad.clone()
    rec["grads"] = {k: p.grad.clone() for k, p in net.named_parameters()}
    # the first forward's backward with the second forward's weights (eval mode: sigma from the stored u, v = those of forward 2)
    net.eval()
    xw = x1.detach().clone().requires_grad_(True)
    (net(xw) * g1).sum().backward()
    rec["gx1_wrong"] = xw.grad.clone()
    # one eval forward after an in-place weight change
    with torch.no_grad():
        X.perturb_(net)
        rec["y_eval"] = net(x1.detach()).clone()
    for n, m in sn:
        assert torch.equal(m.weight_u, rec["uv2"][n][0]) and torch.equal(m.weight_v, rec["uv2"][n][1]), n
    return rec, net


def entry(a64, a32, whole):
    e = {"e32": err(a32, a64), "scale": scale_of(a64)}
    assert e["e32"] > 0 or (a64.numel() == 1 and abs(float(a64)) == 1.0)        # (u of a one-row layer: exactly +-1)
    e.update({"value": a64.detach().clone()} if whole else sample(a64))
    return e


def nets(RD):
    out = {}
    for name, (kw, shape) in X.NETS.items():
        torch.manual_seed(X.NET_SEED)
        cls = RD.NLayerDiscriminator if name == "patchgan" else RD.UNetDiscriminator
        fresh = cls(**kw)
        keys = [(k, tuple(v.shape)) for k, v in fresh.state_dict().items()]
        state = FX.initial_state(keys, X.NET_SEED)
        r64, _ = reference_net_run(RD, name, torch.float64, state)
        r32, _ = reference_net_run(RD, name, torch.float32, state)
        rec = {"keys": keys, "seed": X.NET_SEED, "kw": kw, "shape": shape}
        for k in ("y1", "y2", "gx1", "gx2", "y_eval"):
            rec[k] = entry(r64[k], r32[k], whole=True)
        for f in ("uv1", "uv2"):
            rec[f] = {n: (entry(r64[f][n][0], r32[f][n][0], True), entry(r64[f][n][1], r32[f][n][1], True)) for n in r64[f]}
        rec["grads"] = {k: entry(r64["grads"][k], r32["grads"][k], whole=False) for k in r64["grads"]}
        bound = 2.0 * rec["gx1"]["e32"] + 2e-7 * rec["gx1"]["scale"]
        wrong = err(r64["gx1_wrong"], r64["gx1"])
        assert wrong > 10.0 * bound, (name, wrong, bound)
        rec["wrong_generation"] = {"error": wrong, "bound": bound}
        out[name] = rec
        print("net %-9s %d keys; gx1 e32 %.2e scale %.2e; second generation's weights miss gx1 by %.2e (bound %.2e)" % (
            name, len(keys), rec["gx1"]["e32"], rec["gx1"]["scale"], wrong, bound))
    return out


# ------------------------------------------------------------------------------------------------ steps
def add_key_to_network_D(path):
    """`spectral_norm: true` as the last line of the file's network_D block."""
    with open(path) as f:
        lines = f.read().split("\n")
    i = lines.index("network_D:") + 1
    while lines[i].startswith("  "):
        i += 1
    lines.insert(i, "  spectral_norm: true")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


def pix2pix_steps():
    spec = dict(I2I_CASES["pix2pix_rn2_crop64"], steps=STEPS)
    yml = add_key_to_network_D(R.i2i_yaml(name="golden_pix2pix_sn", **spec["yaml"]))
    opt, model = R.build_reference_model(yml, seed=0)
    assert opt["network_D"]["use_spectral_norm"] is True
    names = list(model.model_names)
    for n in names:
        detrand.fill_state_dict_(getattr(model, "net" + n).state_dict(), I2I_SEEDS[n])
    batch, crop = spec["yaml"]["batch"], spec["yaml"]["crop"]
    random.seed(POOL_SEED)
    logs = []
    with R.reference_env():
        for s in range(1, spec["steps"] + 1):
            A, B = ab_pair(batch, crop, spec["seed"] + s)
            model.feed_data({"A": A, "B": B, "A_path": ["a"] * batch})
            model.optimize_parameters(s)
            logs.append(dict(model.get_current_log()))
            if s == 1:
                imgs1 = {"fake_B": model.fake_B.detach().clone()}
    keys = {n: [(k, tuple(v.shape)) for k, v in getattr(model, "net" + n).state_dict().items()] for n in names}
    assert any(k.endswith("weight_orig") for k, _ in keys["D"]) and not any(k.endswith(".weight") for k, _ in keys["D"])
    for l in logs:
        print("    pix2pix", {k: round(v, 6) for k, v in l.items()})
    return {"name": "pix2pix_sn", "spec": spec, "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": dict(I2I_SEEDS, data=spec["seed"], pool=POOL_SEED), "model_names": names, "logs": logs,
            "images": {"fake_B": model.fake_B.detach().clone()}, "images_step1": imgs1,
            "states": {n: probe_state(getattr(model, "net" + n).state_dict()) for n in names}, "keys": keys}


def sr_steps():
    spec = dict(SR_CASES["esrgan_nb1_unet"], steps=STEPS)
    yml = add_key_to_network_D(R.esrgan_yaml(name="golden_esrgan_unet_sn", **spec["yaml"]))
    import contextlib
    with R.reference_env():
        _purge()
        import options.options as O
        from models import create_model
        from utils import util
        with open(os.devnull, "w") as dn, contextlib.redirect_stdout(dn):
            opt = O.parse(yml, is_train=True)
        assert "spectral_norm" not in opt["network_D"]          # the reference's parser drops the key for `unet`
        opt["network_D"]["spectral_norm"] = True
        util.set_random_seed(0)
        model = create_model(opt, verbose=False)
    detrand.fill_state_dict_(model.netG.state_dict(), G_SEED)
    detrand.fill_state_dict_(model.netD.state_dict(), D_SEED)
    netF = R.reference_netF(model)
    detrand.fill_state_dict_({k: v for k, v in netF.state_dict().items() if k.startswith("feature_net")}, F_SEED, gain=1.0, bias_amp=0.05)
    crop, batch = spec["yaml"]["crop"], spec["yaml"]["batch"]
    logs = []
    for s in range(1, spec["steps"] + 1):
        LR, HR = detrand.synthetic_pair(batch, crop, spec["seed"] + s)
        logs.append(R.reference_step(model, LR, HR, s))
    d_keys = [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()]
    assert any(k.endswith("weight_orig") for k, _ in d_keys) and "conv9.weight" in dict(d_keys)
    for l in logs:
        print("    sr", {k: round(v, 6) for k, v in l.items()})
    return {"name": "esrgan_unet_sn", "spec": spec, "network_G": dict(opt["network_G"]), "network_D": dict(opt["network_D"]),
            "seeds": {"G": G_SEED, "D": D_SEED, "F": F_SEED, "data": spec["seed"]}, "logs": logs, "fake_H": model.fake_H.detach().clone(),
            "g_state": probe_state(model.netG.state_dict()), "d_state": probe_state(model.netD.state_dict()),
            "g_keys": [(k, tuple(v.shape)) for k, v in model.netG.state_dict().items()], "d_keys": d_keys}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    RB, RD = _reference_modules()
    fx = {"torch": torch.__version__, "matrices": matrices(RB), "nets": nets(RD),
          "steps": {"pix2pix_sn": pix2pix_steps(), "esrgan_unet_sn": sr_steps()}}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    torch.save(fx, OUT)
    size = os.path.getsize(OUT)
    assert size < 900 * 1024, size
    print("->", OUT, "%.1f KB" % (size / 1024))


if __name__ == "__main__":
    main()
