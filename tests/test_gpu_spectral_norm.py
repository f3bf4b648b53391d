"""Spectral normalisation on the device (-m gpu): csrc/spectral_norm.hip and the networks and models that run on it, against
tests/golden/spectral_norm.pt (tools/make_golden_spectral_norm.py: the reference's own modules) and the fp64 restatement
(tests/sn_restate.py).

Kernel and network level use the rule for kernels without a derived bound (test_gpu_membound_kernels.yardstick): device error <= 2 x the
fp32 reference's own error + 2e-7 x scale, both against fp64.  The fp32 figure is the golden's (the reference's fp32 run against its
fp64 run, per tensor); `with_error` turns it into the fp32 operand that function takes.  Step level: the bounds of
test_gpu_i2i.test_i2i_step_matches_reference_golden and of test_gpu_step.test_step_matches_reference_golden's esrgan_nb1_unet case.
The network- and step-level bodies also run on the torch-CPU stand-in of the C ABI (tests/test_cpu_spectral_norm.py)."""
import random
from functools import cache

import pytest
import torch

import sn_restate as X
import test_gpu_i2i as TI
import test_gpu_step as TS
from oracle import detrand, fixtures as FX, sr_oracle as O
from test_gpu_membound_kernels import yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -777.25
ALIGN = 64
MISALIGNED = (1, 3)        # matrices whose tensors start one float off a 16-byte boundary: the element-by-element path


@cache
def golden():
    return FX.load("spectral_norm")


def with_error(ref64, e32):
    """An fp32-reference stand-in whose error against ref64 is the recorded e32: ref64 with one element moved by e32."""
    r = ref64.detach().double().clone().reshape(-1)
    r[0] += e32
    return r.view(ref64.shape)


def check(what, got, ref64, e32):
    return yardstick(what, got.detach().reshape(ref64.shape), ref64.double(), with_error(ref64, e32))


@cache
def matrix_reference(i):
    """fp64 restatement of matrix i, computed once and left unchanged."""
    return X.matrix_run(i, torch.float64)


# ---------------------------------------------------------------------------------------------------------------- kernel level
class MatrixTable:
    """Every matrix of X.MATRICES as one job table.  Weights, derived tensors + records, gradient workspace and parameter gradients
    live in four flat buffers pre-filled with SENTINEL; what lies between the tensors must still hold it afterwards."""

    def __init__(self):
        from trainner_amd import ops
        al = lambda n: (n + ALIGN - 1) // ALIGN * ALIGN
        lay, off, roff = [], 0, 0
        for i, (rows, K) in enumerate(X.MATRICES):
            o = off + (1 if i in MISALIGNED else 0)
            r = roff + (1 if i in MISALIGNED else 0)
            lay.append((o, r, r + al(rows) + ALIGN, r + al(rows) + al(K) + 2 * ALIGN))
            off, roff = off + al(rows * K) + ALIGN, roff + al(rows) + al(K) + 4 * ALIGN
        mk = lambda n: torch.full((n,), SENTINEL, dtype=torch.float32, device=DEV)
        self.w, self.wn, self.g, self.dw, self.rec, self.uv = mk(off), mk(off), mk(off), mk(off), mk(roff), mk(roff)
        self.used = {n: torch.zeros(t.numel(), dtype=torch.bool) for n, t in (("wn", self.wn), ("g", self.g), ("dw", self.dw), ("rec", self.rec))}
        layers = []
        for i, ((rows, K), (o, r_u, r_v, r_s)) in enumerate(zip(X.MATRICES, lay)):
            W, u0, v0, G = X.matrix_case(i)
            n = rows * K
            L = dict(w=self.w[o:o + n].view(rows, K), wn=self.wn[o:o + n].view(rows, K), g=self.g[o:o + n].view(rows, K),
                     dw=self.dw[o:o + n].view(rows, K), u=self.uv[r_u:r_u + rows], v=self.uv[r_v:r_v + K],
                     ru=self.rec[r_u:r_u + rows], rv=self.rec[r_v:r_v + K], sig=self.rec[r_s:r_s + 1])
            L["w"].copy_(W.float())
            L["u"].copy_(u0.float())
            L["v"].copy_(v0.float())
            L["g"].copy_(G.float())
            L["dw"].zero_()
            for name in ("wn", "g", "dw"):
                self.used[name][o:o + n] = True
            for a, cnt in ((r_u, rows), (r_v, K), (r_s, 1)):
                self.used["rec"][a:a + cnt] = True
            layers.append(L)
        self.layers = layers
        self.table = ops.SpectralNormTable(layers, torch.device(DEV))

    def run(self):
        from trainner_amd import ops
        for _ in range(X.ITERATIONS):
            ops.sn_forward(self.table, iterate=True)
        ops.sn_backward(self.table)
        torch.cuda.synchronize()
        return self

    def gaps_hold(self):
        for name, mask in self.used.items():
            buf = getattr(self, name).cpu()
            assert bool((buf[~mask] == SENTINEL).all()), name
            assert bool((buf[mask] != SENTINEL).all()), name


def test_kernels_three_iterations_and_correction_under_the_yardstick():
    g = golden()["matrices"]
    t = MatrixTable().run()
    t.gaps_hold()
    for i, ((rows, K), L) in enumerate(zip(X.MATRICES, t.layers)):
        ref = matrix_reference(i)
        tag = "%dx%d " % (rows, K)
        for k, got in (("u", L["u"]), ("v", L["v"]), ("sigma", L["sig"]), ("wn", L["wn"]), ("grad", L["dw"])):
            check(tag + k, got.cpu(), ref[k], g[i][k]["e32"])
        assert torch.equal(L["ru"], L["u"]) and torch.equal(L["rv"], L["v"])         # the record is what sigma was made with
        if rows == 1:
            assert abs(float(L["u"][0])) == 1.0
    # a second backward accumulates: x + x is exact
    from trainner_amd import ops
    before = t.dw.clone()
    ops.sn_backward(t.table)
    mask = t.used["dw"].to(DEV)
    assert torch.equal(t.dw[mask], 2.0 * before[mask])
    t.gaps_hold()


def test_kernels_eval_form_uses_the_stored_vectors():
    """iterate = 0: sigma = u . (W v) from the stored u and v, which stay untouched; the record is their copy."""
    from trainner_amd import ops
    t = MatrixTable()
    u0 = [L["u"].clone() for L in t.layers]
    v0 = [L["v"].clone() for L in t.layers]
    ops.sn_forward(t.table, iterate=False)
    torch.cuda.synchronize()
    for i, L in enumerate(t.layers):
        W, u, v, _ = X.matrix_case(i)
        W, u, v = W.float().double(), u.float().double(), v.float().double()
        wn64, _, _, s64 = X.forward(W, u, v, training=False)
        w32, _, _, s32 = X.forward(W.float(), u.float(), v.float(), training=False)
        tag = "eval %dx%d " % X.MATRICES[i]
        yardstick(tag + "sigma", L["sig"].cpu(), s64.reshape(1), s32.reshape(1))
        yardstick(tag + "wn", L["wn"].cpu(), wn64, w32)
        assert torch.equal(L["u"], u0[i]) and torch.equal(L["v"], v0[i]) and torch.equal(L["ru"], u0[i]) and torch.equal(L["rv"], v0[i])
    t.gaps_hold()


def test_kernels_are_deterministic():
    a, b = MatrixTable().run(), MatrixTable().run()
    for name in ("wn", "rec", "uv", "dw"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---------------------------------------------------------------------------------------------------------------- network level
def build_net(name):
    from trainner_amd.models.modules.architectures import discriminators as D
    fx = golden()["nets"][name]
    cls = D.NLayerDiscriminator if name == "patchgan" else D.UNetDiscriminator
    net = cls(**fx["kw"])
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["keys"]
    net.load_state_dict(FX.initial_state(fx["keys"], fx["seed"]))
    return net.to(DEV).train(), fx


def sn_layers(net):
    return [(n, m) for n, m in net.named_modules() if hasattr(m, "weight_u")]


def check_entry(what, got, e):
    got = got.detach().cpu()
    if "value" in e:
        return check(what, got, e["value"], e["e32"])
    s = got.reshape(-1)[::e["stride"]][:e["samples"].numel()]
    return check(what, s, e["samples"], e["e32"])


def run_sequence(name, swap_generations=False):
    """Two training forwards on different inputs, then both backwards (the first forward's first: its weight generation is no longer
    the live one), then the eval forward after an in-place weight change.  swap_generations: skip putting the first forward's
    generation back -- what an engine without per-forward generations would compute."""
    net, fx = build_net(name)
    x1, x2, g1, g2 = (t.float().to(DEV) for t in X.net_inputs(name))
    x1.requires_grad_(True)
    x2.requires_grad_(True)
    y1 = net(x1)
    uv1 = {n: (m.weight_u.clone(), m.weight_v.clone()) for n, m in sn_layers(net)}
    y2 = net(x2)
    uv2 = {n: (m.weight_u.clone(), m.weight_v.clone()) for n, m in sn_layers(net)}
    if swap_generations:
        net._sn_restore = lambda snap: None
    (y1 * g1).sum().backward()
    (y2 * g2).sum().backward()
    out = dict(y1=y1, y2=y2, gx1=x1.grad, gx2=x2.grad)
    if swap_generations:
        return net, fx, out
    for k, v in out.items():
        check_entry("%s %s" % (name, k), v, fx[k])
    for tag, uv in (("uv1", uv1), ("uv2", uv2)):
        for n, (u, v) in uv.items():
            check_entry("%s %s %s u" % (name, tag, n), u, fx[tag][n][0])
            check_entry("%s %s %s v" % (name, tag, n), v, fx[tag][n][1])
    grads = dict(net.named_parameters())
    assert sorted(grads) == sorted(fx["grads"])
    for k, e in fx["grads"].items():
        check_entry("%s grad %s" % (name, k), grads[k].grad, e)
    # eval forward after an in-place weight change: sigma from the stored vectors and the current weights
    net.eval()
    X.perturb_(net)
    with torch.no_grad():
        ye = net(x1.detach())
    check_entry("%s y_eval" % name, ye, fx["y_eval"])
    for n, m in sn_layers(net):
        assert torch.equal(m.weight_u, uv2[n][0]) and torch.equal(m.weight_v, uv2[n][1]), n
    return net, fx, out


@pytest.mark.parametrize("name", list(X.NETS))
def test_network_two_forwards_two_backwards_and_eval(name):
    run_sequence(name)


@pytest.mark.parametrize("name", list(X.NETS))
def test_network_sequence_fails_with_the_second_forward_s_weights(name):
    """The first backward against the SECOND forward's weights misses the recorded input gradient: the sequence tells the generations
    apart (the golden tool asserts the same of the reference)."""
    _, fx, out = run_sequence(name, swap_generations=True)
    e = fx["gx1"]
    bound = 2.0 * e["e32"] + 2e-7 * e["scale"]
    miss = float((out["gx1"].detach().cpu().double() - e["value"]).abs().max())
    assert miss > 10.0 * bound, (miss, bound)


# ---------------------------------------------------------------------------------------------------------------- step level
def add_key_to_network_D(path):
    with open(path) as f:
        lines = f.read().split("\n")
    i = lines.index("network_D:") + 1
    while lines[i].startswith("  "):
        i += 1
    lines.insert(i, "  spectral_norm: true")
    with open(path, "w") as f:
        f.write("\n".join(lines))
    return path


def _model(make_yaml, yaml_kw, tmp_path):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = add_key_to_network_D(make_yaml(name="engine_sn", out_root=str(tmp_path), gpu_ids="[0]", **yaml_kw))
    opt = options.parse(yml, is_train=True)
    return opt, create_model(opt, verbose=False)


def test_pix2pix_step_with_spectral_norm_matches_reference_golden(tmp_path):
    """test_gpu_i2i.test_i2i_step_matches_reference_golden's body and bounds over the recorded Pix2Pix case with `spectral_norm: true`."""
    from oracle import ref_harness
    fx = golden()["steps"]["pix2pix_sn"]
    opt, model = _model(ref_harness.i2i_yaml, fx["spec"]["yaml"], tmp_path)
    assert dict(opt["network_G"]) == fx["network_G"] and dict(opt["network_D"]) == fx["network_D"]
    assert fx["network_D"]["use_spectral_norm"] is True and list(model.model_names) == fx["model_names"]
    for n, sd in FX.i2i_initial_states(fx).items():
        net = getattr(model, "net" + n)
        assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == fx["keys"][n]
        net.load_state_dict(sd)
    random.seed(fx["seeds"]["pool"])
    for (s, (A, B)), ref_log in zip(FX.i2i_batches(fx), fx["logs"]):
        model.feed_data({"A": A, "B": B, "A_path": ["a"] * A.shape[0]})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("STEP", s, {k: (round(log[k], 6), round(v, 6)) for k, v in ref_log.items()})
        TI.check_logs(log, ref_log, 2e-4 if s < 2 else 3e-3)
        if s == 1:
            for k, ref in fx["images_step1"].items():
                diff = (getattr(model, k).detach().cpu() - ref).abs()
                assert diff.mean().item() <= 2e-5 and diff.max().item() <= 5e-4, (k, diff.mean().item(), diff.max().item())
    for k, ref in fx["images"].items():
        diff = (getattr(model, k).detach().cpu() - ref).abs()
        assert diff.mean().item() <= 1e-2 and diff.max().item() <= 1e-1, (k, diff.mean().item(), diff.max().item())
    lr_steps = 2e-4 * fx["spec"]["steps"]
    for n in fx["model_names"]:
        sd = {k: v.detach().cpu() for k, v in getattr(model, "net" + n).state_dict().items()}
        skip = FX.norm_shadowed_biases(fx["keys"][n], fx["network_G"]["norm_type"]) if n.startswith("G") else ()
        worst, mean, k = FX.state_error(sd, fx["states"][n], skip, lr_steps=lr_steps)
        assert mean < 0.15 and worst < 2.05, (n, k, worst, mean)
        e, k = FX.buffers_error(sd, fx["states"][n])
        assert e < 2e-3, (n, "running stats", k, e)
    # the power-iteration vectors are buffers no optimiser drives: plain comparison with the reference's after the last step
    dsd = {k: v.detach().cpu() for k, v in model.netD.state_dict().items()}
    for k, pr in fx["states"]["D"].items():
        if k.endswith("weight_u") or k.endswith("weight_v"):
            e_s, e_n = FX.probe_error(dsd[k], pr)
            assert max(e_s, e_n) < 2e-3, (k, e_s, e_n)


def test_sr_step_with_spectral_norm_unet_matches_reference_golden(tmp_path):
    """test_gpu_step.test_step_matches_reference_golden's body and the bounds of its esrgan_nb1_unet case (DEFAULT_TOL) over the recorded
    SR case with the spectrally normalised U-Net discriminator."""
    from oracle import ref_harness
    fx = golden()["steps"]["esrgan_unet_sn"]
    T = TS.DEFAULT_TOL
    opt, model = _model(ref_harness.esrgan_yaml, fx["spec"]["yaml"], tmp_path)
    assert dict(opt["network_G"]) == fx["network_G"] and dict(opt["network_D"]) == fx["network_D"]
    assert fx["network_D"]["spectral_norm"] is True
    assert [(k, tuple(v.shape)) for k, v in model.netD.state_dict().items()] == fx["d_keys"]
    g, d, f = FX.initial_states(fx)
    TS.load_initial(model, g, d, f)
    for (s, (LR, HR)), ref_log in zip(FX.batches(fx), fx["logs"]):
        model.feed_data({"LR": LR, "HR": HR})
        model.optimize_parameters(s)
        log = model.get_current_log()
        print("STEP", s, {k: (round(log[k], 6), round(v, 6)) for k, v in ref_log.items()})
        TS.check_logs(log, ref_log, tol=T["log"] if s > 2 else TS.DEFAULT_TOL["log"], d_tol=T["log"] if s > 1 else None)
    ref = fx["fake_H"]
    got = model.fake_H.detach().cpu()
    scale = max(1.0, ref.abs().max().item())
    diff = (got - ref).abs()
    assert diff.mean().item() <= T["fake_mean"] * scale and diff.max().item() <= T["fake_max"] * scale, (diff.mean().item(), diff.max().item())
    _, HR = detrand.synthetic_pair(fx["spec"]["yaml"]["batch"], fx["spec"]["yaml"]["crop"], fx["seeds"]["data"] + fx["spec"]["steps"])
    assert abs(O.psnr_reference(got, HR) - O.psnr_reference(ref, HR)) <= 0.05
    lr_steps = 1e-4 * fx["spec"]["steps"]
    gs = {k: v.detach().cpu() for k, v in model.netG.state_dict().items()}
    worst, mean, k = FX.state_error(gs, fx["g_state"], lr_steps=lr_steps)
    assert mean < T["st_mean"] and worst < T["st_worst"], ("G state", k, worst, mean)
    ds = {k: v.detach().cpu() for k, v in model.netD.state_dict().items()}
    worst, mean, k = FX.state_error(ds, fx["d_state"], FX.bn_shadowed_biases(fx["d_keys"]), lr_steps=lr_steps)
    assert mean < T["st_mean"] and worst < T["st_worst"], ("D state", k, worst, mean)
    # (state_error compares weight_u / weight_v as well, in units of lr * steps: they are not Adam-driven and must simply agree)
    assert model.netD.memoize and model.netD._sn is not None       # the SR model asks for the memo; the net never uses it
    assert model.netD._memo == {}
