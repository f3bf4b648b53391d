"""Stochastic weight averaging against the LIVE reference (-m "not gpu", build container only; skipped where /root/reference is
absent).  The reference's SWA is torch.optim.swa_utils on the CPU (codes/models/swa.py, base_model.py:174-189,209-214,246-312,
454-500,702-720), so both sides run here: the engine over tests/emul_backend.py + tests/swa_restate.py (the C ABI's contract in
torch-CPU; what is under test is host logic and file formats, the kernel is tests/test_gpu_swa.py's).

Configuration: the small SR recipe of tests/test_cpu_step_options_reference.py with `use_swa: true`, `swa_start_iter: 3`,
`swa_anneal_epochs: 3`, a MultiStepLR milestone at step 2, `update_learning_rate(step, warmup_iter=5)` after every step -- so the
run passes through warm-up, a milestone, the switch to the SWA scheduler, the whole anneal and the constant tail."""
import os
import sys
import warnings

import pytest
import torch

import emul_backend
import swa_restate
import test_gpu_step as TS
from oracle import detrand, fixtures as FX, ref_harness as R

pytestmark = pytest.mark.skipif(not R.reference_available(), reason="needs the reference checkout (build container)")
KW = dict(nb=1, batch=2, crop=64, d_nf=16)
LR_ = 1e-4
WARM = 5
START = 3


@pytest.fixture(autouse=True)
def emulated(monkeypatch):
    from trainner_amd import ops
    emul_backend.install(monkeypatch)
    swa_restate.install(monkeypatch, ops)
    monkeypatch.setattr(TS, "DEV", "cpu")
    torch.set_num_threads(8)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # scheduler.step() before optimizer.step() at construction; SWALR's epoch notes
        yield


def _repl(strategy):
    return [("use_swa: false", "use_swa: true"), ("  lr_steps: [50000, 100000]", "  lr_steps: [2, 100000]"),
            ("  niter: 500000", "  niter: 500000\n  swa_start_iter: %d\n  swa_anneal_epochs: 3\n  swa_anneal_strategy: %s" % (START, strategy))]


def _edit(yml, repl):
    txt = open(yml).read()
    for a, b in repl:
        assert a in txt, a
        txt = txt.replace(a, b, 1)
    with open(yml, "w") as fh:
        fh.write(txt)
    return yml


def _purge_reference_modules():
    for m in [k for k in sys.modules if k.split(".")[0] in ("models", "options", "utils", "dataops", "data", "cv2", "torchvision")]:
        del sys.modules[m]


def _engine_netF(model):
    return [l["function"].network for l in model.generatorlosses.loss_list if "fea" in l["name"]][0]


def _load_netF(netF, f):
    sd = netF.state_dict()
    sd.update(f)
    netF.load_state_dict(sd)


def _both(tmp_path, repl):
    """The same configuration on both sides, the same seeded initial state."""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    ryml = _edit(R.esrgan_yaml(name="swa", out_root=str(tmp_path / "ref"), **KW), repl)
    eyml = _edit(R.esrgan_yaml(name="swa", out_root=str(tmp_path / "eng"), gpu_ids="[0]", **KW), repl)
    ropt, ref = R.build_reference_model(ryml, seed=0)
    eopt = options.parse(eyml, is_train=True)
    eng = create_model(eopt, verbose=False)
    g = detrand.fill_state_dict_({n: v.detach().cpu().clone() for n, v in eng.netG.state_dict().items()}, 101)
    d = detrand.fill_state_dict_({n: v.detach().cpu().clone() for n, v in eng.netD.state_dict().items()}, 202)
    f = FX.vgg_state(77)
    TS.load_initial(eng, g, d, f)
    ref.netG.load_state_dict(g)
    ref.netD.load_state_dict(d)
    _load_netF(R.reference_netF(ref), f)
    return (ropt, ref), (eopt, eng), f


def _step(ref, eng, s, seed=6000):
    """One training step + train.py's update_learning_rate on both sides -> (engine log, reference log)."""
    LR, HR = detrand.synthetic_pair(KW["batch"], KW["crop"], seed + s)
    log_ref = R.reference_step(ref, LR, HR, s)
    with R.reference_env():
        ref.update_learning_rate(s, warmup_iter=WARM)
    eng.feed_data({"LR": LR, "HR": HR})
    eng.optimize_parameters(s)
    log_eng = dict(eng.get_current_log())
    eng.update_learning_rate(s, warmup_iter=WARM)
    return log_eng, log_ref


def _lrs(model, s):
    return [g["lr"] for o in model.optimizers for g in o.param_groups], model.get_current_learning_rate(s)


def _logs_close(a, b, tol=2e-4):
    assert list(a) == list(b), (list(a), list(b))
    for k, v in b.items():
        t = max(tol, 2e-3) if k.startswith("D_") else tol       # raw mean logits behind batch-2 BatchNorms (cf. test_gpu_i2i.check_logs)
        assert abs(a[k] - v) <= t * max(1.0, abs(v)), (k, a[k], v)


def _weights(sd_e, sd_r):
    """(mean, worst) |difference| over the trainable tensors in units of lr (BatchNorm-shadowed conv biases excluded)."""
    skip = FX.bn_shadowed_biases([(k, tuple(v.shape)) for k, v in sd_r.items()])
    tot = n = worst = 0
    for k, v in sd_r.items():
        if v.dtype.is_floating_point and k not in skip and "running" not in k:
            d = (sd_e[k].detach().cpu() - v.detach()).abs()
            tot, n, worst = tot + d.sum().item(), n + d.numel(), max(worst, d.max().item())
    return tot / n / LR_, worst / LR_


def _averaged(model):
    """The averaged generator's tensors under the generator's own keys."""
    return {k[len("module."):]: v for k, v in model.swa_model.state_dict().items() if k != "n_averaged"}


@pytest.mark.parametrize("strategy", ["cos", "linear"])
def test_swa_run_tracks_the_reference(tmp_path, strategy):
    (ropt, ref), (eopt, eng), _ = _both(tmp_path, _repl(strategy))
    assert ref.swa and eng.swa and ref.swa_start_iter == eng.swa_start_iter == START
    assert list(eng.swa_model.state_dict()) == list(ref.swa_model.state_dict())
    rates = []
    for s in range(1, 9):
        le, lr = _step(ref, eng, s)
        print("SWA-REF %s step %d lr %s / %s" % (strategy, s, _lrs(eng, s), _lrs(ref, s)))
        assert _lrs(eng, s) == _lrs(ref, s), (s, _lrs(eng, s), _lrs(ref, s))              # ==: the same torch schedulers on both sides
        rates.append(_lrs(ref, s)[1])
        _logs_close(le, lr, 2e-4 if s == 1 else 3e-3)           # (later steps: trajectory drift of two fp32 implementations, as in the goldens)
        n_ref = int(ref.swa_model.n_averaged)
        assert int(eng.swa_model.n_averaged) == n_ref == max(0, s - START)
        mean, worst = _weights(eng.netG.state_dict(), ref.netG.state_dict())
        print("SWA-REF %s step %d trained  mean %.5f lr  worst %.3f lr" % (strategy, s, mean, worst))
        assert mean <= 0.02 and worst <= 2.05 * s, (s, mean, worst)
        if n_ref:
            # the average of two trajectories cannot differ by more than the trajectories do: the same bounds
            mean, worst = _weights(_averaged(eng), ref.swa_model.module.state_dict())
            print("SWA-REF %s step %d averaged mean %.5f lr  worst %.3f lr" % (strategy, s, mean, worst))
            assert mean <= 0.02 and worst <= 2.05 * s, (s, mean, worst)
    mean, worst = _weights(eng.netD.state_dict(), ref.netD.state_dict())
    assert mean <= 0.02 and worst <= 2.05 * 8, (mean, worst)
    # warm-up (1/5, 2/5, 3/5 of lr; the milestone at 2 halves the scheduler's own value underneath), the SWA scheduler from step 4 on,
    # annealed to swa_lr (the default 1e-4) three steps later and constant from there
    assert rates[3] != rates[2] and rates[6] == rates[7] == pytest.approx(1e-4, rel=1e-12) and len(set(rates)) >= 5, rates


def _save_reference(ref, ropt, it):
    """The reference's save() cannot run here (it moves the averaged model with .cuda()): its pieces, in its order."""
    for key in ("models", "training_state"):
        os.makedirs(ropt["path"][key], exist_ok=True)
    with R.reference_env():
        ref.save_network(ref.netG, "G", it)
        ref.save_network(ref.netD, "D", it)
        ref.save_network(ref.swa_model, "swaG", it)
        ref.save_training_state(0, it)
    return os.path.join(ropt["path"]["training_state"], "%d.state" % it)


def _resume_yaml(yml, state_path):
    txt = open(yml).read().replace("path:\n", "path:\n  resume_state: %s\n" % state_path, 1)
    out = yml.replace(".yml", "_resume.yml")
    with open(out, "w") as fh:
        fh.write(txt)
    return out


def _files_agree(models_dir, it, ref_swa_sd, state, inside):
    sd = torch.load(os.path.join(models_dir, "%d_swaG.pth" % it), weights_only=False)
    assert list(sd) == list(ref_swa_sd) and list(sd)[0] == "n_averaged"
    assert sd["n_averaged"].dtype == ref_swa_sd["n_averaged"].dtype == torch.int64
    assert int(sd["n_averaged"]) == int(ref_swa_sd["n_averaged"]) == (it - START if inside else 0)
    assert all(tuple(sd[k].shape) == tuple(v.shape) and sd[k].dtype == v.dtype for k, v in ref_swa_sd.items())
    assert isinstance(state["swa_scheduler"], list) and len(state["swa_scheduler"]) == (1 if inside else 0)
    assert all("swa_lr" in g for g in state["optimizers"][0]["param_groups"])
    assert all("swa_lr" not in g for g in state["optimizers"][1]["param_groups"])


@pytest.mark.parametrize("at", [2, 5], ids=["before_the_regime", "inside_the_regime"])
def test_swa_checkpoints_interchange_with_the_reference(tmp_path, at):
    """reference -> engine at step `at`, both take step at + 1; then engine -> reference at at + 1, both take step at + 2.
    at = 2: neither file is written inside the regime (3 > swa_start_iter is false): `swa_scheduler` is the empty list and the
    averaged model is the generator at construction; at = 5: n_averaged 2 and 3, the SWA scheduler's state travels."""
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    repl = _repl("cos")
    (ropt, ref), (_, first_eng), f = _both(tmp_path, repl)
    del first_eng
    for s in range(1, at + 1):
        LR, HR = detrand.synthetic_pair(KW["batch"], KW["crop"], 6000 + s)
        R.reference_step(ref, LR, HR, s)
        with R.reference_env():
            ref.update_learning_rate(s, warmup_iter=WARM)
    inside = at > START
    state_path = _save_reference(ref, ropt, at)
    # ---- reference -> engine: train.py:81-104 (check_resume), create_model (load + load_swa), train.py:176-189 (resume_training)
    eyml = _resume_yaml(_edit(R.esrgan_yaml(name="swa", out_root=str(tmp_path / "ref"), gpu_ids="[0]", **KW), repl), state_path)
    eopt = options.parse(eyml, is_train=True)
    resume_state = torch.load(eopt["path"]["resume_state"], weights_only=False)
    options.check_resume(eopt)
    assert eopt["path"]["pretrain_model_swaG"].endswith("%d_swaG.pth" % at)
    eng = create_model(eopt, verbose=False)
    _load_netF(_engine_netF(eng), f)
    eng.resume_training(resume_state)
    eng.update_schedulers(eopt["train"])
    ref_swa_sd = ref.swa_model.state_dict()
    _files_agree(ropt["path"]["models"], at, eng.swa_model.state_dict(), resume_state, inside)
    assert int(eng.swa_model.n_averaged) == int(ref.swa_model.n_averaged) == (at - START if inside else 0)
    for k, v in ref_swa_sd.items():
        assert torch.equal(eng.swa_model.state_dict()[k], v), k
    le, lr = _step(ref, eng, at + 1)
    assert _lrs(eng, at + 1) == _lrs(ref, at + 1), (_lrs(eng, at + 1), _lrs(ref, at + 1))
    _logs_close(le, lr)
    assert int(eng.swa_model.n_averaged) == int(ref.swa_model.n_averaged)
    # ---- engine -> reference at at + 1 (the engine above goes on)
    it = at + 1
    inside = it > START
    eng.save(it)
    eng.save_training_state(0, it)
    state2 = os.path.join(eopt["path"]["training_state"], "%d.state" % it)
    _files_agree(eopt["path"]["models"], it, ref.swa_model.state_dict(), torch.load(state2, weights_only=False), inside)
    ryml = _resume_yaml(_edit(R.esrgan_yaml(name="swa", out_root=str(tmp_path / "ref"), **KW), repl), state2)
    with R.reference_env():
        _purge_reference_modules()
        import options.options as O
        from models import create_model as ref_create
        ropt2 = O.parse(ryml, is_train=True)
        rs = torch.load(ropt2["path"]["resume_state"], weights_only=False)
        O.check_resume(ropt2)
        assert ropt2["path"]["pretrain_model_swaG"].endswith("%d_swaG.pth" % it)
        ref2 = ref_create(ropt2, verbose=False)           # load_swa: the engine's file, strictly
        _load_netF(R.reference_netF(ref2), f)
        ref2.resume_training(rs)
        ref2.update_schedulers(ropt2["train"])
    assert int(ref2.swa_model.n_averaged) == int(eng.swa_model.n_averaged) == (it - START if inside else 0)
    for k, v in eng.swa_model.state_dict().items():
        assert torch.equal(ref2.swa_model.state_dict()[k], v), k
    le, lr = _step(ref2, eng, it + 1)
    assert _lrs(eng, it + 1) == _lrs(ref2, it + 1), (_lrs(eng, it + 1), _lrs(ref2, it + 1))
    _logs_close(le, lr)
    assert int(eng.swa_model.n_averaged) == int(ref2.swa_model.n_averaged) == it + 1 - START
    mean, worst = _weights(_averaged(eng), ref2.swa_model.module.state_dict())
    print("SWA-REF resume at %d: averaged mean %.5f lr  worst %.3f lr" % (at, mean, worst))
    assert mean <= 0.02 and worst <= 2.05 * 2, (mean, worst)
