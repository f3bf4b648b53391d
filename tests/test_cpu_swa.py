"""Stochastic weight averaging (`use_swa` / swa_*), host side (-m "not gpu", no reference checkout): the restatement the other SWA
tests lean on is torch's own AveragedModel bit for bit, and the option / checkpoint / refusal logic around the averaged model.
The engine side runs over tests/emul_backend.py + tests/swa_restate.py (the C ABI's contract in torch-CPU)."""
import os
import re

import pytest
import torch
from torch.optim.swa_utils import AveragedModel

import emul_backend
import swa_restate
import test_gpu_step as TS
from oracle import ref_harness as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(nb=1, batch=2, crop=64, d_nf=16)


@pytest.fixture
def emulated(monkeypatch):
    from trainner_amd import ops
    emul_backend.install(monkeypatch)
    swa_restate.install(monkeypatch, ops)
    monkeypatch.setattr(TS, "DEV", "cpu")
    torch.set_num_threads(8)


def _edit(yml, repl):
    txt = open(yml).read()
    for a, b in repl:
        assert a in txt, a
        txt = txt.replace(a, b, 1)
    with open(yml, "w") as fh:
        fh.write(txt)
    return yml


SWA_ON = [("use_swa: false", "use_swa: true"), ("  niter: 500000", "  niter: 500000\n  swa_start_iter: 2\n  swa_lr: 5e-5\n  swa_anneal_epochs: 3")]


def _sr_model(tmp_path, repl=SWA_ON, **kw):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = _edit(R.esrgan_yaml(name="swa", out_root=str(tmp_path), gpu_ids="[0]", **dict(KW, **kw)), repl)
    opt = options.parse(yml, is_train=True)
    return opt, create_model(opt, verbose=False)


def test_restatement_is_torchs_averaged_model_bit_for_bit():
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 5, 3), torch.nn.PReLU(5), torch.nn.Linear(7, 3))
    swa = AveragedModel(net)
    avg32 = [p.detach().clone() for p in net.parameters()]
    avg64 = [p.detach().double() for p in net.parameters()]
    for n in range(6):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(1e-3 * torch.randn_like(p))
        swa.update_parameters(net)
        for i, p in enumerate(net.parameters()):
            swa_restate.swa_update(avg32[i], p.detach(), n)
            avg64[i] = swa_restate.mean64(avg64[i], p.detach(), n)
        assert int(swa.n_averaged) == n + 1
        for a, b, c in zip(avg32, swa.module.parameters(), avg64):
            assert torch.equal(a, b.detach())
            assert (a.double() - c).abs().max().item() <= 4 * 2.0 ** -24 * c.abs().max().item()
            # the lerp form (what the kernel computes) is the same mean to fp32 round-off
    a, p = torch.randn(1000), torch.randn(1000)
    assert torch.equal(swa_restate.update32(a, p, 0, "lerp"), p) and torch.equal(swa_restate.update32(a, a.clone(), 7, "lerp"), a)
    for n in (1, 2, 1000):
        d = (swa_restate.update32(a, p, n, "lerp").double() - swa_restate.mean64(a.double(), p, n)).abs().max().item()
        assert d <= 4 * 2.0 ** -24 * 4.0, (n, d)


def test_swa_start_iter_rel_parses(tmp_path):
    from trainner_amd.options import options
    yml = _edit(R.esrgan_yaml(name="rel", out_root=str(tmp_path), gpu_ids="[0]", **KW),
                [("use_swa: false", "use_swa: true"), ("  niter: 500000", "  niter: 400\n  swa_start_iter_rel: 0.75")])
    opt = options.parse(yml, is_train=True)
    assert opt["train"]["swa_start_iter"] == 300 and "swa_start_iter_rel" not in opt["train"] and opt["use_swa"] is True


@pytest.mark.parametrize("use_swa", [False, True])
def test_check_resume_adds_the_swa_file_only_with_use_swa(tmp_path, use_swa):
    from trainner_amd.options import options
    yml = R.esrgan_yaml(name="res", out_root=str(tmp_path), gpu_ids="[0]", **KW)
    _edit(yml, [("path:\n", "path:\n  resume_state: %s\n" % os.path.join(str(tmp_path), "training_state", "7.state"))]
          + ([("use_swa: false", "use_swa: true")] if use_swa else []))
    opt = options.parse(yml, is_train=True)
    options.check_resume(opt)
    assert opt["path"]["pretrain_model_G"].endswith("7_G.pth") and opt["path"]["pretrain_model_D"].endswith("7_D.pth")
    if use_swa:
        assert opt["path"]["pretrain_model_swaG"].endswith(os.path.join("models", "7_swaG.pth"))
    else:
        assert not opt["path"].get("pretrain_model_swaG")


def test_generator_with_batchnorm_is_refused_by_name(tmp_path, emulated):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    yml = _edit(R.i2i_yaml(name="bn", out_root=str(tmp_path), gpu_ids="[0]", model="pix2pix", n_blocks=1, norm_G="batch"),
                [("use_swa: false", "use_swa: true")])
    with pytest.raises(NotImplementedError, match=r"SWA \(use_swa\).*BatchNorm.*ResnetGenerator.*update_bn"):
        create_model(options.parse(yml, is_train=True), verbose=False)
    # the same recipe with the instance-norm generator constructs
    yml = _edit(R.i2i_yaml(name="inorm", out_root=str(tmp_path), gpu_ids="[0]", model="pix2pix", n_blocks=1),
                [("use_swa: false", "use_swa: true")])
    m = create_model(options.parse(yml, is_train=True), verbose=False)
    assert m.swa and int(m.swa_model.n_averaged) == 0 and m.swa_start_iter == 0
    assert all("swa_lr" in g and g["swa_lr"] == 1e-4 for g in m.optimizer_G.param_groups)            # the reference's defaults


def test_cyclegan_ignores_the_switch(tmp_path, emulated):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    kw = dict(model="cyclegan", batch=1, crop=64, n_blocks=1, ngf=16, ndf=16, pixel_weight=10.0, gpu_ids="[0]")
    off = create_model(options.parse(R.i2i_yaml(name="c0", out_root=str(tmp_path / "a"), **kw), is_train=True), verbose=False)
    on = create_model(options.parse(_edit(R.i2i_yaml(name="c1", out_root=str(tmp_path / "b"), **kw), [("use_swa: false", "use_swa: true")]),
                                    is_train=True), verbose=False)
    assert not on.swa and not off.swa and not hasattr(on, "swa_model")
    assert all("swa_lr" not in g for o in on.optimizers for g in o.param_groups)
    lrs = []
    for m in (off, on):
        for s in range(1, 4):
            m.update_learning_rate(s, warmup_iter=-1)
        lrs.append((m.get_current_learning_rate(3), [g["lr"] for o in m.optimizers for g in o.param_groups]))
    assert lrs[0] == lrs[1]


def test_header_binding_and_wrapper_agree_on_the_symbol():
    from trainner_amd import build, hip, ops
    with open(os.path.join(ROOT, "include", "trainner_hip.h")) as fh:
        text = fh.read()
    m = re.search(r"int tnr_swa_update_guarded\(([^)]*)\);", text)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["float *avg", "const float *p", "int64_t n", "float weight", "const uint32_t *fault", "void *stream"]
    import ctypes as C
    res, args = hip._SIGS["tnr_swa_update_guarded"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]
    assert "tnr_swa_update_guarded" in hip.EXPORTS and callable(ops.swa_update)
    assert "optimizers.hip" in build.SOURCES and not any("swa" in s for s in build.SOURCES)          # beside the other guarded launches
    with open(os.path.join(ROOT, "trainner_amd", "csrc", "optimizers.hip")) as fh:
        assert 'extern "C" int tnr_swa_update_guarded(' in fh.read()
    lib = hip.load()          # types every export: a symbol the library lacks raises here
    assert lib.tnr_version() == hip.ABI_VERSION == 3          # additions only


def test_state_dict_layout_and_strict_load(tmp_path, emulated):
    opt, m = _sr_model(tmp_path)
    sd = m.swa_model.state_dict()
    keys = list(sd)
    assert keys[0] == "n_averaged" and keys[1:] == ["module." + k for k in m.netG.state_dict()]
    assert keys == list(AveragedModel(torch.nn.Sequential()).state_dict()) + keys[1:]
    assert sd["n_averaged"].dtype == torch.int64 and sd["n_averaged"].shape == ()
    for k, v in m.netG.state_dict().items():         # before the first update: the generator at construction, in its own storage
        assert torch.equal(sd["module." + k], v) and sd["module." + k].data_ptr() != v.data_ptr() and sd["module." + k].shape == v.shape
    assert m.swa_model.flat.numel() == m.netG.flat_params().flat.numel() and m.swa_model.flat.dtype == torch.float32
    # three updates of a moving generator == the restatement per tensor; n_averaged counts them
    holder = m.netG.flat_params()
    want = {k: v.detach().clone() for k, v in m.netG.state_dict().items()}
    for n in range(3):
        with torch.no_grad():
            for p in m.netG.parameters():          # (the parameters only: the alignment gaps of the flat buffer stay zero, as in training)
                p.add_(1e-3 * (n + 1))
        m.swa_model.update_parameters(m.netG)
        for k, v in m.netG.state_dict().items():
            want[k] = swa_restate.update32(want[k], v.detach(), n)
    sd = m.swa_model.state_dict()
    assert int(sd["n_averaged"]) == 3
    assert all(torch.equal(sd["module." + k], v) for k, v in want.items())
    # strict load: a missing key, an extra key and a wrong shape are errors; a full dict lands bit for bit
    full = {k: v.detach().clone() for k, v in sd.items()}
    other = _sr_model(tmp_path / "b")[1].swa_model
    for broken in ({k: v for k, v in full.items() if k != keys[3]}, dict(full, extra=torch.zeros(1)),
                   dict(full, **{keys[1]: torch.zeros(2, 2)})):
        with pytest.raises(RuntimeError):
            other.load_state_dict(broken, strict=True)
    other.load_state_dict(full, strict=True)
    assert torch.equal(other.flat, m.swa_model.flat) and int(other.n_averaged) == 3 and other._n == 3


def test_lr_regime_and_training_state(tmp_path, emulated):
    """update_learning_rate past swa_start_iter: the average takes the step's weights, the SWA scheduler steps in G's place, D's
    goes on, no warm-up; the .state file carries an empty swa_scheduler list before the regime and the scheduler's state inside it."""
    opt, m = _sr_model(tmp_path)
    twin_p = [torch.nn.Parameter(torch.zeros(1))]
    twin = torch.optim.Adam(twin_p, lr=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(twin, [50000, 100000], 0.5)
    swalr = torch.optim.swa_utils.SWALR(twin, swa_lr=5e-5, anneal_epochs=3, anneal_strategy="cos")
    twin_d = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-4)
    sched_d = torch.optim.lr_scheduler.MultiStepLR(twin_d, [50000, 100000], 0.5)
    os.makedirs(opt["path"]["training_state"], exist_ok=True)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for s in range(1, 7):
            m.update_learning_rate(s, warmup_iter=4)
            sched_d.step()
            if s > 2:
                swalr.step()
            else:
                sched.step()
                twin.param_groups[0]["lr"] = twin_d.param_groups[0]["lr"] = 1e-4 / 4 * s
            assert m.optimizer_G.param_groups[0]["lr"] == twin.param_groups[0]["lr"], s
            assert m.get_current_learning_rate(s) == (swalr.get_last_lr()[0] if s > 2 else sched.get_last_lr()[0])
            assert int(m.swa_model.n_averaged) == max(0, s - 2)
            # D: its own scheduler throughout, warm-up only outside the regime (MultiStepLR carries the last warm-up value on)
            assert m.optimizer_D.param_groups[0]["lr"] == twin_d.param_groups[0]["lr"] == 1e-4 / 4 * min(s, 2)
            if s in (2, 3):
                m.save_training_state(0, s)
                st = torch.load(os.path.join(opt["path"]["training_state"], "%d.state" % s), weights_only=False)
                assert st["swa_scheduler"] == ([] if s == 2 else [m.swa_scheduler.state_dict()])
                assert all("swa_lr" in g for g in st["optimizers"][0]["param_groups"])
    assert m.optimizer_G.param_groups[0]["lr"] == 5e-5            # annealed to swa_lr after 3 epochs
    # use_swa off: the key is absent, as in the reference
    opt0, m0 = _sr_model(tmp_path / "off", repl=[])
    os.makedirs(opt0["path"]["training_state"], exist_ok=True)
    m0.save_training_state(0, 1)
    assert "swa_scheduler" not in torch.load(os.path.join(opt0["path"]["training_state"], "1.state"), weights_only=False)
    assert not m0.swa and not hasattr(m0, "swa_model")


@pytest.mark.parametrize("rank", [0, 1])
def test_swa_file_is_written_by_rank_0_only(tmp_path, emulated, rank):
    opt, m = _sr_model(tmp_path)
    m.update_learning_rate(3)
    m.dp.rank = rank
    m.save(3)
    m.save_training_state(0, 3)
    models = opt["path"]["models"]
    if rank:
        assert not os.path.isdir(models) or os.listdir(models) == []
        assert not os.path.isdir(opt["path"]["training_state"]) or os.listdir(opt["path"]["training_state"]) == []
        return
    assert sorted(os.listdir(models)) == ["3_D.pth", "3_G.pth", "3_swaG.pth"]
    sd = torch.load(os.path.join(models, "3_swaG.pth"), weights_only=False)
    assert list(sd) == list(m.swa_model.state_dict()) and int(sd["n_averaged"]) == 1 and sd["n_averaged"].dtype == torch.int64
    assert all(not v.is_cuda and torch.equal(v, m.swa_model.state_dict()[k].cpu()) for k, v in sd.items())
    # the reference's tool for the file (scripts/swa2normal.py) strips `module.` and drops n_averaged: that loads into the generator
    plain = {k[len("module."):]: v for k, v in sd.items() if k != "n_averaged"}
    m.netG.load_state_dict(plain, strict=True)


def test_swa_generator_swaps_and_restores(tmp_path, emulated):
    opt, m = _sr_model(tmp_path)
    holder = m.netG.flat_params()
    with torch.no_grad():
        holder.flat.add_(0.01)
    m.update_learning_rate(3)
    with torch.no_grad():
        holder.flat.add_(0.01)
    before, v0 = holder.flat.clone(), holder.version
    with m.swa_generator() as g:
        assert g is m.netG and torch.equal(holder.flat, m.swa_model.flat) and not torch.equal(holder.flat, before)
        assert holder.version > v0
        v1 = holder.version
    assert torch.equal(holder.flat, before) and holder.version > v1 and m.netG.flat_params() is holder
    with pytest.raises(ZeroDivisionError):          # restored when the body raises, too
        with m.swa_generator():
            1 / 0
    assert torch.equal(holder.flat, before)


def test_sync_replicas_covers_the_average(tmp_path, emulated, monkeypatch):
    """Data-parallel start state: the averaged buffer and n_averaged are among the tensors every rank takes from rank 0, and the host
    copy of the count follows (stubbed group: the broadcast writes what rank 0 would hold)."""
    opt, m = _sr_model(tmp_path)
    seen = []

    def broadcast(tensors):
        seen.extend(tensors)
        for t in tensors:
            if t.data_ptr() == m.swa_model.flat.data_ptr():
                t.fill_(0.25)
            if t.data_ptr() == m.swa_model.n_averaged.data_ptr():
                t.fill_(5)

    monkeypatch.setattr(m.dp, "active", True)
    monkeypatch.setattr(m.dp, "broadcast_from_rank0", broadcast)
    m.sync_replicas()
    ptrs = {t.data_ptr() for t in seen}
    assert m.swa_model.flat.data_ptr() in ptrs and m.swa_model.n_averaged.data_ptr() in ptrs
    assert int(m.swa_model.n_averaged) == 5 == m.swa_model._n and bool((m.swa_model.flat == 0.25).all())
    # without the switch the list is what it was
    opt0, m0 = _sr_model(tmp_path / "off", repl=[])
    seen0 = []
    monkeypatch.setattr(m0.dp, "active", True)
    monkeypatch.setattr(m0.dp, "broadcast_from_rank0", seen0.extend)
    m0.sync_replicas()
    assert len(seen) == len(seen0) + 2
