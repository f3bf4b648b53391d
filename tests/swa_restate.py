"""Plain-torch restatements of the stochastic-weight-averaging update (trainner_amd/models/swa.py, csrc/optimizers.hip
tnr_swa_update_guarded).  A helper, not a test.

  mean64            the fp64 reference: the running mean with the exact weight 1 / (n + 1);
  update32          fp32, from torch's own CPU functions.  form "avg_fn": what torch.optim.swa_utils.AveragedModel computes on the CPU
                    (a copy for n = 0, then swa_utils.get_swa_avg_fn()) -- bit-equal to AveragedModel (tests/test_cpu_swa.py);
                    form "lerp": torch.lerp with the fp32 weight, what AveragedModel computes on a GPU (_foreach_lerp_) and the form
                    the kernel is written in -- the yardstick of tests/test_gpu_swa.py;
  install           puts the fp32 restatement behind ops.swa_update, as tests/optim_restate.py does for the optimisers (the CPU tests
                    of the host classes run over tests/emul_backend.py, which knows nothing of SWA: tests install both).
"""
import torch
from torch.optim import swa_utils


def mean64(avg64, p, n):
    """avg64 (fp64) after one more update with the snapshot p, n updates made before (avg64 may be None for n = 0)."""
    p = p.double()
    return p.clone() if n == 0 else avg64 + (p - avg64) / (n + 1)


def update32(avg, p, n, form="avg_fn"):
    """avg (fp32) after one more update with p, n updates made before (avg may be None for n = 0); returns a new tensor."""
    if avg is None:
        assert n == 0
        return p.clone()
    if form == "avg_fn":
        return p.clone() if n == 0 else swa_utils.get_swa_avg_fn()(avg, p, torch.tensor(int(n), dtype=torch.long))
    assert form == "lerp", form
    return torch.lerp(avg, p, float(torch.tensor(1.0 / (int(n) + 1), dtype=torch.float32)))


def swa_update(avg, p, n_averaged):
    """ops.swa_update's contract on the CPU: avg is updated in place, p is only read."""
    avg.copy_(update32(avg, p, n_averaged))


def install(monkeypatch, ops):
    monkeypatch.setattr(ops, "swa_update", swa_update)
