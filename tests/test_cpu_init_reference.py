"""Same seed => the reference's initial weights, bit for bit (-m "not gpu"; tests/golden/init_weights.json, oracle/make_golden_init.py:
one SHA-256 per tensor of the reference's own networks, and the live reference as well where its checkout is present).

train.py:107 seeds python / numpy / torch (`util.set_random_seed(manual_seed)`) before `create_model`; the networks are then
built module by module -- every nn.Conv2d / nn.ConvTranspose2d / nn.Linear draws its default init from torch's generator -- and
`networks.init_weights` (kaiming_normal_ x init_scale, networks.py:41-54,71-100) draws again in `Module.apply` order.  The
engine's parameter holders (block.Conv2dHIP, LinearHIP, ResNet_arch.ConvTranspose2dHIP) make the same draws in the same order, so
a run started from scratch with the reference's seed starts from the reference's weights.  Checked for every network kind built:
RRDBNet, SRResNet, Discriminator_VGG, UNetDiscriminator, ResnetGenerator, UnetGenerator, PatchGAN."""
import json
import os
import random

import numpy as np
import pytest
import torch

import emul_backend
from oracle import fixtures as FX, ref_harness as R
from oracle.make_golden_init import CASES, SEED, digest

with open(os.path.join(FX.GOLDEN_DIR, "init_weights.json")) as _f:
    STORED = json.load(_f)


@pytest.mark.parametrize("case", list(CASES))
def test_same_seed_gives_the_reference_initial_weights(case, tmp_path, monkeypatch):
    from trainner_amd.models import create_model
    from trainner_amd.options import options
    emul_backend.install(monkeypatch)
    make, kw, nets = CASES[case]
    ref = None
    if R.reference_available():
        opt, ref = R.build_reference_model(make(name="init", out_root=str(tmp_path / "ref"), **kw), seed=SEED)   # set_random_seed(7)
    eopt = options.parse(make(name="init", out_root=str(tmp_path / "eng"), gpu_ids="[0]", **kw), is_train=True)
    random.seed(SEED)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    eng = create_model(eopt, verbose=False)
    for n in nets:
        a = getattr(eng, "net" + n).state_dict()
        assert list(a) == [e[0] for e in STORED[case][n]], n
        for k, shape, dtype, h in STORED[case][n]:
            assert digest(a[k]) == [shape, dtype, h], (n, k)
        if ref is not None:
            b = getattr(ref, "net" + n).state_dict()
            assert list(a) == list(b)
            for k, v in b.items():
                assert torch.equal(a[k].detach().cpu(), v.detach().cpu()), (n, k)
        w = next(v for k, v in a.items() if k.endswith("weight") and v.dim() == 4)
        assert w.std().item() > 0                                  # (a drawn tensor, not a constant fill)
