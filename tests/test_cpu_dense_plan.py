"""The host-side dispatch of the dense blocks, without a device: ops.dense_block_plan / conv_chain / dense_block replayed against the
table tools/record_dense_plan.py recorded from the dispatch as it was before the plan function existed (tests/golden/dense_plan.json
names the commit), and the one cache of derived weight images (ops._stream_image) under a fake library."""
import json

import pytest
import torch

from tools import record_dense_plan as R
from trainner_amd import hip, ops

with open(R.GOLDEN) as _f:
    TABLE = json.load(_f)


def test_table_covers_the_whole_cross_product():
    assert [tuple(s) for s in TABLE["states"]] == R.STATES
    assert set(TABLE["rows"]) == set(R.KINDS)
    for kind in R.KINDS:
        assert set(TABLE["rows"][kind]) == set(R.MMAS)
        for mma in R.MMAS:
            assert set(TABLE["rows"][kind][mma]) == {R.flips_id(f) for f in R.FLIPS}
            assert all(len(rows) == len(R.STATES) for rows in TABLE["rows"][kind][mma].values())


def _plan_matches(plan, got, st, kind):
    """Is dense_block_plan's answer the form the row's recorded entries show?"""
    form, why = plan
    n = len(st)
    (db, db_counts), (cc, cc_counts) = (part.split("/") for part in got.split(";")[:2])
    per_layer = int(cc_counts.split(",")[1])
    if form in ("split", "sweep") and kind == "unsweepable":          # the late fallback: what the plan says without the sweep
        late = ops.dense_block_plan(st[:4] if form == "split" else st, sweepable=False)
        if form == "split":
            return late == ("chain", None) and db == "chain4+wino" and cc == "chain5"
        form, why = late
    if form == "split":
        return db == "sweep4+wino" and cc == "sweep5" and n == 5
    if form in ("sweep", "chain"):
        return db == cc == "%s%d" % (form, n) and per_layer == 0
    return form == "layers" and db == cc == R.run_of("direct", n) and db_counts == cc_counts and per_layer == (why == "crowded") \
        and why in ("switch", "shape", "calibrated", "crowded")


@pytest.mark.parametrize("mma", list(R.MMAS))
@pytest.mark.parametrize("kind", R.KINDS)
def test_dispatch_equals_the_recorded_table(kind, mma):
    """Every row: the entries dense_block and conv_chain reach, the COUNTERS deltas and the three predicates equal the record, and
    dense_block_plan names that form."""
    lib = R.FakeLib()
    bad = []
    with R.stand_ins(ops, lib):
        for flips in R.FLIPS:
            want = TABLE["rows"][kind][mma][R.flips_id(flips)]
            for state, w in zip(R.STATES, want):
                st = R.configure(ops, lib, kind, mma, flips, state)
                got, plan = R.row(ops, lib, st), ops.dense_block_plan(st)
                if got != w or not _plan_matches(plan, got, st, kind):
                    bad.append((R.flips_id(flips), state, "recorded " + w, "got " + got, plan))
    assert not bad, "%d rows differ from the table recorded at %s; first: %s" % (len(bad), TABLE["recorded_at_commit"], bad[:3])


def test_plan_what_ifs_do_not_touch_the_module(monkeypatch):
    monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    for k, v in R.DEFAULTS.items():
        monkeypatch.setattr(ops, k, v)
    monkeypatch.setattr(ops, "COLLECTIVES_IN_FLIGHT", False)
    monkeypatch.setitem(ops.SWEEP_AUTO_STATE, "choice", None)
    st = R.stages(ops, "chain3", False)
    assert ops.dense_block_plan(st) == ("chain", None)
    assert ops.dense_block_plan(st, crowded=True) == ("layers", "crowded")
    assert ops.COLLECTIVES_IN_FLIGHT is False
    assert ops.dense_block_plan(st) == ("chain", None)
    monkeypatch.setattr(ops, "CONV_CHAIN", False)          # (read at call time)
    assert ops.dense_block_plan(st) == ("layers", "switch")


# ----------------------------------------------------------------------------------------------
# the image cache
# ----------------------------------------------------------------------------------------------
class _Packer:
    def __init__(self):
        self.gen = 1


@pytest.fixture
def fake(monkeypatch):
    lib = R.FakeLib()
    lib.stream = 0
    monkeypatch.setattr(hip, "load", lambda *a, **k: lib)
    monkeypatch.setattr(hip, "stream", lambda: lib.stream)
    saved = {name: dict(d) for name, d in ops._ONEOFF_IMAGES.items()}
    for d in ops._ONEOFF_IMAGES.values():
        d.clear()
    yield lib
    for name, d in ops._ONEOFF_IMAGES.items():
        d.clear()
        d.update(saved[name])


def _packed(owner=None):
    return ops.Packed(torch.zeros(8), 64, 64, ops.PACK_FWD, owner)


def _packs(lib, name="tnr_conv_wq_pack"):
    return sum(1 for c in lib.calls if c[0] == name)


CPU = torch.device("cpu")


def test_image_packed_once_per_owner_generation(fake):
    owner = _Packer()
    wp, d = _packed(owner), hip.ConvDesc()
    a = ops._wq_image(fake, d, wp, CPU)
    b = ops._wq_image(fake, d, wp, CPU)
    assert a is b and a.numel() * 4 == 1024 and _packs(fake) == 1
    owner.gen += 1
    assert ops._wq_image(fake, d, wp, CPU) is a and _packs(fake) == 2
    assert ops._wq_image(fake, d, wp, CPU) is a and _packs(fake) == 2
    assert not ops._wq_oneoff and owner.__dict__["_wq_images"][wp.t.data_ptr()] == [a, 2]


def test_one_off_images_repack_every_call_and_are_kept_per_stream(fake):
    wp, d = _packed(), hip.ConvDesc()
    a = ops._wq_image(fake, d, wp, CPU)
    assert ops._wq_image(fake, d, wp, CPU) is a and _packs(fake) == 2
    fake.stream = 7
    b = ops._wq_image(fake, d, wp, CPU)
    assert b is not a and _packs(fake) == 3 and len(ops._wq_oneoff) == 2
    fake.stream = 0
    assert ops._wq_image(fake, d, wp, CPU) is a and _packs(fake) == 4


def test_one_off_cache_keeps_the_64_most_recently_used(fake):
    d = hip.ConvDesc()
    wps = [_packed() for _ in range(66)]
    imgs = [ops._wq_image(fake, d, wp, CPU) for wp in wps[:64]]
    assert len(ops._wq_oneoff) == 64
    assert ops._wq_image(fake, d, wps[0], CPU) is imgs[0]          # touch the oldest: wps[1] is now the least recently used
    ops._wq_image(fake, d, wps[64], CPU)
    assert len(ops._wq_oneoff) == 64
    assert ops._wq_image(fake, d, wps[0], CPU) is imgs[0]          # kept
    assert ops._wq_image(fake, d, wps[1], CPU) is not imgs[1]       # evicted, built anew (which evicts wps[2])
    assert len(ops._wq_oneoff) == 64
    keys = [k[0] for k in ops._wq_oneoff]
    assert wps[2].t.data_ptr() not in keys and keys[-1] == wps[1].t.data_ptr() and keys[-2] == wps[0].t.data_ptr()
    for i in range(40):          # sweep images share the rule, in a cache of their own
        ops._stream_image(None, "_sweep_images", (i,), 64, CPU, lambda img, nb: None)
        ops._stream_image(None, "_sweep_images", (100 + i,), 64, CPU, lambda img, nb: None)
    assert len(ops._sweep_images) == 64 and len(ops._wq_oneoff) == 64


def test_image_grows_with_need(fake):
    owner, packs = _Packer(), []
    ent, fresh = ops._stream_image(owner, "_wq_images", 1, 1024, CPU, lambda img, nb: packs.append(nb))
    assert fresh and ent[0].numel() == 256
    ent2, fresh2 = ops._stream_image(owner, "_wq_images", 1, 512, CPU, lambda img, nb: packs.append(nb))
    assert ent2 is ent and not fresh2 and packs == [1024]
    ent3, fresh3 = ops._stream_image(owner, "_wq_images", 1, 4096, CPU, lambda img, nb: packs.append(nb))
    assert fresh3 and ent3 is not ent and ent3[0].numel() == 1024 and packs == [1024, 4096]
    assert owner.__dict__["_wq_images"] == {1: ent3}


def test_plain_shuffle_and_wino_images_share_one_dictionary(fake):
    owner = _Packer()
    wp, d = _packed(owner), hip.ConvDesc()
    p = wp.t.data_ptr()
    imgs = [ops._wq_image(fake, d, wp, CPU), ops._wq_image(fake, d, wp, CPU, tag="shuffle2"), ops._wino_image(fake, d, wp, CPU)]
    assert len({id(i) for i in imgs}) == 3
    assert set(owner.__dict__["_wq_images"]) == {p, ("shuffle2", p), ("wino", p)}
    assert _packs(fake) == 2 and _packs(fake, "tnr_conv_wino_pack") == 1
    one = _packed()
    ops._wq_image(fake, d, one, CPU, tag="shuffle2"), ops._wino_image(fake, d, one, CPU)
    assert set(ops._wq_oneoff) == {(("shuffle2", one.t.data_ptr()), 0), (("wino", one.t.data_ptr()), 0)}


def test_sweep_image_lives_on_the_stages_common_owner(fake):
    st = R.stages(ops, "train", False)
    descs = (hip.ConvDesc * 5)()
    img = ops._sweep_image(fake, descs, 5, st, CPU)
    owner = st[0]["wp"].owner
    assert list(owner.__dict__["_sweep_images"]) == [tuple(s["wp"].t.data_ptr() for s in st)] and not ops._sweep_images
    assert ops._sweep_image(fake, descs, 5, st, CPU) is img and _packs(fake, "tnr_conv_sweep_pack") == 1
    ops._sweep_image(fake, (hip.ConvDesc * 4)(), 4, st[:4], CPU)
    assert sorted(len(k) for k in owner.__dict__["_sweep_images"]) == [4, 5]
    st[2] = dict(st[2], wp=_packed())          # a stage packed elsewhere: a one-off image, per stream
    ops._sweep_image(fake, descs, 5, st, CPU)
    assert list(ops._sweep_images) == [(tuple(s["wp"].t.data_ptr() for s in st), 0)]
    fake.sweepable = False
    assert ops._sweep_image(fake, descs, 5, st, CPU) is None
