"""The host-side dispatch of single convolutions, without a device: ops.conv_plan / conv / conv_shuffle2 and ConvOp.fwd / dgrad / fwd_shuffle2
replayed against the table tools/record_conv_plan.py recorded from the dispatch as it was before the plan function existed
(tests/golden/conv_plan.json names the commit)."""
import json

import pytest

from tools import record_conv_plan as R
from trainner_amd import engine, hip, ops

with open(R.GOLDEN) as _f:
    TABLE = json.load(_f)
# The ONE place the replay differs from the record: an up-sampler whose packing has padding rows (20 -> 80: KoutP 96 != 4 * 20) raised
# AssertionError out of ops.conv_shuffle2 wherever the fold was switched on and the arithmetic offered it; it now declines -- False, no library
# entry reached -- as the docstring always promised.  Every other row of that layer, and every row of every other layer, equals the record.
PADDED_SHUFFLE, WAS, NOW = "shuffle_20to80_32", "!AssertionError", "=False"


def test_table_covers_the_whole_cross_product():
    assert [(e, w, tuple(a)) for e, w, a in TABLE["states"]] == R.STATES
    assert len(R.STATES) == len(R.EPIS) * len(R.WINOS) * 8 and len(R.SWITCHES) == 10 and len(R.LAYERS) == 18
    assert set(TABLE["rows"]) == set(R.LAYERS)
    for name in R.LAYERS:
        assert set(TABLE["rows"][name]) == set(R.MMAS)
        for mma in R.MMAS:
            assert set(TABLE["rows"][name][mma]) == {R.switches_id(sw) for sw in R.SWITCHES}
            assert all(len(rows) == len(R.STATES) and all(0 <= i < len(TABLE["outcomes"]) for i in rows) for rows in TABLE["rows"][name][mma].values())


def _plan(c, wino, answers, **kw):
    """ops.conv_plan asked about a recorder case the way ConvOp / ops.conv ask it, with the row's library answers."""
    how, op = c["how"], c["op"]
    said = dict(zip(("splitk", "wino_ok", "stream_ok"), map(bool, answers)), **kw)
    if how == "bare":
        return ops.conv_plan(c["x"], c["wp"], c["y"], c["mode"], c["epi"], wino=wino, **said)
    mode, layer = op.dirs[how == "dgrad"]
    return ops.conv_plan(c["x"], op.packer.get(layer.direct), c["y"], mode, c["epi"], 2 if how == "shuffle" else 0, layer, None if how == "shuffle" else wino, **said)


@pytest.mark.parametrize("mma", list(R.MMAS))
@pytest.mark.parametrize("name", list(R.LAYERS))
def test_dispatch_equals_the_recorded_table(name, mma):
    """Every row: the library entries reached, the descriptor fields of each launch, fwd_shuffle2's answer and the exception type equal the
    record, and conv_plan -- given the row's library answers -- names that form (R.plan_matches: the form-to-entries mapping)."""
    lib = R.FakeLib()
    bad = []
    with R.stand_ins(ops, lib):
        for sw in R.SWITCHES:
            want = TABLE["rows"][name][mma][R.switches_id(sw)]
            R.configure(ops, mma, sw)
            for (epi_name, wino, answers), w in zip(R.STATES, want):
                c = R.case(ops, engine, name, epi_name)
                c["conv"] = ops.conv
                got, w = R.run(lib, c, wino, answers), TABLE["outcomes"][w]
                if name == PADDED_SHUFFLE and w == WAS:
                    w = NOW
                plan = _plan(c, wino, answers)
                ok = R.plan_matches(ops, plan, got)
                if got == "!AssertionError":          # wino=True where the library declines the image: the plan alone says what runs without it
                    ok = ok and wino is True and not answers[1] and _plan(c, wino, answers, wino_ok=True)[0] == "wino"
                why = plan[1]          # the reason words: each only where its cause is present in the row
                ok = ok and why in (None, "switch", "arithmetic", "shape", "epilogue", "declined", "forbidden", "splitk", "forced") \
                    and (why != "switch" or bool(sw)) and (why != "arithmetic" or mma != "bf16x3") and (why != "declined" or 0 in answers) \
                    and (why != "forbidden" or wino is False) and (why != "forced" or wino is True) and (why != "epilogue" or epi_name != "plain" or "reflect" in name)
                if got != w or not ok:
                    bad.append((R.switches_id(sw), epi_name, wino, answers, "recorded " + w, "got " + got, plan))
    assert not bad, "%d rows differ from the table recorded at %s; first: %s" % (len(bad), TABLE["recorded_at_commit"], bad[:3])


def test_padded_shuffle_declines_instead_of_asserting():
    rows = TABLE["rows"][PADDED_SHUFFLE]
    was = [TABLE["outcomes"][i] for mma in R.MMAS for r in rows[mma].values() for i in r]
    assert set(was) == {WAS, NOW} and WAS in [TABLE["outcomes"][i] for i in rows["bf16x3"]["defaults"]]          # (the crash was on the default path)


def test_plan_what_ifs_do_not_touch_the_module(monkeypatch):
    monkeypatch.setattr(ops, "MMA", hip.MMA_BF16X3)
    for k, v in R.DEFAULTS.items():
        monkeypatch.setattr(ops, k, v)
    c = R.case(ops, engine, "3x3_64to64_64", "plain")
    x, y, wp = c["x"], c["y"], c["op"].packer.get(c["op"].i_f)
    assert ops.conv_plan(x, wp, y) == ("wino", None)
    assert ops.conv_plan(x, wp, y, mma=hip.MMA_F32) == ("tile", "arithmetic")
    assert ops.conv_plan(x, wp, y, mma=hip.MMA_BF16) == ("stream", "arithmetic")
    assert ops.conv_plan(x, wp, y, wino_ok=False) == ("stream", "declined")
    assert ops.conv_plan(x, wp, y, wino_ok=False, stream_ok=False) == ("tile", "declined")
    assert ops.conv_plan(x, wp, y, wino=False) == ("stream", "forbidden")
    assert ops.MMA == hip.MMA_BF16X3 and ops.conv_plan(x, wp, y) == ("wino", None)
    monkeypatch.setattr(ops, "WINO", False)          # (read at call time)
    assert ops.conv_plan(x, wp, y) == ("stream", "switch") and ops.conv_plan(x, wp, y, wino=True) == ("wino", "forced")
    monkeypatch.setattr(ops, "X3_D4", False)
    assert ops.conv_plan(x, wp, y) == ("tile", "switch")
    big = R.case(ops, engine, "3x3_512to512_64", "plain")
    bwp = big["op"].packer.get(big["op"].i_f)
    monkeypatch.setattr(ops, "WINO", True)
    assert ops.conv_plan(big["x"], bwp, big["y"]) == ("tile", "splitk") and ops.conv_plan(big["x"], bwp, big["y"], splitk=False) == ("wino", None)
