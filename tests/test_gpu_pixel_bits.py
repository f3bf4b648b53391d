"""The pixel-major matrix-core kernels compute the recorded bits (-m gpu): every output buffer of tnr_upconv3_*, tnr_upconv_i2i_*,
tnr_conv_unshuffle_fwd and tnr_wgrad_unshuffle, and the packed weight images of one x3 and one i2i layer, hashed by
tools/record_pixel_bits.py on its deterministic inputs, against tests/golden/pixel_bits.json, group by group and output by output.

A refactor of these kernels leaves the fixture alone: a differing hash is a changed operation order, to be found by reading and put back.
After a DELIBERATE change of their arithmetic, record again from the new kernels with `python tools/record_pixel_bits.py` on the device
and say so in the change; the fixture then carries that tree's build.source_hash()."""
import json

import pytest

from tools import record_pixel_bits as R

gpu = pytest.mark.gpu
with open(R.GOLDEN) as fh:
    FIXTURE = json.load(fh)


def test_fixture_lists_every_group():
    assert sorted(FIXTURE["bits"]) == sorted(R.group_id(g) for g in R.GROUPS) and len(FIXTURE["source_hash"]) == 16


@gpu
@pytest.mark.parametrize("g", R.GROUPS, ids=R.group_id)
def test_bits(g):
    want, got = FIXTURE["bits"][R.group_id(g)], R.group(g)
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, "%s: other bits than recorded in %s" % (R.group_id(g), differ)
