"""The depth column family keeps its bits (CPU only): every array that the five host harnesses and the five NumPy twins return for the cases
of tests/golden/column_family.npz, recomputed from the stored inputs by tests/golden/make_column_family.py's compute(), has the stored bit
pattern -- compared as bytes, so that NaN and -0 count.  The fixture was written by the commit before the family's shared parts were
merged; together with the GPU tests, which hold the device to the CPU build of the same headers bit for bit, it ties the device's figures
to that commit's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_column_family as MCF      # noqa: E402

FROZEN = MCF.load()


def test_the_fixture_holds_every_case():
    assert sorted(FROZEN) == sorted(c[0] for c in MCF.CASES)
    for name, nx, ny, M, K, weights, twins in MCF.CASES:
        inp, out = FROZEN[name]
        assert [int(v) for v in inp["dims"]] == [nx, ny, M, K, int(twins)] and ("wt" in inp) == weights
        assert any(k.startswith("twin_radial_lateral") for k in out) == twins and any(k.startswith("host_radial_lateral") for k in out)


@pytest.mark.parametrize("case", [c[0] for c in MCF.CASES])
def test_bits(case):
    inp, want = FROZEN[case]
    got = MCF.compute(inp)
    assert sorted(got) == sorted(want), "case %s: the fields differ: %s" % (case, sorted(set(got) ^ set(want)))
    bad = []
    for field in sorted(want):
        g, w = np.ascontiguousarray(got[field]), want[field]
        if g.shape != w.shape or g.dtype != w.dtype:
            bad.append("%s: %s %s, stored %s %s" % (field, g.dtype, g.shape, w.dtype, w.shape))
        elif not np.array_equal(g.reshape(-1).view(np.uint8), np.ascontiguousarray(w).reshape(-1).view(np.uint8)):
            bad.append("%s: %d of %d values differ" % (field, int((g.reshape(-1).view(np.uint8) != w.reshape(-1).view(np.uint8)).reshape(g.size, -1).any(axis=1).sum()), g.size))
    assert not bad, "case %s: %s" % (case, "; ".join(bad))
