"""The bundled node trip's arithmetic helpers (csrc/eikonal_core.h: sqrt_nonneg, min_canon, min3_sel) against the plain forms they replace,
bit for bit, on the device: dsa_selfcheck_trip draws the operands from the ranges the solver produces (csrc/selfcheck.hip says which) and
counts the results that differ.

The helpers leave out what the compiler wraps round the bare instructions for operands the solver never has -- the rescaling of sqrtf for
arguments below 2^-96, the quieting of signalling NaNs in front of a minimum -- so "the same bits" is a statement about operand ranges, and this
is where it is measured.  sqrt_nonneg keeps a guard for the range it does not take: the count of guarded operands must not be zero (the guard is
exercised) and stays below 1 % of the draws.

The deliberate quiet NaN of an outer neighbour that a trip did not fetch (bundle_kernel.hip) never reaches the minima: the second test solves with
and without those NaNs (option bundle_far_all fetches every outer neighbour) and compares whole fields."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_trip_helpers_equal_their_plain_forms():
    from dsurftomo_amd.engine import selfcheck_trip
    nsq, badsq, guarded, nmin, badmin = selfcheck_trip(20261017, 20)
    print("sqrt_nonneg: %d operands, %d differ from sqrtf, %d left to sqrtf by the guard; minima: %d, %d differ" % (nsq, badsq, guarded, nmin, badmin))
    assert nsq >= 20_000_000 and nmin >= 20_000_000
    assert badsq == 0 and badmin == 0
    assert 0 < guarded < nsq // 100


def test_unfetched_outer_values_do_not_reach_the_minima(engine):
    e = engine
    e.set_option("exact_ties", 0)
    e.set_option("field_pool", -1)
    e.set_option("bundle", 16)
    nx, nsrc, nper, nrec = 19, 4, 16, 3
    pv = np.stack([synth.medium(nx, "checker4", 0) * (1.0 + 0.015 * p) for p in range(nper)])
    u = synth.units(nx, nsrc, nper, nrec, seed=synth.SEED + 5)
    n = nsrc * nper
    e.set_maps(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, pv)
    out = {}
    for far_all in (1, 0):
        e.set_option("bundle_far_all", far_all)
        t = e.traveltimes(**u)
        assert e.stats()["bundled_units"] == n
        out[far_all] = (t, np.stack([e.field(k) for k in range(n)]))
    assert np.isfinite(out[0][1]).all()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0]))
    assert np.array_equal(bits(out[0][1]), bits(out[1][1]))
