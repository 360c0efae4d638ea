"""The units of tests/golden/solve_units.json are what tests/test_gpu_solve_shapes.py takes them for: units without exact ties, whose fixed
point is the oracle's Fast Marching field in every bit under every schedule.  No GPU involved: the property (solve_units.tie_free) is
derived again for every listed unit from the oracle and the CPU emulation of the device schedule, so that a change to the oracle or to the
core headers cannot silently turn a listed unit into a tie case.

Media dropped: `wild` on the 257^2 grid -- none of its 64 candidates holds the property there (fewer than four: dropped); the other
fifteen (grid, medium) pairs yield 6 to 56 (the list's "candidates_that_hold_of_64").
"""
import json

import pytest

import solve_units as SU


@pytest.fixture(scope="module")
def H():
    return SU.hostcheck()


def test_the_list_covers_every_grid():
    units = SU.load()
    assert set(units) == set(SU.GRIDS)
    for name, rows in units.items():
        assert 8 <= len(rows) <= 12, name
        assert len({k for k, _, _ in rows}) >= 2, name
        assert all(k in SU.MEDIA for k, _, _ in rows)
        cand = SU.candidates(name)
        assert all((fx, fz) in cand for _, fx, fz in rows), "a listed source is not among the grid's candidates"
        g = SU.grid_of(name)
        # sources within three cells of an edge are among them
        assert any(min(fx * (g.nnx - 1), (1 - fx) * (g.nnx - 1), fz * (g.nnz - 1), (1 - fz) * (g.nnz - 1)) < 3.0 for _, fx, fz in rows), name
    with open(SU.LIST) as f:
        held = json.load(f)["candidates_that_hold_of_%d" % SU.NCAND]
    assert all(held["%s/%s" % (name, k)] >= 4 for name, rows in units.items() for k, _, _ in rows)


@pytest.mark.parametrize("name", list(SU.GRIDS))
def test_listed_units_are_tie_free(H, name):
    cases = {}
    for kind, fx, fz in SU.load()[name]:
        if kind not in cases:
            cases[kind] = SU.Case(name, kind)
        good, why = SU.tie_free(H, cases[kind], fx, fz)
        assert good, (name, kind, fx, fz, why)


def test_the_property_rejects_a_unit_with_ties(H):
    """a source on a node of the +-13 % checkerboard (the named tie case of tests/test_gpu_parity.py) does not pass"""
    import _libs as L
    import synth
    case = SU.Case("257", "smooth")
    case.kind, case.pv = "checker4", synth.medium(35, "checker4")
    case.veln = L.o_gridder(case.g, case.pv)
    good, why = SU.tie_free(H, case, 5.0 / 256, 7.0 / 256)
    assert not good and why
