"""The bundled node trip (csrc/bundle_kernel.hip, pass B) against the unit-by-unit solve, bit for bit, with bundles of 16 forced: whole fields and
receiver times at the smallest grids that bundle (nx = 17 and 19: 113^2 and 129^2 nodes at dicing 8) and at 257^2 --

  * 8 sources x 16 periods on the smooth medium;
  * the same on the checkerboard (synth's "checker": +-8 %, 16-vertex squares, the velocity rising from period to period), where exact ties,
    slow-queue members and census candidates occur;
  * one source on a node line and one in a corner cell;
  * a ragged bundle: a source with data at 5 of the 16 periods.

The trip's member body is written for instruction count (eikonal_core.h: sqrt_nonneg, min3_sel, the sign tests' OR, the change hash); every member
evaluation must still be the unit-by-unit solve's operations on the same operands.

The reference has to be a function of its inputs for "bit for bit" to mean anything: an exact tie has two states ("Ties"), and on a medium
that ties densely the unit-by-unit solve does not repeat ITSELF.  A first version of this file took 4-vertex squares of +-13 % scaled by 1.5 % per
period: at 257^2 two unit-by-unit runs of the same call differed at 17 field nodes, and bundles differed from either at 1611 - 1628 of 8.45 M nodes
(max 5.2e-6 s, no receiver time; the parent commit's library: 1618 - 1621).  On the project's checkerboard every run repeats, ties included.

In exact_ties = 1 the census of the converged field decides which units the literal march solves again.  Its candidates come from the round loop
(the trip lists a member whose value equals a near neighbour's); the sweep of the whole converged field (option tie_list = 0: no list at all, the
census the kernel falls back to when the list overflows) does not depend on that marking, so it is the record the listed census must reproduce:
flags, largest influences, counts and sums of every unit, and the set of marched units.  Both are bundled runs, which repeat on every medium
here, so this comparison also takes the densely tied small-square medium (the project's checkerboard has one or two squares at these sizes)."""
import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu
NPER, NREC = 16, 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def maps(nx, kind):
    if kind == "smooth":
        return np.stack([synth.medium(nx, "smooth", p) for p in range(NPER)])
    if kind == "checker4s":      # 4-vertex squares of +-13 %, scaled from period to period: ties everywhere (the census' subject; see the module docstring)
        return np.stack([synth.medium(nx, "checker4", 0) * (1.0 + 0.015 * p) for p in range(NPER)])
    return np.stack([synth.medium(nx, "checker", p) for p in range(NPER)])


def place(nx, fx, fz):
    """a position given in nodes of the propagation grid -> (colatitude, longitude) fp32 radians"""
    gox, goz, dnx, dnz = synth.grid_origin(nx)
    return np.float32(gox + np.float32(fx) * dnx), np.float32(goz + np.float32(fz) * dnz)


def units_of(nx, case):
    """8 sources x 16 periods in the reference's order; `edge`: source 0 on a node line, source 1 in the corner cell; `ragged`: source 2 has data
    at its first 5 periods only"""
    nsrc = 8
    u = synth.units(nx, nsrc, NPER, NREC, seed=synth.SEED + 17)
    if case == "edge":
        N = synth.nprop(nx)
        sx, sz = u["scx"][:nsrc].copy(), u["scz"][:nsrc].copy()
        sx[0], sz[0] = place(nx, float(N // 3), N / 2.0 + 0.37)
        sx[1], sz[1] = place(nx, 0.4, 0.6)
        idx = (np.arange(nsrc)[:, None] + 1 + np.arange(NREC)[None, :]) % nsrc
        u = dict(u, scx=np.tile(sx, NPER), scz=np.tile(sz, NPER), rcx=np.tile(sx[idx].reshape(-1), NPER), rcz=np.tile(sz[idx].reshape(-1), NPER))
    if case == "ragged":
        k = np.arange(nsrc * NPER)
        keep = ~((k % nsrc == 2) & (k // nsrc >= 5))
        rkeep = np.repeat(keep, NREC)
        u = dict(map_index=u["map_index"][keep], scx=u["scx"][keep], scz=u["scz"][keep], nrec=u["nrec"][keep], rcx=u["rcx"][rkeep], rcz=u["rcz"][rkeep])
    return u


@pytest.mark.parametrize("nx", [17, 19, 35])
@pytest.mark.parametrize("kind,case", [("smooth", "full"), ("checker", "full"), ("checker", "edge"), ("smooth", "edge"), ("checker", "ragged")])
def test_bundles_of_16_equal_unit_by_unit(engine, nx, kind, case):
    e = engine
    e.set_option("exact_ties", 0)             # the fixed point is the subject: no unit is handed to the march behind it
    e.set_option("field_pool", -1)            # a field per unit
    u = units_of(nx, case)
    n = u["map_index"].size
    e.set_maps(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, maps(nx, kind))
    e.set_option("bundle", 0)
    ref_t = e.traveltimes(**u)
    assert e.stats()["bundles"] == 0
    ref_f = np.stack([e.field(k) for k in range(n)])
    assert np.isfinite(ref_f).all()
    again = e.traveltimes(**u)                  # (the reference repeats: see the module docstring)
    assert np.array_equal(bits(again), bits(ref_t)) and np.array_equal(bits(np.stack([e.field(k) for k in range(n)])), bits(ref_f))
    e.set_option("bundle", 16)
    t = e.traveltimes(**u)
    st = e.stats()
    assert st["bundle_size"] == 16 and st["bundles"] > 0 and st["bundled_units"] == n, st
    f = np.stack([e.field(k) for k in range(n)])
    nbad_t, nbad_f = int((bits(t) != bits(ref_t)).sum()), int((bits(f) != bits(ref_f)).sum())
    print(f"N={e.nnx} {kind} {case}: {nbad_t} of {t.size} times, {nbad_f} of {f.size} field nodes differ from unit by unit")
    assert nbad_t == 0 and nbad_f == 0


@pytest.mark.parametrize("nx", [19, 35])
@pytest.mark.parametrize("kind", ["smooth", "checker", "checker4s"])
def test_listed_census_equals_the_sweep(engine, nx, kind):
    e = engine
    u = units_of(nx, "full")
    n = u["map_index"].size
    e.set_maps(nx, nx, synth.GOXD, synth.GOZD, synth.DVD, synth.DVD, maps(nx, kind))
    e.set_option("bundle", 16)
    out = {}
    for tl in (0, 1):
        e.set_option("tie_list", tl)
        t = e.traveltimes(**u)
        st = e.stats()
        assert st["bundled_units"] == n, st
        fl, infl = e.unit_ties()
        cnt, sm, fr = e.unit_tie_sums()
        out[tl] = (t, fl.copy(), infl.copy(), cnt.copy(), sm.copy(), fr.copy(), int(st["tie_units"]), int(st["exact_units"]))
    a, b = out[0], out[1]
    print(f"N={e.nnx} {kind}: sweep flags {a[6]} units, marches {a[7]}; list flags {b[6]}, marches {b[7]}; ties counted {int(a[3].sum())} / {int(b[3].sum())}")
    assert np.array_equal(a[1], b[1]), np.nonzero(a[1] != b[1])[0][:8]          # (bit 0: met a tie, bit 1: solved by the literal march)
    assert np.array_equal(bits(a[2]), bits(b[2]))
    assert np.array_equal(a[3], b[3]) and np.array_equal(bits(a[4]), bits(b[4])) and np.array_equal(a[5], b[5])
    assert a[6] == b[6] and a[7] == b[7]
    assert np.array_equal(bits(a[0]), bits(b[0]))
    if kind == "checker4s":
        assert int(a[3].sum()) > 0          # (the medium does tie: the comparison is not one of empty records)
