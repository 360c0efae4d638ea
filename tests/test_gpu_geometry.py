"""The device on the geometries of tests/geometry_cases.py, where swapping nnx / nnz or dnx / dnz, a wrong risti_table length, a wrong
sin_rx or a wrong branch of sinf_libm shows: rectangles both ways, unequal spacings, latitudes 65 and 80 N and 50 S, negative longitudes,
the equator, dicing 3.  The oracle these tests compare with is pinned to the reference on the same inputs, bit for bit, by
tests/test_oracle_vs_ref.py::test_fields_rays_geometry.

  * grid: dimensions and the diced velocity grid (bit-identical to dso_gridder);
  * literal march (exact_ties = 2): coarse field, refined snapshot on the alive set, status classes, receiver times -- the oracle's, bit
    for bit; on the homogeneous media every front is full of ties, so this is the tie-order test on a rectangle; once more on `tall` with
    a small tree in LDS and its global part in blocks, and once times-only through the pooled tiles;
  * default mode (exact_ties = 1) on four maps per case: every field within 1e-4 s (BASELINE north_star), marched units bit-identical;
    under exact_ties = 0 the automatic mode's and forced bundles' receiver times against unit-by-unit ones.  (The scaled homogeneous
    maps of `tall` showed a status tie at the hand-off that the census let pass in a homogeneous box, 1.9e-4 s: fixed in
    stage_kernels.hip k_handoff_probe, pinned on the square by tests/test_gpu_exact.py);
  * rays (exact_ties = 2, so the fields are the oracle's own): every ray's points against dso_rpaths_path, the Frechet rows against
    dso_rpaths -> dso_assemble_row, bit for bit;
  * azimuthal rows: the per-ray sums of cos 2psi / sin 2psi against the path-point model of tests/test_hostcheck_azimuthal.py.

Every test takes the session's engine with the product's defaults (conftest.py) and sets each option it depends on; what it sets outside
conftest's list (ray_path_cap, keep_fields) it puts back.  The oracle's solves are computed once per case and shared.
"""
import numpy as np
import pytest

import _libs as L
import geometry_cases as G
import parity_log
import test_gpu_rows as R
import test_hostcheck_azimuthal as T

pytestmark = pytest.mark.gpu
TOL = 1e-4
NMAPS = 4                   # maps per case in the default-mode test: a bundle is four units of one source on different maps
TIE = 2e-5                  # the census's tie_threshold (csrc/engine.h kDefaultTieThreshold): what two states of an exact tie may differ by
PATH_CAP = 8192


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    """one (geometry, medium): the oracle's grid, maps, diced velocities and solves -- computed when first asked for, then kept"""

    def __init__(self, name, kind):
        self.name, self.kind = name, kind
        self.geo = G.geometry(name)
        nx, ny = self.geo[:2]
        self.g = g = L.grid(*self.geo)
        assert (g.nnx, g.nnz) == G.nodes(name)
        pv0 = G.medium(nx, ny, kind)
        self.pv = np.stack([pv0 * (1.0 + 0.02 * p) for p in range(NMAPS)])          # map 0 is the pinned medium itself
        self._veln, self._sol = {}, {}
        src, rec = G.plan(name)
        self.sx, self.sz = G.radians(g.gox, g.goz, g.dnx, g.dnz, src)
        self.rx, self.rz = G.radians(g.gox, g.goz, g.dnx, g.dnz, rec)

    def veln(self, p=0):
        if p not in self._veln:
            self._veln[p] = L.o_gridder(self.g, self.pv[p])
        return self._veln[p]

    def sol(self, s, p=0):
        if (s, p) not in self._sol:
            self._sol[s, p] = L.o_solve(self.g, self.pv[p], self.veln(p), self.sx[s], self.sz[s])
        return self._sol[s, p]

    def time(self, s, i, p=0):
        return L.o_srtimes(self.g, self.veln(p), self.sol(s, p)["T"], self.sx[s], self.sz[s], self.rx[s, i], self.rz[s, i])

    def units(self, nrec, nmaps=1):
        """the plan: period slot outer, source inner; the first nrec receivers of every source"""
        return dict(map_index=np.repeat(np.arange(nmaps, dtype=np.int32), G.NSRC), scx=np.tile(self.sx, nmaps), scz=np.tile(self.sz, nmaps),
                    nrec=np.full(G.NSRC * nmaps, nrec, np.int32), rcx=np.tile(self.rx[:, :nrec].reshape(-1), nmaps),
                    rcz=np.tile(self.rz[:, :nrec].reshape(-1), nmaps))

    def set_maps(self, e, nmaps=1):
        nx, ny, goxd, gozd, dvxd, dvzd, gd = self.geo
        e.set_maps(nx, ny, goxd, gozd, dvxd, dvzd, self.pv[:nmaps], dicing=gd)
        assert (e.nnx, e.nnz) == (self.g.nnx, self.g.nnz)


_cases = {}


def case(name, kind):
    if (name, kind) not in _cases:
        _cases[name, kind] = Case(name, kind)
    return _cases[name, kind]


def assert_march(e, c, t, nrec, what):
    """fields, refined snapshots, status classes and receiver times of the six units of map 0 against the oracle, bit for bit"""
    alive_n = 0
    for s in range(G.NSRC):
        o = c.sol(s)
        assert (bits(e.field(s)) != bits(o["T"])).sum() == 0, (what, s, "coarse field")
        Tr, Sr = e.refined(s)
        cls_o = np.sign(o["Sr"]).clip(-1, 1)
        assert Sr.shape == cls_o.shape and (cls_o != Sr).sum() == 0, (what, s, "status classes")
        alive = cls_o == 0
        alive_n += int(alive.sum())
        assert (bits(Tr[alive]) != bits(o["Tr"][alive])).sum() == 0, (what, s, "refined snapshot")
        for i in range(nrec):
            assert np.float32(t[nrec * s + i]).view(np.uint32) == np.float32(c.time(s, i)).view(np.uint32), (what, s, i)
    return alive_n


# ---- grid ------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", G.PAIRS)
def test_grid_and_diced_velocity(engine, name, kind):
    c = case(name, kind)
    c.set_maps(engine, NMAPS)
    for p in range(NMAPS):
        v = engine.velocity(p)
        assert v.shape == (c.g.nnx, c.g.nnz) and (bits(v) != bits(c.veln(p))).sum() == 0, (name, kind, p)
    parity_log.add("geometry %s %s: %d x %d nodes, %d diced velocity grids bit-identical to the oracle's" % (name, kind, c.g.nnx, c.g.nnz, NMAPS))


# ---- the literal march -----------------------------------------------------------------------------------------------------------------------

MARCH = [(n, k, 2048) for n, k in G.PAIRS] + [("tall", "smooth", -63), ("tall", "homog", -63)]


@pytest.mark.parametrize("name,kind,lds", MARCH)
def test_literal_march_is_the_oracle_bit_for_bit(engine, name, kind, lds):
    """lds as in test_gpu_exact.py: the tree slots kept in LDS; negative: that many, with the tree's global part in blocks of three levels"""
    e, c = engine, case(name, kind)
    e.set_option("exact_ties", 2)
    e.set_option("exact_heap_blocked", 2 if lds < 0 else 0)
    e.set_option("exact_lds_slots", abs(lds))
    e.set_option("exact_tiles", 0)
    e.set_option("field_pool", 0)
    c.set_maps(e)
    t = e.traveltimes(**c.units(2))
    st = e.stats()
    assert st["exact_units"] == G.NSRC
    alive = assert_march(e, c, t, 2, (name, kind, lds))
    parity_log.add("geometry %s %s, literal march (tree slots in LDS %d%s): %d sources, %d field nodes, %d alive refined nodes, %d receiver times "
                   "bit-identical to the oracle (%d accepts)" % (name, kind, abs(lds), ", global part blocked" if lds < 0 else "", G.NSRC,
                                                              G.NSRC * c.g.nnx * c.g.nnz, alive, 2 * G.NSRC, int(st["exact_pops"])))


def test_march_in_pooled_tiles_on_a_rectangle(engine):
    """`tall` (121 x 257 nodes: 16 x 33 tiles), both media, times only: the march on pooled 8 x 8-node tiles gives the receiver times of
    the march on whole fields, and those are the oracle's"""
    from dsurftomo_amd.engine import EngineError
    e = engine
    cs = [case("tall", "smooth"), case("tall", "homog")]
    nx, ny, goxd, gozd, dvxd, dvzd, gd = cs[0].geo
    pv = np.stack([c.pv[0] for c in cs])
    u = cs[0].units(G.NREC, 2)
    e.set_option("exact_ties", 2)
    e.set_option("exact_heap_blocked", 1)
    e.set_option("exact_lds_slots", 0)
    e.set_option("exact_tile_cap", 0)
    e.set_option("field_pool", 4)               # fewer compact slots than units: a times-only call
    e.set_maps(nx, ny, goxd, gozd, dvxd, dvzd, pv, dicing=gd)
    e.set_option("exact_tiles", 0)
    t_full = e.traveltimes(**u)
    st_full = e.stats()
    e.set_option("exact_tiles", 1)
    t_tiles = e.traveltimes(**u)
    st = e.stats()
    with pytest.raises(EngineError):
        e.field(0)
    assert st_full["exact_tiles"] == 0 and st["exact_tiles"] > 0 and st["exact_units"] == 2 * G.NSRC
    assert st["exact_pops"] == st_full["exact_pops"]
    want = np.array([c.time(s, i) for c in cs for s in range(G.NSRC) for i in range(G.NREC)], np.float32)
    nbad = int((bits(t_tiles) != bits(t_full)).sum())
    nbad_o = int((bits(t_full) != bits(want)).sum())
    parity_log.add("geometry tall, march in pooled tiles: %d units, %d tiles per unit of the grid's %d: %d of %d receiver times differ from the march on "
                   "whole fields, %d from the oracle" % (2 * G.NSRC, int(st["exact_tiles"]), ((e.nnx + 7) // 8) * ((e.nnz + 7) // 8), nbad, t_full.size, nbad_o))
    assert np.isfinite(t_full).all() and nbad == 0 and nbad_o == 0


# ---- the default mode ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", G.PAIRS)
def test_default_mode_and_bundles(engine, name, kind):
    """six sources on four maps (the pinned medium and three scaled copies), four receivers each.  exact_ties = 1: every field within
    1e-4 s of the oracle's, the units the census hands to the march bit-identical.  exact_ties = 0: the receiver times of the automatic
    mode (bundle = 1) equal those unit by unit (bundle = 0), bit for bit.  The automatic mode leaves launches this small unit by unit
    (bundle_plan.h: choose_bundle_size), so the bundle kernel itself is run with bundle = 4, six bundles of four: its times are the
    unit-by-unit ones bit for bit on the smooth media, whose fixed point is unique; on the rough and homogeneous media an exact tie has
    two self-consistent states (tests/test_gpu_bundles.py), which differ by less than the census's threshold"""
    e, c = engine, case(name, kind)
    n = G.NSRC * NMAPS
    u = c.units(G.NREC, NMAPS)
    e.set_option("field_pool", -1)              # a field per unit: bundles leave their members' fields behind
    e.set_option("exact_ties", 1)
    e.set_option("bundle", 1)
    c.set_maps(e, NMAPS)
    t1 = e.traveltimes(**u)
    marched = (e.unit_ties()[0] & 2) != 0
    worst = worst_t = 0.0
    for k in range(n):
        s, p = k % G.NSRC, k // G.NSRC
        o = c.sol(s, p)
        T = e.field(k)
        d = float(np.abs(T - o["T"]).max())
        worst = max(worst, d)
        assert d <= TOL, (name, kind, k, d)
        if marched[k]:
            assert (bits(T) != bits(o["T"])).sum() == 0, (name, kind, k, "marched unit")
        for i in range(G.NREC):
            dt = abs(float(t1[G.NREC * k + i]) - float(c.time(s, i, p)))
            worst_t = max(worst_t, dt)
            assert dt <= TOL, (name, kind, k, i, dt)
            if marched[k]:
                assert np.float32(t1[G.NREC * k + i]).view(np.uint32) == np.float32(c.time(s, i, p)).view(np.uint32), (name, kind, k, i)
    e.set_option("exact_ties", 0)
    out, stb = {}, None
    for b in (0, 1, 4):
        e.set_option("bundle", b)
        out[b] = e.traveltimes(**u)
        if b == 4:
            stb = e.stats()
    e.set_option("bundle", 1)
    assert stb["bundle_size"] == 4 and stb["bundles"] == G.NSRC and stb["bundled_units"] == n, stb
    nbad1 = int((bits(out[1]) != bits(out[0])).sum())
    nbad4 = int((bits(out[4]) != bits(out[0])).sum())
    d4 = float(np.abs(out[4] - out[0]).max())
    parity_log.add("geometry %s %s, default mode: %d units, worst field |dT| %.3g s, worst receiver |dt| %.3g s, %d units marched (bit-identical); "
                   "exact_ties = 0: of %d receiver times %d differ between bundle = 1 and unit by unit, %d between %d bundles of 4 and unit by unit (max %.3g s)" %
                   (name, kind, n, worst, worst_t, int(marched.sum()), out[0].size, nbad1, nbad4, int(stb["bundles"]), d4))
    assert np.isfinite(out[0]).all() and nbad1 == 0
    assert d4 <= TIE and (nbad4 == 0 or kind != "smooth")


# ---- rays and rows ---------------------------------------------------------------------------------------------------------------------------

RAYS = [(n, k) for n, k in G.PAIRS if n in ("north80", "north65", "south50", "equator", "unequal", "tall")]


def sine_branch(name):
    """n of sinf_libm's reduction (ray_core.h) over the grid's colatitudes: 0 below pi/4, else the nearest multiple of pi/2"""
    return sorted({0 if x < np.pi / 4 else int(np.rint(x * 2 / np.pi)) for x in G.colatitudes(name)})


def test_the_cases_reach_every_branch_of_the_sine():
    """north80 (and north65) lie wholly in the branch without a reduction, south50 wholly in n = 2, every other case in n = 1"""
    assert sine_branch("north80") == [0] and sine_branch("north65") == [0] and sine_branch("south50") == [2]
    assert all(sine_branch(n) == [1] for n in G.CASES if n not in ("north80", "north65", "south50"))
    lo, hi = G.colatitudes("equator")
    assert lo < np.pi / 2 < hi and G.geometry("equator")[3] == 0.0 and G.geometry("north80")[3] < 0 and G.geometry("south50")[3] < 0


@pytest.mark.parametrize("name,kind", RAYS)
def test_ray_paths_and_rows_against_the_oracle(engine, name, kind):
    e, c = engine, case(name, kind)
    g = c.g
    nx, ny = c.geo[:2]
    u = c.units(G.NREC)
    dm = R.depth_model(nx, ny)
    if name == "north80":
        assert sine_branch(name) == [0]
    if name == "south50":
        assert sine_branch(name) == [2]
    e.set_option("exact_ties", 2)
    e.set_option("exact_heap_blocked", 0)
    e.set_option("exact_lds_slots", 2048)
    e.set_option("field_pool", 0)
    e.set_option("ray_lanes", 0)
    e.set_option("ray_path_cap", PATH_CAP)
    try:
        c.set_maps(e)
        r = R.solve_rows(e, u, dm)
        paths = e.ray_paths(PATH_CAP)
        t, st = r[0], r[4]
        assert st["exact_units"] == G.NSRC and st["rays"] == G.NSRC * G.NREC
        assert_march(e, c, t, G.NREC, (name, kind, "rays"))                      # the fields are the oracle's own
    finally:
        e.set_option("ray_path_cap", 0)
        e.keep_fields(False)
    assert [d for d, _ in paths] == list(range(1, G.NSRC * G.NREC + 1))
    npts = 0
    for s in range(G.NSRC):
        for i in range(G.NREC):
            want = L.o_ray_path(g, c.sol(s), c.veln(), c.sx[s], c.sz[s], c.rx[s, i], c.rz[s, i], cap=PATH_CAP)
            got = paths[G.NREC * s + i][1]
            assert got.shape == want.shape and (bits(got) == bits(want)).all(), (name, kind, s, i, got.shape, want.shape)
            npts += len(got)
    sols = [(c.veln(), c.sol(s)["T"], c.sol(s)["Tr"], c.sol(s)["Sr"]) for s in range(G.NSRC)]
    o = R.oracle_rows(g, u, dm, lambda k: sols[k])
    R.assert_against(r, o, "geometry %s %s" % (name, kind))
    assert o["rw"].size > 0 and o["steps"].sum() > 10 * o["steps"].size
    parity_log.add("geometry %s %s, rays: %d rays, %d path points, %d steps (%d clamped), %d row entries bit-identical to the oracle end to end" %
                   (name, kind, o["steps"].size, npts, int(o["steps"].sum()), int((o["rbint"] == 1).sum()), o["rw"].size))


# ---- azimuthal rows --------------------------------------------------------------------------------------------------------------------------

def azimuthal_plan(c):
    """test_hostcheck_azimuthal.py's rays on a rectangle: three sources, eight receivers each, all at least three node cells inside the
    grid and at least a quarter of the shorter side from the source"""
    import synth
    g = c.g
    NX, NZ = g.nnx, g.nnz
    r = synth.LCG(23 + NX + NZ)
    src, rec = [(0.43 * NX + 0.3, 0.61 * NZ + 0.6), (4.4, NZ / 2 + 0.2), (NX - 5.5, NZ - 6.3)], []
    for fx, fz in src:
        k = 0
        while k < 8:
            v = r.uniform(2)
            px, pz = 3.3 + v[0] * (NX - 7.6), 3.3 + v[1] * (NZ - 7.6)
            if np.hypot(px - fx, pz - fz) < 0.25 * min(NX, NZ):
                continue
            rec.append((px, pz))
            k += 1
    sx, sz = G.radians(g.gox, g.goz, g.dnx, g.dnz, np.array(src))
    rx, rz = G.radians(g.gox, g.goz, g.dnx, g.dnz, np.array(rec))
    return dict(map_index=np.zeros(3, np.int32), scx=sx, scz=sz, nrec=np.full(3, 8, np.int32), rcx=rx, rcz=rz)


@pytest.mark.parametrize("name,kind", [("south50", "rough"), ("south50", "homog"), ("unequal", "smooth")])
def test_azimuthal_sums_against_the_path_point_model(engine, name, kind):
    """dsa_solve_rows_azimuthal on marched fields: the isotropic block is the oracle's rows, the steps are the oracle's, and every ray's
    mean cos 2psi / sin 2psi lies within test_hostcheck_azimuthal.DELTA of the model built from the oracle's path points alone (south = dx R,
    east = dz R sin x: a swapped spacing, a wrong sine or a wrong sign is an error of order 1).  DELTA was derived for steps of 1.1e-5 to
    1.7e-5 rad at coordinates below 2 rad; here the steps are no shorter and the coordinates below 4 rad (one binade: twice the ulp, under
    steps four times as long on south50), so the same bound holds"""
    e, c = engine, case(name, kind)
    g = c.g
    nx, ny = c.geo[:2]
    u = azimuthal_plan(c)
    dm = R.depth_model(nx, ny)
    e.set_option("exact_ties", 2)
    e.set_option("exact_heap_blocked", 0)
    e.set_option("exact_lds_slots", 2048)
    e.set_option("field_pool", 0)
    e.set_option("ray_lanes", 0)
    e.set_azimuthal_slots(None)
    try:
        c.set_maps(e)
        e.keep_fields(False)
        e.set_depth_kernels(*dm)
        e.plan(u["map_index"], u["scx"], u["scz"], u["nrec"], u["rcx"], u["rcz"])
        t, rw, iw, col = e.solve_rows_azimuthal(3 * R.capacity(u))
        datum, steps, sums = e.ray_azimuths()
    finally:
        e.keep_fields(False)
    assert (datum == np.arange(1, 25)).all()
    maxvp = (nx - 2) * (ny - 2) * (dm[0].shape[0] - 1)
    sols = [L.o_solve(g, c.pv[0], c.veln(), u["scx"][s], u["scz"][s]) for s in range(3)]
    o = R.oracle_rows(g, u, dm, lambda k: (c.veln(), sols[k]["T"], sols[k]["Tr"], sols[k]["Sr"]))
    iso = col <= maxvp
    R.assert_rows(dict(rw=rw[iso], iw=iw[iso], col=col[iso]), o, "geometry %s %s, isotropic block" % (name, kind))
    assert (~iso).sum() > 0 and (steps == o["steps"]).all() and (o["rbint"] & 1 == 0).all() and steps.min() > 20
    worst = 0.0
    for s in range(3):
        for i in range(8):
            q = 8 * s + i
            pts, rb, ns, _ = T.oracle_path_radians(g, sols[s], c.veln(), u["scx"][s], u["scz"][s], u["rcx"][q], u["rcz"][q])
            assert ns == steps[q] and len(pts) == ns + 2
            c2, s2 = T.model_2psi(g, pts, ns)
            worst = max(worst, abs(float(sums[q, 0]) / ns - c2.mean()), abs(float(sums[q, 1]) / ns - s2.mean()))
    parity_log.add("geometry %s %s, azimuthal rows: 24 rays, %d isotropic entries bit-identical to the oracle's rows, %d gc / gs entries; worst deviation of a "
                   "ray's mean cos 2psi / sin 2psi from the path-point model %.3g (bound %.3g)" % (name, kind, int(iso.sum()), int((~iso).sum()), worst, T.DELTA))
    assert worst <= T.DELTA
