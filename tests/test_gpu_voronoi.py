"""dsa_lsmr_voronoi (csrc/lsmr_batch.hip): K LSMR solves on random Voronoi projections of the resident system's data rows.  Member k
must equal, in every output bit (z, itn, istop, normA, condA, normr, normAr, normx), dsa_lsmr -- and the oracle's restatement of the
reference's LSMR -- on M_k: the data rows listed row by row with every column j relabelled cell_k(j), built here in numpy.  The cells
must equal invert.voronoi_cells exactly and the ensemble statistics invert.voronoi_stats bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import _libs as L
import inversion as inv
import synth
import synth_matrix as SM
from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei
from dsurftomo_amd.engine import Engine, EngineError, load_library
from test_gpu_lsmr import system
from test_gpu_lsmr_batch import EST, assert_all_equal, load, realisation
from test_gpu_tradeoff import same_bits

pytestmark = pytest.mark.gpu


def projected(S, nd, cell_k, ncells):
    """M_k as the contract states it: the entries of the rows below nd, rows ascending, each row's entries in storage order (a stable
    sort of the COO by row), column j -> cell_k[j]; right-hand side b[:nd]"""
    nar = S["nar"]
    rows, cols = S["iw"][1:nar + 1], S["iw"][nar + 1:]
    keep = np.flatnonzero(rows <= nd)
    keep = keep[np.argsort(rows[keep], kind="stable")]
    r, cc = rows[keep], (cell_k[cols[keep] - 1] + 1).astype(np.int32)
    k = keep.size
    return dict(m=nd, n=ncells, nar=k, iw=np.concatenate([[k], r, cc]).astype(np.int32), rw=np.ascontiguousarray(S["rw"][keep], np.float32),
                b=np.ascontiguousarray(S["b"][:nd], np.float32))


def member(V, k):
    return dict(x=V["z"][k], istop=int(V["istop"][k]), itn=int(V["itn"][k]), **{q: V[q][k] for q in EST})


def empty_cells(Mk):
    return np.bincount(Mk["iw"][Mk["nar"] + 1:] - 1, minlength=Mk["n"]) == 0


def assert_members(V, S, nd, ncells, damp, some, engine=None, oracle=True, **kw):
    """members `some` of V against the oracle's LSMR on M_k and (engine: a second engine) dsa_lsmr after spmv_load(M_k); returns how many
    cells without data were met"""
    nempty = 0
    for k in some:
        Mk = projected(S, nd, V["cell"][k], ncells)
        if oracle:
            want = inv.call_lsmr(L.oracle().dso_lsmr, Mk, damp, **kw)
            assert inv.same(member(V, k), want) == [], ("oracle", k)
        if engine is not None:
            load(engine, Mk)
            own = engine.lsmr(Mk["b"], damp, **kw)
            assert inv.same(member(V, k), own) == [], ("dsa_lsmr", k)
        none = empty_cells(Mk)
        assert not V["z"][k][none].any(), k                            # a cell no data entry touches gets z = 0
        nempty += int(none.sum())
    return nempty


def assert_stats(V):
    x = np.take_along_axis(V["z"], V["cell"], axis=1)
    want = invert.voronoi_stats(x)
    assert same_bits(V["stats"], want), "stats differ from the fp64 loop: max |d mean| %g, max |d std| %g" % (
        np.abs(V["stats"][0] - want[0]).max(), np.abs(V["stats"][1] - want[1]).max())


def lattice_xyz(c):
    """integer lattice points of the unknowns (i fastest, then j, then k; depth step 1.5): exact ties abound"""
    ni, nj, nk = c["nx"] - 2, c["ny"] - 2, c["nz"] - 1
    k, j, i = np.meshgrid(np.arange(nk), np.arange(nj), np.arange(ni), indexing="ij")
    return np.stack([i.ravel() * 1.0, j.ravel() * 1.0, k.ravel() * 1.5], axis=1)


@pytest.fixture(scope="module")
def boundary():
    c = synth.boundary_case()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


@pytest.mark.parametrize("local_size,itnlim", [(10, 400), (0, 100), (3, 7)])
def test_voronoi_boundary_case_against_the_oracle(boundary, local_size, itnlim):
    """five members, 6 and 40 cells, lattice points (ties): the cells == voronoi_cells, every member == the oracle's LSMR and dsa_lsmr
    on M_k, the statistics == the fp64 loop; the same bits without z and cell, and on a second call"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, n = c["ndata"], S["n"]
    assert nd == S["m"] - n
    xyz = lattice_xyz(c)
    assert xyz.shape == (n, 3)
    e, e2 = Engine(0), Engine(0)
    kw = dict(itnlim=itnlim, local_size=local_size)
    try:
        load(e, S)
        for ncells in (6, 40):
            seeds = invert.voronoi_seeds(n, ncells, 5, seed=3 + ncells)
            V = e.lsmr_voronoi(S["b"], nd, ncells, xyz, seeds, 0.5, **kw)
            assert V["z"].shape == (5, ncells) and V["cell"].shape == (5, n) and V["stats"].shape == (2, n)
            assert np.array_equal(V["cell"], invert.voronoi_cells(xyz, seeds))
            assert_members(V, S, nd, ncells, 0.5, range(5), engine=e2, **kw)
            assert_stats(V)
            assert max(int(v) for v in V["itn"]) > 3
            V2 = e.lsmr_voronoi(S["b"], nd, ncells, xyz, seeds, 0.5, want_z=False, want_cell=False, **kw)
            assert V2["z"] is None and V2["cell"] is None and same_bits(V2["stats"], V["stats"])
            assert np.array_equal(V2["itn"], V["itn"]) and np.array_equal(V2["istop"], V["istop"])
            V3 = e.lsmr_voronoi(S["b"], nd, ncells, xyz, seeds, 0.5, **kw)
            for q in ("z", "cell", "stats", "istop", "itn") + EST:
                assert same_bits(V3[q], V[q]), q
            V1 = e.lsmr_voronoi(S["b"], nd, ncells, xyz, seeds[:1], 0.5, **kw)      # one member: its own mean, std 0
            assert same_bits(V1["z"][0], V["z"][0]) and not V1["stats"][1].any()
            assert same_bits(V1["stats"][0], V["z"][0][V["cell"][0]].astype(np.float64))
    finally:
        e.close(); e2.close()


@pytest.mark.parametrize("ncells", [1, 2, 64, 65])
def test_voronoi_tiny_cell_counts(boundary, ncells):
    """ncells = 1 (k_b_chain's len == 1 exit, localVecs = 1: every member the same one-column system), 2, and 64 / 65 on the wave edge
    of the chain: five members == the oracle's LSMR and dsa_lsmr on M_k under the three argument sets of the test above"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, n = c["ndata"], S["n"]
    xyz = lattice_xyz(c)
    seeds = invert.voronoi_seeds(n, ncells, 5, seed=3 + ncells)
    e, e2 = Engine(0), Engine(0)
    try:
        load(e, S)
        for local_size, itnlim in ((10, 400), (0, 100), (3, 7)):
            kw = dict(itnlim=itnlim, local_size=local_size)
            V = e.lsmr_voronoi(S["b"], nd, ncells, xyz, seeds, 0.5, **kw)
            assert V["z"].shape == (5, ncells) and V["cell"].shape == (5, n)
            assert np.array_equal(V["cell"], invert.voronoi_cells(xyz, seeds))
            assert_members(V, S, nd, ncells, 0.5, range(5), engine=e2, **kw)
            assert_stats(V)
            assert min(int(v) for v in V["itn"]) >= 1
    finally:
        e.close(); e2.close()


def test_voronoi_identity_tessellation(boundary):
    """ncells = n, seeds 0 .. n-1: every unknown is its own cell, and the result is the oracle's LSMR on the data rows alone"""
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, n = c["ndata"], S["n"]
    xyz = lattice_xyz(c)
    seeds = np.arange(n, dtype=np.int32)[None, :].repeat(2, axis=0)
    e = Engine(0)
    try:
        load(e, S)
        V = e.lsmr_voronoi(S["b"], nd, n, xyz, seeds, 1.0)
    finally:
        e.close()
    assert np.array_equal(V["cell"], seeds)
    nar = S["nar"]
    keep = np.flatnonzero(S["iw"][1:nar + 1] <= nd)
    assert np.array_equal(keep, np.arange(keep.size))                  # (the data rows come first and row by row: M is the COO's head)
    D = dict(m=nd, n=n, nar=keep.size, iw=np.concatenate([[keep.size], S["iw"][1:nar + 1][keep], S["iw"][nar + 1:][keep]]).astype(np.int32),
             rw=S["rw"][keep], b=S["b"][:nd].copy())
    want = inv.call_lsmr(L.oracle().dso_lsmr, D, 1.0)
    assert want["itn"] > 3
    assert_all_equal(dict(V, x=V["z"]), [want, want])
    assert same_bits(V["stats"][0], V["z"][0].astype(np.float64)) and not V["stats"][1].any()


@pytest.fixture(scope="module")
def taipei_forward():
    c = taipei.load()
    return c, L.call_boundary(load_library().dsa_calsurfg, c)


def test_voronoi_taipei_crosses_a_lane_group(taipei_forward):
    """70 members (two lane groups, the second partial) of 200 cells on the first iteration's Taipei system: members 0, 37, 63, 64, 69
    against the oracle and dsa_lsmr on M_k; dsa_lsmr, dsa_lsmr_batch and dsa_lsmr_tradeoff keep their bits around the call"""
    c, fwd = taipei_forward
    S = inv.build_system(c, fwd, c["obst"], 3.0, 4.0)
    nd, n = c["ndata"], S["n"]
    xyz = invert.voronoi_xyz(c, 1.0)
    seeds = invert.voronoi_seeds(n, 200, 70, seed=1)
    some = [0, 37, 63, 64, 69]
    ones = np.ones((1, S["m"]), np.float32)
    damp = float(c["damp"])
    e, e2 = Engine(0), Engine(0)
    try:
        load(e, S)
        own0 = e.lsmr(S["b"], damp)
        B0 = e.lsmr_batch(S["b"], ones, damp)
        T0 = e.lsmr_tradeoff(S["b"], nd, 4.0, [4.0, 1.0], [damp, 0.5])
        V = e.lsmr_voronoi(S["b"], nd, 200, xyz, seeds, damp)
        own1 = e.lsmr(S["b"], damp)
        B1 = e.lsmr_batch(S["b"], ones, damp)
        T1 = e.lsmr_tradeoff(S["b"], nd, 4.0, [4.0, 1.0], [damp, 0.5])
        V2 = e.lsmr_voronoi(S["b"], nd, 200, xyz, seeds, damp, want_z=False, want_cell=False)
        assert np.array_equal(V["cell"][some], invert.voronoi_cells(xyz, seeds[some]))
        assert_members(V, S, nd, 200, damp, some, engine=e2)
    finally:
        e.close(); e2.close()
    assert_stats(V)
    assert same_bits(V2["stats"], V["stats"]) and np.array_equal(V2["itn"], V["itn"]) and np.array_equal(V2["istop"], V["istop"])
    assert inv.same(own1, own0) == []
    assert inv.same(realisation(B1, 0), realisation(B0, 0)) == [] and inv.same(realisation(B0, 0), own0) == []
    for q in ("x", "measures", "istop", "itn") + EST:
        assert same_bits(T1[q], T0[q]), q
    assert max(int(v) for v in V["itn"]) > 3 and (V["stats"][1] > 0).any()


def banded_seeds(n, ncells, nreal, seed, nvx=47, nvy=47, layer=18):
    """voronoi_seeds whose first 25 seeds of every member are a 5 x 5 lattice (i = 3, 13, .., 43; j = 5, 10, .., 25) in one layer: with
    layers far apart, the cell of the lattice's centre (i 23, j 15) holds only unknowns with |di| <= 5, |dj| <= 2.5 around it"""
    fixed = np.array([layer * nvx * nvy + j * nvx + i for j in (5, 10, 15, 20, 25) for i in (3, 13, 23, 33, 43)])
    rest = np.setdiff1d(np.arange(n), fixed)
    rng = np.random.default_rng(seed)
    return np.stack([np.concatenate([fixed, rng.choice(rest, size=ncells - fixed.size, replace=False)]) for _ in range(nreal)]).astype(np.int32)


def test_voronoi_multiblock_system():
    """a 100 001 x 68 479 system over several SpMV blocks whose data rows touch no column of [40000, 41000): 70 members of 300 cells,
    members 0, 63, 69 against the oracle's LSMR on M_k; cell 12 of every member (inside the untouched range) has no data and z = 0"""
    nvx, nvy, nl, nd = 47, 47, 31, 31522
    M = SM.system(nd, nvx, nvy, nl, seed=11, skip=(40000, 41000))
    m, n, nar = M["m"], M["n"], M["rw"].size
    b = np.zeros(m, np.float32)
    b[:nd] = (SM.mix(np.arange(nd), 12) - 0.5).astype(np.float32)
    S = dict(m=m, n=n, nar=nar, iw=np.concatenate([[nar], M["row"], M["col"]]).astype(np.int32), rw=M["rw"], b=b)
    data_cols = M["col"][:M["nar_data"]] - 1
    assert not ((data_cols >= 40000) & (data_cols < 41000)).any() and n > 2 * 32768
    k, j, i = np.meshgrid(np.arange(nl), np.arange(nvy), np.arange(nvx), indexing="ij")
    xyz = np.stack([i.ravel() * 1.0, j.ravel() * 1.0, k.ravel() * 100.0], axis=1)
    seeds = banded_seeds(n, 300, 70, seed=5)
    some = [0, 63, 69]
    e = Engine(0)
    try:
        load(e, S)
        V = e.lsmr_voronoi(S["b"], nd, 300, xyz, seeds, 0.7, itnlim=35)
        V2 = e.lsmr_voronoi(S["b"], nd, 300, xyz, seeds, 0.7, want_z=False, want_cell=False, itnlim=35)
    finally:
        e.close()
    assert np.array_equal(V["cell"][some], invert.voronoi_cells(xyz, seeds[some]))
    inside = np.flatnonzero(V["cell"][0] == 12)
    assert inside.size > 0 and inside.min() >= 40000 and inside.max() < 41000
    nempty = assert_members(V, S, nd, 300, 0.7, some, itnlim=35)
    assert nempty >= len(some)
    assert not V["z"][:, 12].any()
    assert max(int(v) for v in V["itn"]) > 3
    assert_stats(V)
    assert same_bits(V2["stats"], V["stats"]) and np.array_equal(V2["itn"], V["itn"])


def test_voronoi_errors(boundary):
    c, fwd = boundary
    S = system(c, weight0=2.0, fwd=fwd)
    nd, m, n = c["ndata"], S["m"], S["n"]
    xyz = lattice_xyz(c)
    seeds = invert.voronoi_seeds(n, 8, 3, seed=2)
    e = Engine(0)
    try:
        e._mn = (m, n)                                                # (what spmv_load would note: the binding sizes its arrays from it)
        with pytest.raises(EngineError) as exc:
            e.lsmr_voronoi(S["b"], nd, 8, xyz, seeds, 1.0)
        assert exc.value.code == -5 and "dsa_spmv_load" in str(exc.value)            # DSA_ERR_STATE: no matrix yet
        load(e, S)
        want = e.lsmr(S["b"], 1.0)
        nan_xyz = xyz.copy(); nan_xyz[n // 2, 1] = np.nan
        inf_xyz = xyz.copy(); inf_xyz[0, 2] = np.inf
        low = seeds.copy(); low[1, 3] = -1
        high = seeds.copy(); high[2, 7] = n
        bad = [dict(ndata=0), dict(ndata=m + 1), dict(ncells=0, seeds=seeds[:, :0]), dict(ncells=n + 1, seeds=np.zeros((3, n + 1), np.int32)),
               dict(seeds=seeds[:0]), dict(seeds=low), dict(seeds=high), dict(xyz=nan_xyz), dict(xyz=inf_xyz), dict(damp=float("nan")),
               dict(damp=float("inf"))]
        for kw in bad:
            a = dict(ndata=nd, ncells=8, xyz=xyz, seeds=seeds, damp=1.0)
            a.update(kw)
            with pytest.raises(EngineError) as exc:
                e.lsmr_voronoi(S["b"], a["ndata"], a["ncells"], a["xyz"], a["seeds"], a["damp"])
            assert exc.value.code == -2, kw                                        # DSA_ERR_ARGUMENT
            assert inv.same(e.lsmr(S["b"], 1.0), want) == [], kw                   # the engine is still usable
        # null pointers, through the C ABI
        lib = load_library()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        bb = np.ascontiguousarray(S["b"], np.float32); sd = np.ascontiguousarray(seeds); pts = np.ascontiguousarray(xyz)
        istop = np.zeros(3, np.int32); itn = np.zeros(3, np.int32); est = np.zeros((3, 5), np.float32)
        full = [p(bb), p(pts), p(sd), p(istop), p(itn), p(est)]
        for hole in range(6):
            q = list(full); q[hole] = None
            rc = lib.dsa_lsmr_voronoi(e._h, 3, nd, 8, q[0], q[1], q[2], 1.0, 1e-6, 1e-6, 100.0, 400, 10, None, None, None, q[3], q[4], q[5])
            assert rc == -2, hole
        assert lib.dsa_lsmr_voronoi(e._h, 3, nd, 8, *full[:3], 1.0, 1e-6, 1e-6, 100.0, 400, 10, None, None, None, *full[3:]) == 0
        assert inv.same(e.lsmr(S["b"], 1.0), want) == []
        # ndata = m is valid (every row a data row), and so is one cell
        V = e.lsmr_voronoi(S["b"], m, 1, xyz, seeds[:, :1], 1.0)
        assert not V["cell"].any() and V["z"].shape == (3, 1)
    finally:
        e.close()


def test_invert_voronoi_writes_the_ensemble(tmp_path):
    """invert.run on the Taipei directory, maxiter 2, 64 members of 200 cells: every file of the plain run byte-identical, plus
    Voronoi.dat == the statistics of a direct dsa_lsmr_voronoi call on the second iteration's system with the same seeds; with
    voronoi_update the model after iteration 1 == dsa_model_update of float32(mean) on the host's copy"""
    c = taipei.load()
    n, nd = c["nparpi"], c["ndata"]
    plain, ens, upd = tmp_path / "plain", tmp_path / "ens", tmp_path / "upd"
    for d in (plain, ens, upd):
        d.mkdir()
    lp, le, lu = [], [], []
    invert.run(taipei.HERE, maxiter=2, out_dir=str(plain), log=lp.append)
    _, hist = invert.run(taipei.HERE, maxiter=2, out_dir=str(ens), log=le.append, voronoi=(64, 200), voronoi_seed=7)
    names = sorted(os.listdir(plain))
    assert sorted(os.listdir(ens)) == sorted(names + ["DSurfTomo.inVoronoi.dat"])
    for nm in names:
        assert (plain / nm).read_bytes() == (ens / nm).read_bytes(), nm
    assert [l for l in le if not l.startswith(" voronoi") and "(forward" not in l] == [l for l in lp if "(forward" not in l]
    assert sum(l.startswith(" voronoi") for l in le) == 1
    assert "voronoi" not in hist[0]
    hv = hist[1]["voronoi"]
    assert hv["realisations"] == 64 and hv["iteration"] == 2 and hv["cells"] == 200 and hv["seed"] == 8 and hv["chunk"] % 64 == 0 and hv["calls"] == 1
    assert hv["std_max"] > 0 and not hv["applied"]
    mean, std = invert.read_voronoi(str(ens / "DSurfTomo.inVoronoi.dat"))
    assert mean.size == n

    # the direct call: two plain iterations by hand, then dsa_lsmr_voronoi on the resident system of the second
    lib = invert.bind(load_library())
    obst = np.ascontiguousarray(c["obst"])
    xyz = np.ascontiguousarray(invert.voronoi_xyz(c, 1.0))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def direct(cbst, seed):
        sd = np.ascontiguousarray(invert.voronoi_seeds(n, 200, 64, seed))
        stats = np.zeros((2, n)); istop = np.zeros(64, np.int32); itn = np.zeros(64, np.int32); est = np.zeros((64, 5), np.float32)
        rc = lib.dsa_lsmr_voronoi(lib.dsa_dropin_engine(), 64, nd, 200, p(cbst), p(xyz), p(sd), C.c_float(c["damp"]), C.c_float(1e-6), C.c_float(1e-6),
                                  C.c_float(100.0), 400, 10, None, None, p(stats), p(istop), p(itn), p(est))
        assert rc == 0
        return stats, itn

    vsf = np.asfortranarray(c["vels"].copy())
    st1 = invert.iteration_device(lib, c, vsf, obst, lambda *_: None)
    stats1, _ = direct(st1["cbst"], 7)                                  # (the first iteration's ensemble, for the update below)
    st2 = invert.iteration_device(lib, c, vsf, obst, lambda *_: None)
    stats2, itn2 = direct(st2["cbst"], 8)
    fmt = lambda a: np.array([float("%10.5f" % v) for v in a])
    assert np.array_equal(mean, fmt(stats2[0])) and np.array_equal(std, fmt(stats2[1]))
    assert hv["itn_max"] == int(itn2.max()) and hv["std_max"] == float(stats2[1].max())

    # --voronoi-update: the ensemble in every iteration, its mean applied
    _, hu = invert.run(taipei.HERE, maxiter=2, out_dir=str(upd), log=lu.append, voronoi=(64, 200), voronoi_seed=7, voronoi_update=True)
    assert "voronoi" in hu[0] and "voronoi" in hu[1] and hu[0]["voronoi"]["applied"] and hu[0]["voronoi"]["seed"] == 7 and hu[1]["voronoi"]["seed"] == 8
    assert sum(l.startswith(" voronoi") for l in lu) == 2
    dv = np.ascontiguousarray(stats1[0].astype(np.float32))
    raw = (float(dv.min()), float(dv.max()))                            # (dsa_model_update clips dv in place: main.f90:520-523)
    host = np.asfortranarray(c["vels"].copy())
    lib.dsa_model_update(c["nx"], c["ny"], c["nz"], p(dv), p(host), c["minvel"], c["maxvel"])
    want = tmp_path / "want.iter001"
    invert.write_model(str(want), c, host)
    assert (upd / "DSurfTomo.inMeasure.dat.iter001").read_bytes() == want.read_bytes()
    assert (hu[0]["dv_min"], hu[0]["dv_max"]) == raw
    assert hu[0]["itn"] == hist[0]["itn"] and hu[0]["istop"] == hist[0]["istop"]          # dsa_lsmr still ran, on the same first system
    assert (upd / "DSurfTomo.inMeasure.dat.iter001").read_bytes() != (plain / "DSurfTomo.inMeasure.dat.iter001").read_bytes()
