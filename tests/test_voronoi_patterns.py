"""The host side of the Poisson-Voronoi ensemble (dsurftomo_amd.invert): the points and the seeds of the tessellations, the numpy
restatement of dsa_lsmr_voronoi's cell assignment and of its ensemble statistics, the chunk size of the calls, the checks of
--voronoi* before the library is loaded and the writer of <input>Voronoi.dat.  Host code only: runs without a GPU."""
import numpy as np
import pytest

from dsurftomo_amd import invert


def grid(nx=6, ny=7, nz=4):
    """a small model description: what unknown_coords / write_model read"""
    f = np.float32
    return dict(nx=nx, ny=ny, nz=nz, goxd=f(25.2), gozd=f(121.35), dvxd=f(0.03), dvzd=f(0.05), depz=np.array([0.0, 0.4, 1.1, 2.5][:nz], f),
                nparpi=(nx - 2) * (ny - 2) * (nz - 1))


def test_cells_every_seed_owns_itself():
    rng = np.random.default_rng(3)
    xyz = rng.standard_normal((200, 3))
    seeds = invert.voronoi_seeds(200, 17, 5, seed=4)
    cell = invert.voronoi_cells(xyz, seeds)
    assert cell.shape == (5, 200) and cell.dtype == np.int32
    for k in range(5):
        assert cell[k, seeds[k]].tolist() == list(range(17))
        # brute force, one unknown at a time
        for j in (0, 7, 199):
            d = xyz[j] - xyz[seeds[k]]
            assert cell[k, j] == int(np.argmin((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]))


def test_cells_ties_go_to_the_lowest_index():
    xyz = np.array([[0.0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]])
    assert invert.voronoi_cells(xyz, [[0, 2, 4]]).tolist() == [[0, 0, 1, 1, 2]]       # unknowns 1 and 3 lie half way
    assert invert.voronoi_cells(xyz, [[4, 2, 0]]).tolist() == [[2, 1, 1, 0, 0]]       # ... the lowest CELL index, not the lowest unknown
    same = np.zeros((4, 3))
    assert invert.voronoi_cells(same, [[3, 1]]).tolist() == [[0, 0, 0, 0]]
    # blocks of the restatement do not change it
    rng = np.random.default_rng(8)
    pts = rng.integers(0, 4, (300, 3)).astype(np.float64)                            # many exact ties
    sd = invert.voronoi_seeds(300, 40, 2, 1)
    assert np.array_equal(invert.voronoi_cells(pts, sd, block=7), invert.voronoi_cells(pts, sd))


def test_cells_single_cell_is_all_zeros():
    xyz = np.random.default_rng(1).standard_normal((50, 3))
    assert not invert.voronoi_cells(xyz, [[13], [2]]).any()


def test_seeds():
    a = invert.voronoi_seeds(500, 60, 6, seed=9)
    assert a.shape == (6, 60) and a.dtype == np.int32 and a.min() >= 0 and a.max() < 500
    assert all(len(set(row.tolist())) == 60 for row in a)                             # distinct within a member
    assert np.array_equal(a, invert.voronoi_seeds(500, 60, 6, seed=9))                # reproducible
    assert not np.array_equal(a, invert.voronoi_seeds(500, 60, 6, seed=10))
    assert all(not np.array_equal(a[0], a[k]) for k in range(1, 6))                   # members differ
    assert np.array_equal(a[:3], invert.voronoi_seeds(500, 60, 3, seed=9))            # members are drawn in order
    assert sorted(invert.voronoi_seeds(12, 12, 1, 0)[0].tolist()) == list(range(12))
    for bad in (0, 13):
        with pytest.raises(ValueError):
            invert.voronoi_seeds(12, bad, 1, 0)


def test_xyz():
    c = grid()
    co = invert.unknown_coords(c)
    a = invert.voronoi_xyz(c, 1.0)
    b = invert.voronoi_xyz(c, 2.5)
    assert a.shape == (c["nparpi"], 3) and a.dtype == np.float64
    assert np.array_equal(a[:, :2], b[:, :2]) and np.array_equal(b[:, 2], 2.5 * co[:, 2]) and np.array_equal(a[:, 2], co[:, 2])
    d2r = np.pi / 180.0
    assert np.array_equal(a[:, 0], 6371.0 * (co[:, 0] - co[:, 0].mean()) * d2r)
    assert np.array_equal(a[:, 1], 6371.0 * np.cos(co[:, 0].mean() * d2r) * (co[:, 1] - co[:, 1].mean()) * d2r)
    # kilometres: one latitude step of 0.03 degrees is 3.336 km
    assert abs(abs(a[1, 0] - a[0, 0]) - 6371.0 * 0.03 * d2r) < 1e-3


def test_stats_is_the_stated_loop():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((7, 30)).astype(np.float32)
    got = invert.voronoi_stats(x)
    for j in (0, 11, 29):
        s = 0.0
        for k in range(7):
            s = s + float(x[k, j])
        mean = s / 7.0
        ss = 0.0
        for k in range(7):
            ss = ss + (float(x[k, j]) - mean) * (float(x[k, j]) - mean)
        assert got[0, j] == mean and got[1, j] == np.sqrt(ss / 6.0)
    one = invert.voronoi_stats(x[:1])
    assert np.array_equal(one[0], x[0].astype(np.float64)) and not one[1].any()


def voronoi_bytes(ndata, n, ncells, nnz, L, nreal):
    """the buffers of csrc/lsmr_batch.hip (dsa_lsmr_voronoi), counted from their ensure() calls"""
    Rp = 64 * ((nreal + 63) // 64)
    G = Rp // 64
    Lv = max(0, min(L, ndata, ncells))
    mx = max(ndata, ncells)
    batch = 4 * (2 * Rp * ndata + (4 + Lv) * Rp * ncells + Rp * mx + G * -(-mx // 256) * 64 + 12 * Rp + 3 * Rp + nreal * ncells + ndata)
    own = 4 * (3 * Rp * n + Rp * ndata + Rp * nnz + Rp * (ncells + 1) + nnz + 3 * 64 * nnz + nreal * ncells) + 8 * 5 * n
    return batch + own


@pytest.mark.parametrize("ndata,n,ncells,nnz,L", [(6106, 2160, 200, 360000, 10), (31522, 68479, 300, 1400000, 10), (31522, 68479, 1000, 1400000, 0),
                                                  (400000, 500000, 5000, 30000000, 10)])
def test_voronoi_chunk(ndata, n, ncells, nnz, L):
    k = invert.voronoi_chunk(ndata, n, ncells, nnz, L)
    assert k % 64 == 0 and 64 <= k <= 4096
    budget = 32 << 30
    assert invert.voronoi_bytes(ndata, n, ncells, nnz, L, k) >= voronoi_bytes(ndata, n, ncells, nnz, L, k)
    if k > 64:
        assert invert.voronoi_bytes(ndata, n, ncells, nnz, L, k) <= budget
    if k < 4096:                                           # lowered only as far as needed
        assert invert.voronoi_bytes(ndata, n, ncells, nnz, L, k + 64) > budget
    assert invert.voronoi_chunk(ndata, n, ncells, nnz, L, budget=1) == 64
    ks = [invert.voronoi_chunk(ndata, n, ncells, nnz, L, budget=b << 30) for b in (1, 2, 8, 32, 128)]
    assert ks == sorted(ks)                                # monotone in the budget
    assert all(v % 64 == 0 and v >= 64 for v in ks)


@pytest.mark.parametrize("text,want", [("64,300", (64, 300)), ("1,1", (1, 1)), (" 256 , 1000", (256, 1000))])
def test_parse_voronoi(text, want):
    assert invert.parse_voronoi(text) == want


@pytest.mark.parametrize("text", ["", "64", "64,", "64,300,2", "0,300", "64,0", "-1,5", "a,b", "6.5,300"])
def test_parse_voronoi_rejects(text):
    with pytest.raises(ValueError):
        invert.parse_voronoi(text)


def test_check_voronoi():
    invert.check_voronoi(None)
    invert.check_voronoi((64, 300), True, False, 2.0, 0.5, 1000, 128)
    invert.check_voronoi((1, 1000), nunknowns=1000)
    bad = [dict(voronoi=None, update=True), dict(voronoi=(64, 300), host_rows=True), dict(voronoi=(0, 300)), dict(voronoi=(64, 0)),
           dict(voronoi=(64,)), dict(voronoi=(64.5, 300)), dict(voronoi=(64, 300), zscale=float("nan")), dict(voronoi=(64, 300), zscale=-1.0),
           dict(voronoi=(64, 300), damp=-0.5), dict(voronoi=(64, 300), damp=float("inf")), dict(voronoi=(64, 1001), nunknowns=1000),
           dict(voronoi=(64, 300), chunk=100), dict(voronoi=(64, 300), chunk=0)]
    for kw in bad:
        with pytest.raises(ValueError):
            invert.check_voronoi(**kw)


@pytest.mark.parametrize("argv", [["--voronoi", "64"], ["--voronoi", "0,300"], ["--voronoi", "64,x"], ["--voronoi", "64,300", "--host-rows"],
                                  ["--voronoi-update"], ["--voronoi", "64,300", "--voronoi-zscale", "nan"], ["--voronoi", "64,300", "--voronoi-damp", "-1"],
                                  ["--voronoi", "64,300", "--voronoi-seed", "x"]])
def test_cli_rejects_bad_voronoi_arguments_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(voronoi=(64, 300), host_rows=True), dict(voronoi_update=True), dict(voronoi=(64, 0)), dict(voronoi=(64, 300), voronoi_chunk=96),
                                dict(voronoi=(64, 300), voronoi_damp=float("nan"))])
def test_run_rejects_bad_voronoi_arguments_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)


def test_voronoi_file_round_trips(tmp_path):
    c = grid()
    rng = np.random.default_rng(6)
    mean = rng.standard_normal(c["nparpi"]) * 0.2
    std = rng.random(c["nparpi"]) * 0.05
    path = tmp_path / "DSurfTomo.inVoronoi.dat"
    invert.write_voronoi(str(path), c, mean, std)
    lines = path.read_text().splitlines()
    assert len(lines) == c["nparpi"] and all(len(l) == 50 for l in lines)
    m2, s2 = invert.read_voronoi(str(path))
    assert np.array_equal(m2, np.array([float("%10.5f" % v) for v in mean])) and np.array_equal(s2, np.array([float("%10.5f" % v) for v in std]))
    # the first three columns are those of the other model files (the layout of <input>Std.dat)
    ref = tmp_path / "std.dat"
    invert.write_std(str(ref), c, mean)
    assert [l[:40] for l in lines] == ref.read_text().splitlines()
    path.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        invert.read_voronoi(str(path))
