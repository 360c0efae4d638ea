"""The host side of the linearised resolution tests (dsurftomo_amd.invert): checkerboard patterns, the unknowns' coordinates, the chunk
size of the PSF solves, the recovery metrics, the CLI's checks of --resolution / --checkerboard and write_model's extra columns.  Host
code only: runs without a GPU."""
import numpy as np
import pytest

from dsurftomo_amd import invert


def small(nx=7, ny=6, nz=4):
    f = np.float32
    return dict(nx=nx, ny=ny, nz=nz, nparpi=(nx - 2) * (ny - 2) * (nz - 1), goxd=f(25.3), gozd=f(121.2), dvxd=f(0.05), dvzd=f(0.07),
                depz=np.array([0.0, 1.5, 3.25, 7.0, 9.5, 12.0][:nz], f))


def test_checkerboard_values_signs_and_edges():
    c = small(nx=9, ny=7, nz=5)                           # interior 7 x 5 x 4: cells of 3, 2, 3 do not divide it
    v = invert.checkerboard(c, (3, 2, 3))
    assert v.dtype == np.float32 and v.shape == (c["nparpi"],)
    g = v.reshape(4, 5, 7)                                # [k][j][i]: i (latitude index) fastest
    assert set(np.unique(v).tolist()) == {float(np.float32(-0.1)), float(np.float32(0.1))}
    assert g[0, 0, 0] == np.float32(0.1)                  # the first block is positive
    for k in range(4):
        for j in range(5):
            for i in range(7):
                want = np.float32(0.1) if (i // 3 + j // 2 + k // 3) % 2 == 0 else np.float32(-0.1)
                assert g[k, j, i] == want, (i, j, k)
    # block edges: the sign flips between i = 2 and 3, 5 and 6, j = 1 and 2, k = 2 and 3 and nowhere else inside a block
    assert g[0, 0, 2] == g[0, 0, 0] and g[0, 0, 3] == -g[0, 0, 2] and g[0, 0, 6] == -g[0, 0, 5]
    assert g[0, 1, 0] == g[0, 0, 0] and g[0, 2, 0] == -g[0, 1, 0]
    assert g[2, 0, 0] == g[0, 0, 0] and g[3, 0, 0] == -g[2, 0, 0]
    # a cell larger than the grid: one positive block
    assert (invert.checkerboard(c, (50, 50, 50)) == np.float32(0.1)).all()
    # cell 1 along every axis: neighbours differ
    one = invert.checkerboard(c, (1, 1, 1)).reshape(4, 5, 7)
    assert (one[:, :, 1:] == -one[:, :, :-1]).all() and (one[:, 1:, :] == -one[:, :-1, :]).all() and (one[1:] == -one[:-1]).all()


def test_checkerboard_amplitude():
    c = small()
    v = invert.checkerboard(c, (2, 2, 1), amplitude=0.25)
    assert set(np.abs(v).tolist()) == {0.25}


@pytest.mark.parametrize("text,want", [("4,4,2", (4, 4, 2)), (" 1, 2 ,3", (1, 2, 3))])
def test_parse_checkerboard(text, want):
    assert invert.parse_checkerboard(text) == want


@pytest.mark.parametrize("text", ["4,4", "4,4,2,1", "4,x,2", "0,4,2", "4,-1,2", "", "4.5,4,2"])
def test_parse_checkerboard_rejects(text):
    with pytest.raises(ValueError):
        invert.parse_checkerboard(text)


def test_unknown_coords_match_the_model_rows(tmp_path):
    c = small()
    vsf = np.zeros((c["nx"], c["ny"], c["nz"]), np.float32)
    path = tmp_path / "m.dat"
    invert.write_model(str(path), c, vsf)
    rows = path.read_text().splitlines()
    xyz = invert.unknown_coords(c)
    assert xyz.shape == (c["nparpi"], 3) and xyz.dtype == np.float64
    assert len(rows) == c["nparpi"]
    for q, line in enumerate(rows):                        # row q of a model file is unknown q
        lat, lon, dep = xyz[q]
        assert line[:30] == "%10.5f%10.5f%10.5f" % (lon, lat, dep), q
    # unknown q = k (ny-2)(nx-2) + j (nx-2) + i
    nx, ny = c["nx"], c["ny"]
    q = 2 * (ny - 2) * (nx - 2) + 3 * (nx - 2) + 4
    f = np.float32
    assert xyz[q, 2] == c["depz"][2]
    assert xyz[q, 0] == np.float64(f(c["goxd"] - f(f(4) * c["dvxd"])))
    assert xyz[q, 1] == np.float64(f(c["gozd"] + f(f(3) * c["dvzd"])))


def test_unknowns_grid_round_trip():
    c = small()
    v = np.arange(c["nparpi"], dtype=np.float64)
    g = invert.unknowns_grid(c, v)
    assert g.shape == (c["nx"], c["ny"], c["nz"])
    assert g[0].sum() == 0 and g[-1].sum() == 0 and g[:, 0].sum() == 0 and g[:, -1].sum() == 0 and g[:, :, -1].sum() == 0
    assert g[1 + 2, 1 + 1, 1] == v[1 * (c["ny"] - 2) * (c["nx"] - 2) + 1 * (c["nx"] - 2) + 2]


def test_write_model_one_column_is_unchanged(tmp_path):
    """write_model(path, c, vsf) writes what it wrote before the extra columns existed: the '(5f10.5)' rows, byte for byte"""
    c = small()
    rng = np.random.default_rng(4)
    vsf = (2.5 + rng.random((c["nx"], c["ny"], c["nz"]))).astype(np.float32)
    invert.write_model(str(tmp_path / "a.dat"), c, vsf)
    f = np.float32
    want = []
    for k in range(c["nz"] - 1):
        for j in range(c["ny"] - 2):
            for i in range(c["nx"] - 2):
                lon = f(c["gozd"] + f(f(j) * c["dvzd"]))
                lat = f(c["goxd"] - f(f(i) * c["dvxd"]))
                want.append("%10.5f%10.5f%10.5f%10.5f\n" % (lon, lat, c["depz"][k], vsf[i + 1, j + 1, k]))
    assert (tmp_path / "a.dat").read_text() == "".join(want)
    # extra columns follow the fourth, in the same format
    e1 = vsf * np.float32(2)
    e2 = -vsf
    invert.write_model(str(tmp_path / "b.dat"), c, vsf, e1, e2)
    rows_a = (tmp_path / "a.dat").read_text().splitlines()
    rows_b = (tmp_path / "b.dat").read_text().splitlines()
    assert len(rows_a) == len(rows_b)
    q = 0
    for k in range(c["nz"] - 1):
        for j in range(c["ny"] - 2):
            for i in range(c["nx"] - 2):
                assert rows_b[q] == rows_a[q] + "%10.5f%10.5f" % (e1[i + 1, j + 1, k], e2[i + 1, j + 1, k])
                q += 1


def test_write_std_unchanged(tmp_path):
    c = small()
    std = np.linspace(0.0, 1.0, c["nparpi"])
    invert.write_std(str(tmp_path / "s.dat"), c, std)
    got = np.loadtxt(str(tmp_path / "s.dat"))
    assert np.allclose(got[:, 3], std, atol=5e-6)


def batch_bytes(m, n, L, R):
    """the batch buffers of dsa_lsmr_batch for R realisations (lsmr_batch.hip: batch_begin and dsa_lsmr_batch's temporary)"""
    G = (R + 63) // 64
    Rp = 64 * G
    L = max(0, min(L, m, n))
    mx = max(m, n)
    floats = (2 * G * m * 64 + 4 * G * n * 64 + G * n * 64 * L + 12 * Rp + 3 * Rp + G * mx * 64 + G * (-(-mx // 256)) * 64
              + max(R * m + m, R * n))
    return 4 * floats


@pytest.mark.parametrize("m,n,L", [(4109, 2048, 10), (100001, 68479, 10), (100001, 68479, 0), (3_000_000, 1_500_000, 10),
                                   (40_000_000, 20_000_000, 10), (10, 5, 10)])
def test_resolution_chunk(m, n, L):
    k = invert.resolution_chunk(m, n, L)
    assert k % 64 == 0 and 64 <= k <= 4096
    budget = 32 << 30
    if k > 64:
        assert batch_bytes(m, n, L, k) <= budget
    if k < 4096:                                           # lowered only as far as needed
        assert batch_bytes(m, n, L, k + 64) > budget
    assert invert.resolution_chunk(m, n, L) == k           # pure


def test_resolution_chunk_values():
    assert invert.resolution_chunk(4109, 2048, 10) == 4096
    assert invert.resolution_chunk(100001, 68479, 10) == 4096
    assert invert.resolution_chunk(3_000_000, 1_500_000, 10) < 4096
    assert invert.resolution_chunk(4109, 2048, 10, budget=batch_bytes(4109, 2048, 10, 640)) == 640


def test_recovery_metrics_match_numpy():
    rng = np.random.default_rng(3)
    nl, per = 4, 30
    m = np.where(rng.random(nl * per) < 0.5, 0.1, -0.1).astype(np.float32)
    x = (0.6 * m + 0.02 * rng.standard_normal(nl * per)).astype(np.float32)
    got = invert.recovery_metrics(m, x, nl)
    m64, x64 = m.astype(np.float64), x.astype(np.float64)
    assert got["corr"] == pytest.approx(np.corrcoef(m64, x64)[0, 1], rel=1e-12)
    assert got["gain"] == pytest.approx(np.dot(m64, x64) / np.dot(m64, m64), rel=1e-12)
    assert len(got["corr_layers"]) == nl and len(got["gain_layers"]) == nl
    for k in range(nl):
        a, b = m64[k * per:(k + 1) * per], x64[k * per:(k + 1) * per]
        assert got["corr_layers"][k] == pytest.approx(np.corrcoef(a, b)[0, 1], rel=1e-12)
        assert got["gain_layers"][k] == pytest.approx(np.dot(a, b) / np.dot(a, a), rel=1e-12)
    # exact cases: x = 2 m (correlation 1, gain 2); x = 0 (no correlation defined: 0, gain 0); x = -m
    e = invert.recovery_metrics(m, 2 * m, nl)
    assert e["corr"] == pytest.approx(1.0, abs=1e-12) and e["gain"] == pytest.approx(2.0, rel=1e-12)
    z = invert.recovery_metrics(m, np.zeros_like(m), nl)
    assert z["corr"] == 0.0 and z["gain"] == 0.0 and z["corr_layers"] == [0.0] * nl
    n = invert.recovery_metrics(m, -m, nl)
    assert n["corr"] == pytest.approx(-1.0, abs=1e-12) and n["gain"] == pytest.approx(-1.0, rel=1e-12)


def test_psf_columns():
    """R_jj, horizontal and vertical PSF lengths sqrt(sum x^2 dh^2 / sum x^2), sqrt(sum x^2 dz^2 / sum x^2); no data: zeros"""
    psf = np.array([[0.5, 2.0, 8.0, 18.0], [0.0, 0.0, 0.0, 0.0], [0.25, 4.0, 100.0, 0.0]])
    rjj, lh, lv, nodata = invert.psf_columns(psf)
    assert np.array_equal(rjj, [0.5, 0.0, 0.25])
    assert np.allclose(lh, [2.0, 0.0, 5.0]) and np.allclose(lv, [3.0, 0.0, 0.0])
    assert nodata == 1


def test_great_circle_km():
    d = invert.great_circle_km(np.array([0.0, 10.0]), np.array([0.0, 20.0]), 0.0, 20.0)
    assert d[1] == pytest.approx(np.radians(10.0) * 6371.0, rel=1e-12)
    assert d[0] == pytest.approx(np.radians(20.0) * 6371.0, rel=1e-12)
    assert invert.great_circle_km(np.array([25.0]), np.array([121.5]), 25.0, 121.5)[0] == 0.0


@pytest.mark.parametrize("argv", [["--resolution", "--host-rows"], ["--checkerboard", "4,4,2", "--host-rows"], ["--checkerboard", "4,4"],
                                  ["--checkerboard", "4,0,2"], ["--checkerboard", "a,b,c"]])
def test_cli_rejects_bad_resolution_arguments_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(resolution=True, host_rows=True), dict(checkerboard=[(4, 4, 2)], host_rows=True),
                                dict(checkerboard=[(4, 0, 2)]), dict(checkerboard=[(4, 4)]), dict(resolution=True, resolution_chunk=0)])
def test_run_rejects_bad_resolution_arguments_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)
