"""The host side of the regularisation trade-off sweep (dsurftomo_amd.invert): the lists of weights and damps, the member grid, the
corner of the curve, the chunk size of the dsa_lsmr_tradeoff calls, the checks of --tradeoff-* before the library is loaded and the
writer of <input>Tradeoff.dat.  Host code only: runs without a GPU."""
import numpy as np
import pytest

from dsurftomo_amd import invert


@pytest.mark.parametrize("text,want", [("2", [2.0]), ("0,0.5, 4 ,1e2", [0.0, 0.5, 4.0, 100.0]), ("3,1,2", [3.0, 1.0, 2.0])])
def test_parse_tradeoff_list(text, want):
    assert invert.parse_tradeoff_list(text) == want


@pytest.mark.parametrize("text", ["", "1,x", "-1", "nan", "1,,2", "inf", "2,-0.5"])
def test_parse_tradeoff_list_rejects(text):
    with pytest.raises(ValueError):
        invert.parse_tradeoff_list(text)


def test_tradeoff_grid_is_weight_major():
    w, d = invert.tradeoff_grid([1.0, 2.0, 4.0], [0.5, 0.25])
    assert w.dtype == np.float32 and d.dtype == np.float32
    assert w.tolist() == [1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    assert d.tolist() == [0.5, 0.25, 0.5, 0.25, 0.5, 0.25]
    w, d = invert.tradeoff_grid([3.0], [1.0])
    assert w.tolist() == [3.0] and d.tolist() == [1.0]


def l_curve(nflat=5, nsteep=4, flat_slope=-0.02, steep_slope=-30.0):
    """(misfit, rough) over increasing weight: log misfit against log rough is a straight line of slope flat_slope while the
    roughness falls by a factor 2 per point, then one of slope steep_slope while it falls by 2 per cent per point; the vertex is
    point nflat"""
    lr = [5.0 - np.log(2.0) * k for k in range(nflat + 1)]
    lm = [0.0 + flat_slope * (v - lr[0]) for v in lr]
    for k in range(1, nsteep + 1):
        lr.append(lr[nflat] - 0.02 * k)
        lm.append(lm[nflat] + steep_slope * (-0.02 * k))
    return np.exp(lm), np.exp(lr)


def test_lcurve_corner_finds_the_vertex():
    mis, rou = l_curve()
    assert invert.lcurve_corner(mis, rou) == 5
    mis, rou = l_curve(nflat=2, nsteep=6)
    assert invert.lcurve_corner(mis, rou) == 2
    # the mirror image (the misfit rises first, then the roughness falls: an inverted L) has no positive curvature
    assert invert.lcurve_corner(mis[::-1], rou[::-1]) is None


def test_lcurve_corner_straight_line_and_too_few_points():
    rou = np.exp(np.linspace(4.0, 0.0, 9))
    mis = np.exp(0.5 * np.linspace(0.0, 4.0, 9))                       # log misfit = 2 - log rough / 2: a straight line up to rounding
    assert invert.lcurve_corner(mis, rou) is None
    assert invert.lcurve_corner(2.0 ** np.arange(9.0), 2.0 ** -np.arange(9.0)) is None
    assert invert.lcurve_corner(mis[:2], rou[:2]) is None
    assert invert.lcurve_corner([], []) is None
    m3, r3 = l_curve(nflat=1, nsteep=1)
    assert invert.lcurve_corner(m3, r3) == 1                            # three points are enough
    assert invert.lcurve_corner([0.0, m3[1], m3[2]], r3) is None        # ... two usable ones are not


def test_lcurve_corner_skips_zeros():
    mis, rou = l_curve()
    mis2 = np.insert(mis, [0, 3, 5], [0.0, 1.0, -1.0])
    rou2 = np.insert(rou, [0, 3, 5], [7.0, 0.0, 3.0])
    # the vertex (index 5 before the insertions) has moved behind three inserted points, none of which is usable
    assert invert.lcurve_corner(mis2, rou2) == 8
    assert invert.lcurve_corner(np.zeros(6), rou[:6]) is None


def tradeoff_bytes(m, n, nar, L, R):
    """the device buffers of a dsa_lsmr_tradeoff call (lsmr_batch.hip): batch_begin's for R members with the temporary R n + m + R, the
    two coefficient copies, the measures' partials and results (fp64)"""
    G = (R + 63) // 64
    Rp = 64 * G
    L = max(0, min(L, m, n))
    mx = max(m, n)
    floats = 2 * G * m * 64 + 4 * G * n * 64 + G * n * 64 * L + 12 * Rp + 3 * Rp + G * mx * 64 + G * (-(-mx // 256)) * 64 + R * n + m + R
    doubles = G * (-(-m // 64)) * 64 * 2 + G * (-(-n // 1024)) * 64 + 3 * Rp
    return 4 * floats + 8 * nar + 8 * doubles + 4


@pytest.mark.parametrize("m,n,L", [(4109, 2048, 10), (100001, 68479, 10), (100001, 68479, 0), (3_000_000, 1_500_000, 10),
                                   (40_000_000, 20_000_000, 10), (10, 5, 10)])
def test_tradeoff_chunk(m, n, L):
    nar = 60 * (m - n) + 7 * n
    k = invert.tradeoff_chunk(m, n, nar, L)
    assert k % 64 == 0 and 64 <= k <= 4096
    budget = 32 << 30
    if k > 64:
        assert tradeoff_bytes(m, n, nar, L, k) <= budget
        assert invert.tradeoff_bytes(m, n, nar, L, k) >= tradeoff_bytes(m, n, nar, L, k)
    if k < 4096:                                           # lowered only as far as needed
        assert invert.tradeoff_bytes(m, n, nar, L, k + 64) > budget
    assert invert.tradeoff_chunk(m, n, nar, L) == k           # pure
    assert invert.tradeoff_chunk(m, n, nar, L, budget=1) == 64


@pytest.mark.parametrize("argv", [["--tradeoff-weights", "1,2", "--host-rows"], ["--tradeoff-weights", ""], ["--tradeoff-weights", "1,-2"],
                                  ["--tradeoff-weights", "1,2", "--tradeoff-damps", "x"], ["--tradeoff-weights", "1,2", "--tradeoff-damps", "-1"],
                                  ["--tradeoff-weights", "1,2", "--tradeoff-iter", "0"], ["--tradeoff-weights", "1,2", "--tradeoff-iter", "3", "--maxiter", "2"],
                                  ["--tradeoff-damps", "1"]])
def test_cli_rejects_bad_tradeoff_arguments_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(tradeoff_weights=[1.0, 2.0], host_rows=True), dict(tradeoff_weights=[]), dict(tradeoff_weights=[1.0, -2.0]),
                                dict(tradeoff_weights=[1.0], tradeoff_damps=[]), dict(tradeoff_weights=[1.0], tradeoff_damps=[float("nan")]),
                                dict(tradeoff_weights=[1.0], tradeoff_iter=0), dict(tradeoff_weights=[1.0], tradeoff_iter=3, maxiter=2),
                                dict(tradeoff_damps=[1.0]), dict(tradeoff_weights=[1.0], tradeoff_chunk=100)])
def test_run_rejects_bad_tradeoff_arguments_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)


def test_tradeoff_file_round_trips(tmp_path):
    f = np.float32
    rng = np.random.default_rng(2)
    members = [dict(weight=float(f(w)), damp=float(f(d)), misfit=float(rng.random() * 10), rough=float(rng.random() * 1e-3), xnorm=float(rng.random()),
                    itn=int(rng.integers(0, 400)), istop=int(rng.integers(0, 8)), dv_min=float(f(-rng.random())), dv_max=float(f(rng.random())))
               for w in (0.0, 0.1, 2.0, 11.3) for d in (0.0, 1.0 / 3.0)]
    path = tmp_path / "DSurfTomo.inTradeoff.dat"
    invert.write_tradeoff(str(path), members)
    rows = path.read_text().splitlines()
    assert len(rows) == len(members) and all(len(r.split()) == 9 for r in rows)
    assert invert.read_tradeoff(str(path)) == members
    path.write_text("1 2 3\n")
    with pytest.raises(ValueError):
        invert.read_tradeoff(str(path))


def test_tradeoff_corners_per_damp():
    mis, rou = l_curve()
    weights = [0.1 * 2 ** k for k in range(len(mis))]
    members = []
    for i, w in enumerate(weights):
        members.append(dict(weight=w, damp=0.5, misfit=float(mis[i]), rough=float(rou[i])))
        members.append(dict(weight=w, damp=2.0, misfit=float(2.0 ** i), rough=float(2.0 ** -i)))      # a straight line: no corner
    got = invert.tradeoff_corners(members)
    assert got == [dict(damp=0.5, weight=weights[5], member=10), dict(damp=2.0, weight=None, member=None)]
    # the order of the weights in the file does not matter: the curve runs over increasing weight
    assert invert.tradeoff_corners(members[::-1])[1] == dict(damp=0.5, weight=weights[5], member=len(members) - 1 - 10)
