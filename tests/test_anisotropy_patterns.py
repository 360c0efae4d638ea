"""The host side of dsurftomo_amd.anisotropy: the three checkerboard models of a board, the columns and the leakage
figures taken from block PSF measures, the parser's refusals and the two file kinds.  No GPU and no library: nothing here loads it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _libs as L
import synth
from dsurftomo_amd import anisotropy as A
from dsurftomo_amd import invert


def case():
    return synth.boundary_case(nx=7, ny=6, nz=4)


def test_checkerboard_models_blocks_signs_amplitudes():
    c = case()
    n = c["nparpi"]
    cell = (2, 3, 1)
    M = A.azimuthal_checkerboards(c, cell, 0.03)
    assert M.shape == (3, 3 * n) and M.dtype == np.float32
    sign = np.sign(invert.checkerboard(c, cell))
    assert set(np.unique(sign)) == {-1.0, 1.0} and sign[0] == 1.0
    for B, amp in enumerate((np.float32(0.1), np.float32(0.03), np.float32(0.03))):
        blocks = M[B].reshape(3, n)
        assert (blocks[B] == sign * amp).all()
        for other in range(3):
            if other != B:
                assert not blocks[other].any()
    # the default amplitude: 0.04, i.e. 2 % peak to peak (50 sqrt(gc^2 + gs^2) = 2)
    D = A.azimuthal_checkerboards(c, cell)
    assert np.abs(D[1, n:2 * n]).max() == np.float32(0.04) and np.abs(D[2, 2 * n:]).min() == np.float32(0.04)
    assert abs(float(invert.azimuthal_strength(D[1, n:2 * n], 0.0).max()) - 2.0) < 1e-6
    # fast axes: gc = +-G is 0 / 90 degrees, gs = +-G is 45 / 135 (= -45) degrees
    assert set(np.round(np.abs(invert.azimuthal_axis(D[1, n:2 * n], 0.0 * D[1, n:2 * n]))).tolist()) == {0.0, 90.0}
    assert set(np.round(invert.azimuthal_axis(0.0 * D[2, 2 * n:], D[2, 2 * n:])).tolist()) == {45.0, -45.0}


def handmade_psf():
    """nb = 2 cells, three blocks: six spikes; spike 3 (block 1, cell 1) has no energy at all, spike 4 none in its own block"""
    psf = np.zeros((6, 3, 4))
    # spike 0 (Vs, cell 0): own block energy 4 with sums 36 and 16 -> lengths 3 and 2; leaks 1 into gc and 3 into gs
    psf[0, 0] = (0.5, 4.0, 36.0, 16.0); psf[0, 1] = (0.1, 1.0, 0.0, 0.0); psf[0, 2] = (-0.2, 3.0, 0.0, 0.0)
    psf[1, 0] = (0.25, 1.0, 1.0, 0.0); psf[1, 1] = (0.0, 0.0, 0.0, 0.0); psf[1, 2] = (0.0, 0.0, 0.0, 0.0)
    psf[2, 1] = (0.4, 6.0, 6.0, 24.0); psf[2, 0] = (0.3, 2.0, 0.0, 0.0); psf[2, 2] = (0.0, 0.0, 0.0, 0.0)
    psf[4, 2] = (0.0, 0.0, 0.0, 0.0); psf[4, 0] = (0.7, 5.0, 1.0, 1.0); psf[4, 1] = (0.0, 0.0, 0.0, 0.0)
    psf[5, 2] = (0.9, 9.0, 9.0, 81.0); psf[5, 0] = (0.0, 1.0, 0.0, 0.0); psf[5, 1] = (0.0, 0.0, 0.0, 0.0)
    return psf


def test_block_psf_columns():
    col = A.block_psf_columns(handmade_psf())
    assert col["block"].tolist() == [0, 0, 1, 1, 2, 2]
    assert col["others"].tolist() == [[1, 2], [1, 2], [0, 2], [0, 2], [0, 1], [0, 1]]
    assert col["rjj"].tolist() == [0.5, 0.25, 0.4, 0.0, 0.0, 0.9]
    assert col["psf_h_km"].tolist() == [3.0, 1.0, 1.0, 0.0, 0.0, 1.0]
    assert col["psf_v_km"].tolist() == [2.0, 0.0, 2.0, 0.0, 0.0, 3.0]
    assert col["colocated"].tolist() == [[0.1, -0.2], [0.0, 0.0], [0.3, 0.0], [0.0, 0.0], [0.7, 0.0], [0.0, 0.0]]
    assert col["share"][0].tolist() == [0.5, 0.125, 0.375] and col["share"][2].tolist() == [0.25, 0.75, 0.0]
    assert col["share"][3].tolist() == [0.0, 0.0, 0.0] and col["share"][4].tolist() == [1.0, 0.0, 0.0]
    assert col["no_data"] == 1
    for bad in (np.zeros((6, 4)), np.zeros((5, 3, 4)), np.zeros((6, 3, 3))):
        with pytest.raises(ValueError):
            A.block_psf_columns(bad)


def test_leakage_metrics():
    lk = A.leakage_metrics(handmade_psf())
    # Vs spikes: shares into (gc, gs) 0.5 and 0; g spikes with energy (2, 4, 5): shares into Vs 0.25, 1, 0.1
    assert lk["spikes_vs"] == 2 and lk["spikes_g"] == 3
    assert lk["vs_to_g_median"] == 0.25 and lk["vs_to_g_worst"] == 0.5
    assert lk["g_to_vs_median"] == 0.25 and lk["g_to_vs_worst"] == 1.0
    none = A.leakage_metrics(np.zeros((6, 3, 4)))
    assert none["spikes_vs"] == 0 and none["vs_to_g_worst"] == 0.0 and none["g_to_vs_median"] == 0.0
    with pytest.raises(ValueError):
        A.leakage_metrics(np.zeros((4, 2, 4)))


def test_checker_metrics():
    c = case()
    n = c["nparpi"]
    M = A.azimuthal_checkerboards(c, (2, 2, 1), 0.04)
    x = np.zeros(3 * n, np.float32)
    x[n:2 * n] = 0.5 * M[1, n:2 * n]                    # half the gc board recovered ...
    x[:n] = 0.02                                        # ... and 0.02 km/s of Vs everywhere
    mt = A.checker_metrics(c, M[1], x, 1)
    assert abs(mt["corr"] - 1.0) < 1e-12 and abs(mt["gain"] - 0.5) < 1e-6 and len(mt["gain_layers"]) == c["nz"] - 1
    assert set(mt["leak"]) == {"vs", "gs"} and abs(mt["leak"]["vs"] - 0.5) < 1e-6 and mt["leak"]["gs"] == 0.0


@pytest.mark.parametrize("text", ["2,2", "2,2,1,0.04,1", "2,0,1", "a,2,1", "2,2,1,0", "2,2,1,-0.1", "2,2,1,nan", "2,2,1,inf", "2.5,2,1"])
def test_parser_refuses(text, capsys):
    with pytest.raises(ValueError):
        A.parse_board(text)
    with pytest.raises(SystemExit) as exc:
        A.main(["nowhere", "--checkerboard", text])
    assert exc.value.code == 2 and "--checkerboard" in capsys.readouterr().err


@pytest.mark.parametrize("flags", [["--weight", "-1"], ["--weight", "nan"], ["--damp", "-0.5"], ["--damp", "inf"], ["--maxiter", "0"]])
def test_preconditions_come_before_the_library(flags, capsys, monkeypatch):
    """a bad value ends in argparse's error (exit 2) without the input directory being read or the library loaded"""
    from dsurftomo_amd import engine
    monkeypatch.setattr(engine, "load_library", lambda *a, **k: pytest.fail("the library was loaded"))
    with pytest.raises(SystemExit) as exc:
        A.main(["nowhere"] + flags)
    assert exc.value.code == 2 and flags[0] in capsys.readouterr().err
    with pytest.raises(ValueError):
        A.run("nowhere", model="MOD", weight=float("nan"))
    with pytest.raises(ValueError):
        A.run("nowhere", model="MOD", checkerboards=[(2, 2, 0, 0.04)])


def test_parser_accepts():
    assert A.parse_board("2,3,1") == (2, 3, 1, 0.04) and A.parse_board("4,4,2,0.02") == (4, 4, 2, 0.02)


def test_resolution_file_round_trip(tmp_path):
    c = case()
    n = c["nparpi"]
    rng = np.random.default_rng(3)
    psf = rng.random((3 * n, 3, 4))
    psf[:, :, 0] -= 0.5
    psf[5] = 0.0                                        # a spike without data
    a, b = tmp_path / "a.dat", tmp_path / "b.dat"
    A.write_azim_resolution(str(a), c, psf)
    rows = A.read_azim_resolution(str(a))
    assert len(rows) == 3 * n and [r["block"] for r in rows] == [j // n for j in range(3 * n)]
    from dsurftomo_amd import io
    io.write_table(str(b), A.AZIM_RESOLUTION_TABLE, rows)
    assert a.read_bytes() == b.read_bytes()
    col = A.block_psf_columns(psf)
    assert [r["rjj"] for r in rows] == col["rjj"].tolist() and [r["share_b"] for r in rows] == [col["share"][j, col["others"][j, 1]] for j in range(3 * n)]
    assert rows[5]["psf_h_km"] == 0.0 and rows[5]["share_a"] == 0.0
    # the cells are the model files' vertices, in their order, block after block
    from dsurftomo_amd.analyses.common import vertices
    want = [(float(lon), float(lat), float(c["depz"][k])) for _, _, k, lon, lat in vertices(c)]
    assert [(r["lon"], r["lat"], r["depth"]) for r in rows] == want * 3


def test_checker_file_round_trip(tmp_path):
    c = case()
    n = c["nparpi"]
    M = A.azimuthal_checkerboards(c, (2, 2, 2))
    x = (0.3 * np.random.default_rng(4).standard_normal(3 * n)).astype(np.float32)
    a, b = tmp_path / "a.dat", tmp_path / "b.dat"
    A.write_azim_checker(str(a), c, M[2], x)
    rows = A.read_azim_checker(str(a))
    from dsurftomo_amd import io
    io.write_table(str(b), A.AZIM_CHECKER_TABLE, rows)
    assert a.read_bytes() == b.read_bytes() and len(rows) == n
    assert np.array_equal(np.array([r["in_gs"] for r in rows], np.float32), M[2, 2 * n:]) and not any(r["in_vs"] or r["in_gc"] for r in rows)
    assert np.array_equal(np.array([[r["out_vs"], r["out_gc"], r["out_gs"]] for r in rows], np.float32).T.ravel(), x)


def test_help_parses_without_a_library():
    env = dict(os.environ, PYTHONPATH=L.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-m", "dsurftomo_amd.anisotropy", "--help"], capture_output=True, text=True, env=env, cwd=L.ROOT)
    assert out.returncode == 0, out.stderr
    assert "--checkerboard NX,NY,NZ[,G]" in out.stdout and "--resolution" in out.stdout and "AzimResolution.dat" in out.stdout
