"""The bootstrap's row scales (dsurftomo_amd.invert.bootstrap_row_scales) and the CLI's checks of --bootstrap.  Host code only:
runs without a GPU."""
import numpy as np
import pytest

from dsurftomo_amd import invert


def test_scales_are_deterministic_per_seed():
    a = invert.bootstrap_row_scales(500, 620, 6, seed=3)
    b = invert.bootstrap_row_scales(500, 620, 6, seed=3)
    c = invert.bootstrap_row_scales(500, 620, 6, seed=4)
    assert a.shape == (6, 620) and a.dtype == np.float32
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert not np.array_equal(a, c)
    assert not np.array_equal(a[0], a[1])                 # realisations differ from each other


def test_scales_are_square_roots_of_draw_counts():
    ndata, m, R = 731, 900, 9
    s = invert.bootstrap_row_scales(ndata, m, R, seed=11)
    sq = s[:, :ndata].astype(np.float64) ** 2
    counts = np.rint(sq)
    assert np.abs(sq - counts).max() < 1e-5 * max(1.0, counts.max())
    assert (counts.sum(axis=1) == ndata).all()             # ndata draws per realisation
    assert (counts == 0).any(axis=1).all()                 # with replacement: some rows are never drawn
    assert np.array_equal(s[:, :ndata], np.sqrt(counts).astype(np.float32))
    assert (s[:, ndata:] == 1.0).all()                     # the regularisation rows keep their weight


def test_scales_match_their_definition():
    ndata, m = 40, 47
    s = invert.bootstrap_row_scales(ndata, m, 3, seed=7)
    rng = np.random.default_rng(7)
    for r in range(3):
        cnt = np.bincount(rng.integers(0, ndata, size=ndata), minlength=ndata)
        assert np.array_equal(s[r, :ndata], np.sqrt(cnt).astype(np.float32))


@pytest.mark.parametrize("argv", [["--bootstrap", "1"], ["--bootstrap", "-3"], ["--bootstrap", "8", "--host-rows"]])
def test_cli_rejects_bad_bootstrap_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), bootstrap=int(argv[1]), host_rows="--host-rows" in argv)
