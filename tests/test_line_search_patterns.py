"""Host-side pieces of the step-length line search (dsurftomo_amd/invert.py): parsing, the candidate models, the selection rule, the
LineSearch.dat file and the refusals.  No GPU: dsa_model_update is a host function of the library."""
import ctypes as C

import numpy as np
import pytest

from dsurftomo_amd import invert
from dsurftomo_amd import io as taipei


@pytest.fixture(scope="module")
def lib():
    from dsurftomo_amd import build
    return invert.bind(C.CDLL(build.build()))


def test_parse_keeps_the_order_and_drops_duplicates():
    assert invert.parse_line_search("0,0.5,1") == [0.0, 0.5, 1.0]
    assert invert.parse_line_search("1, 0.25 ,1,0.25,2") == [1.0, 0.25, 2.0]
    assert invert.parse_line_search("1.5") == [1.5]
    # equal as float32, the precision the update is scaled in
    assert invert.parse_line_search("0.1,0.10000000001") == [0.1]


@pytest.mark.parametrize("text", ["", ",", "-1", "0.5,-0.25", "nan", "1,inf", "x", "1;2"])
def test_parse_rejects(text):
    with pytest.raises(ValueError):
        invert.parse_line_search(text)


def model_update_rule(vsf, dv, minvel, maxvel):
    """numpy restatement of dsa_model_update (reference main.f90:520-535): the update clipped to +-0.5 km/s, added to the inner nodes of
    the layers above the last, the model clipped to [minvel, maxvel]; all in float32"""
    f = np.float32
    nx, ny, nz = vsf.shape
    d = np.clip(np.asarray(dv, f).reshape(nz - 1, ny - 2, nx - 2), f(-0.5), f(0.5))
    out = np.array(vsf, f, copy=True, order="F")
    inner = (out[1:nx - 1, 1:ny - 1, :nz - 1] + d.transpose(2, 1, 0)).astype(f)
    out[1:nx - 1, 1:ny - 1, :nz - 1] = np.clip(inner, f(minvel), f(maxvel))
    return out


def test_candidates_follow_the_update_rule(lib):
    f = np.float32
    nx, ny, nz = 5, 4, 3
    r = np.random.default_rng(5)
    vsf = np.asfortranarray((2.0 + r.random((nx, ny, nz))).astype(f))
    dv = ((r.random((nx - 2) * (ny - 2) * (nz - 1)) - 0.5) * 1.6).astype(f)          # beyond +-0.5: clipped at full length, not at half
    c = dict(nx=nx, ny=ny, nz=nz, minvel=f(2.1), maxvel=f(2.9))
    alphas = [0.0, 0.5, 1.0, 2.0]
    keep_v, keep_d = vsf.copy(order="F"), dv.copy()
    cands = invert.line_search_candidates(lib, c, vsf, dv, alphas)
    assert (vsf == keep_v).all() and (dv == keep_d).all()          # inputs untouched: dsa_model_update works on copies
    assert len(cands) == 4
    for a, m in zip(alphas, cands):
        want = model_update_rule(keep_v, (f(a) * keep_d).astype(f), c["minvel"], c["maxvel"])
        assert m.flags.f_contiguous and m.dtype == f
        assert (m.view(np.uint32) == want.view(np.uint32)).all(), a
    # step 0 still clips the model to [minvel, maxvel]; the steps differ; the boundary nodes and the last layer never move
    assert (cands[0] == np.asfortranarray(keep_v)).sum() < keep_v.size and (cands[1] != cands[2]).any()
    for m in cands:
        assert (m[0] == keep_v[0]).all() and (m[:, -1] == keep_v[:, -1]).all() and (m[:, :, -1] == keep_v[:, :, -1]).all()
    # full length: what the plain run applies
    plain = keep_v.copy(order="F"); d = keep_d.copy()
    assert lib.dsa_model_update(nx, ny, nz, d.ctypes.data_as(C.c_void_p), plain.ctypes.data_as(C.c_void_p), c["minvel"], c["maxvel"]) == 0
    assert (plain.view(np.uint32) == cands[2].view(np.uint32)).all()


def test_scores_are_the_logged_rms():
    f = np.float32
    r = np.random.default_rng(2)
    obst = (20 + 10 * r.random(37)).astype(f)
    dsyn = (obst[None, :] + r.normal(0, 0.5, (3, 37))).astype(f)
    w = (r.random(37) > 0.2).astype(f)
    wr, pr = invert.line_search_scores(obst, dsyn, w)
    for k in range(3):
        res = (obst - dsyn[k]).astype(f)
        cb = res.copy(); cb[w == 0] = 0          # iteration_device's cbst[:dall]
        assert wr[k] == float(f(np.sqrt((cb.astype(np.float64) ** 2).sum()) / np.sqrt(37)))
        assert pr[k] == float(f(np.sqrt((res.astype(np.float64) ** 2).sum()) / np.sqrt(37)))
        assert abs(wr[k] - np.sqrt(((w * res).astype(np.float64) ** 2).sum() / 37)) < 1e-6
    assert (wr <= pr).all()


def test_select_smallest_first_listed_on_ties_and_eligible_only():
    assert invert.line_search_select([3.0, 1.0, 2.0], [0, 0, 0]) == 1
    assert invert.line_search_select([1.0, 1.0, 2.0], [0, 0, 0]) == 0          # tie: first listed
    assert invert.line_search_select([2.0, 1.0, 1.0], [0, 0, 0]) == 1
    assert invert.line_search_select([3.0, 1.0, 2.0], [0, 4, 0]) == 2          # a dispersion failure: not eligible
    assert invert.line_search_select([3.0, 1.0, 2.0], [0, 1, 1]) == 0
    assert invert.line_search_select([float("nan"), 5.0], [0, 0]) == 1
    with pytest.raises(RuntimeError):
        invert.line_search_select([3.0, 1.0], [1, 2])
    with pytest.raises(RuntimeError):
        invert.line_search_select([], [])


def test_line_search_file_round_trips(tmp_path):
    rows = [dict(iteration=1, alpha=0.0, weighted_rms=float(np.float32(1.2345678)), rms=1.5, disp_failures=0, chosen=0),
            dict(iteration=1, alpha=float(np.float32(0.1)), weighted_rms=0.1 + 0.2, rms=1e-30, disp_failures=3, chosen=0),
            dict(iteration=1, alpha=1.0, weighted_rms=1.0 / 3.0, rms=2.0 / 3.0, disp_failures=0, chosen=1),
            dict(iteration=12, alpha=2.5, weighted_rms=7.0, rms=8.0, disp_failures=0, chosen=1)]
    path = tmp_path / "DSurfTomo.inLineSearch.dat"
    taipei.write_line_search(str(path), rows)
    assert taipei.read_line_search(str(path)) == rows
    lines = path.read_text().splitlines()
    assert lines[0].startswith("#") and len(lines) == 5 and all(len(l.split()) == 6 for l in lines[1:])
    taipei.write_line_search(str(path), [])
    assert taipei.read_line_search(str(path)) == []


def test_check_line_search():
    invert.check_line_search(None, True)
    invert.check_line_search([0.0, 1.0], False)
    for bad in ([], [-1.0], [float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError):
            invert.check_line_search(bad, False)
    with pytest.raises(ValueError, match="--host-rows"):
        invert.check_line_search([1.0], True)


@pytest.mark.parametrize("argv", [["--line-search", "1", "--host-rows"], ["--line-search", "-1"], ["--line-search", ""], ["--line-search", "1,nan"]])
def test_cli_refuses_before_the_library(monkeypatch, tmp_path, argv):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(SystemExit) as exc:
        invert.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("kw", [dict(line_search=[1.0], host_rows=True), dict(line_search=[]), dict(line_search=[-0.5])])
def test_run_refuses_before_the_library(monkeypatch, tmp_path, kw):
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(invert, "load_library", refuse)
    with pytest.raises(ValueError):
        invert.run(str(tmp_path), **kw)


def test_forward_takes_several_models(monkeypatch, tmp_path, capsys):
    """--model is repeatable: several models go through one call_forward_models (dicing 5), one residual file per model; one model
    takes the CalSurfG path as before"""
    from dsurftomo_amd import forward
    c = taipei.load()
    calls = []

    def fake_models(case, models, dicing=8, ldd=None, lib=None):
        calls.append(("models", len(models), dicing))
        return np.stack([case["obst"] + np.float32(k) for k in range(len(models))]), np.zeros(len(models), np.int64)

    def fake_calsurfg(case, capacity=None):
        calls.append(("calsurfg",))
        z = np.zeros(0, np.float32)
        return case["obst"].copy(), z, z.astype(np.int32), z.astype(np.int32)

    monkeypatch.setattr(taipei, "call_forward_models", fake_models)
    monkeypatch.setattr(taipei, "call_calsurfg", fake_calsurfg)
    out = str(tmp_path / "fw")
    assert forward.main([taipei.HERE, "--out", out, "--model", "MOD", "--model", "MOD", "--model", "MOD"]) == 0
    assert calls == [("models", 3, 5)]
    for k in (1, 2, 3):
        a = np.loadtxt("%s.m%02d.residual.dat" % (out, k))
        assert a.shape == (c["ndata"], 3) and np.allclose(a[:, 1] - a[:, 2], k - 1, atol=1e-4)
    del calls[:]
    assert forward.main([taipei.HERE, "--out", out]) == 0 and forward.main([taipei.HERE, "--out", out, "--model", "MOD"]) == 0
    assert calls == [("calsurfg",), ("calsurfg",)]
    assert np.loadtxt(out + ".residual.dat").shape == (c["ndata"], 3)
