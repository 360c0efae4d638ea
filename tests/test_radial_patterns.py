"""The host side of the direct radial inversion (dsurftomo_amd/radial.py), no GPU: the new symbols in the header, the
binding (both kinds of handle), the built library and build.HEADERS; the parser's defaults and the refusals before the engine exists; the
plan; the two files' round trips; the NumPy twin of the update rule against dsa_model_update, which is a host function."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _libs as L
from dsurftomo_amd import depth, io, radial

F = np.float32
NEW = ("dsa_kernels_from_dispersion_radial", "dsa_solve_rows_radial", "dsa_iteration_system_radial_device", "dsa_update_radial")
METHODS = ("kernels_from_dispersion_radial", "solve_rows_radial", "solve_rows_radial_device", "iteration_system_radial_device", "update_radial")


@pytest.fixture(scope="module")
def taipei():
    return io.load()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def test_new_symbols_declared_bound_and_exported():
    """the entry points: declared in the public header, argtypes set on load_library's handle and on a bare CDLL through declare_solvers,
    the five Engine methods present, exported by the built library; the placement header is a dependency of the build"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    with open(os.path.join(L.ROOT, "include", "dsurftomo_amd.h")) as fh:
        header = fh.read()
    lib = E.load_library()
    bare = E.declare_solvers(C.CDLL(E.LIB_PATH))
    for name in NEW:
        assert re.search(r"^int %s\(dsa_engine\* e" % name, header, re.M), name
        assert getattr(lib, name).argtypes and getattr(bare, name).argtypes, name
        assert not name.startswith("dsa_lsmr")
    assert len(lib.dsa_iteration_system_radial_device.argtypes) == 17 and len(lib.dsa_update_radial.argtypes) == 8
    for method in METHODS:
        assert callable(getattr(E.Engine, method)), method
    assert "radial_system.h" in build.HEADERS and os.path.exists(os.path.join(L.ROOT, "dsurftomo_amd", "csrc", "radial_system.h"))


def test_parser_defaults():
    a = radial.parser().parse_args(["dir"])
    assert (a.model, a.iterations, a.weight, a.weight_h, a.damp, a.aniso, a.dvmax, a.resolution) == (None, 3, None, None, None, 0.2, 0.5, False)
    a = radial.parser().parse_args(["dir", "--model", "M2", "--iterations", "5", "--weight", "3", "--weight-h", "1.5", "--damp", "0.1", "--aniso", "0.4", "--dvmax", "0.2",
                                    "--resolution"])
    assert (a.model, a.iterations, a.weight, a.weight_h, a.damp, a.aniso, a.dvmax, a.resolution) == ("M2", 5, 3.0, 1.5, 0.1, 0.4, 0.2, True)


@pytest.mark.parametrize("argv", [["--iterations", "0"], ["--weight", "-1"], ["--weight", "nan"], ["--weight-h", "-2"], ["--weight-h", "inf"], ["--damp", "-0.5"],
                                  ["--damp", "inf"], ["--aniso", "-0.1"], ["--aniso", "nan"], ["--dvmax", "0"], ["--dvmax", "nan"]])
def test_cli_refuses_bad_numbers_before_the_library(monkeypatch, tmp_path, argv):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(SystemExit) as exc:
        radial.main([str(tmp_path)] + argv)
    assert exc.value.code == 2


@pytest.mark.parametrize("change,word", [(dict(tLc=np.zeros(0), tLg=np.zeros(0)), "Love"), (dict(tRc=np.zeros(0), tRg=np.zeros(0)), "Rayleigh"), (dict(ifsyn=1), "synthetic")])
def test_run_refuses_the_input_before_the_library(monkeypatch, tmp_path, taipei, change, word):
    import dsurftomo_amd.engine as E

    def refuse(*_):
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(E, "load_library", refuse)
    monkeypatch.setattr(E, "Engine", refuse)
    monkeypatch.setattr(io, "load", lambda *_: dict(taipei, **change))
    with pytest.raises(ValueError) as exc:
        radial.run(str(tmp_path))
    assert word in str(exc.value)


@pytest.mark.parametrize("kw", [dict(iterations=0), dict(weight=-1.0), dict(weight_h=float("nan")), dict(damp=float("inf")), dict(aniso=-0.2), dict(dvmax=0.0)])
def test_run_refuses_before_the_input_is_read(monkeypatch, tmp_path, kw):
    def refuse(*_):
        raise AssertionError("the input was read")
    monkeypatch.setattr(io, "load", refuse)
    with pytest.raises(ValueError):
        radial.run(str(tmp_path), **kw)


def test_plan_is_the_dropins(taipei):
    """phase periods: one unit of mode 3 on the slot's map; group periods: the times (mode 1) on the slot's map and the rays (mode 2) on a
    map of the phase velocity at that period behind the kmax maps; the data in file order; every datum's wave type"""
    c = dict(taipei)
    k = c["kmax"]
    # the Taipei example's periods dealt out over the four wave types, as the driver test does
    t = np.asarray(taipei["tRc"], np.float64)
    kRc, kRg, kLc = 8, 5, 7
    c.update(tRc=t[:kRc], tRg=t[kRc:kRc + kRg], tLc=t[kRc + kRg:kRc + kRg + kLc], tLg=t[kRc + kRg + kLc:], kRc=kRc, kRg=kRg, kLc=kLc, kLg=k - kRc - kRg - kLc)
    u = radial.radial_plan(c)
    kLg = k - kRc - kRg - kLc
    assert u["nmaps"] == k + kRg + kLg and [(w, p.size, f) for w, p, f in u["copies"]] == [(2, kRg, k), (1, kLg, k + kRg)]
    assert u["ndata"] == c["ndata"] == u["wave"].size
    group = lambda s: kRc <= s < kRc + kRg or s >= kRc + kRg + kLc
    nunits = sum(int(c["nsrcsurf1"][s]) * (2 if group(s) else 1) for s in range(k))
    assert u["map_index"].size == nunits == u["mode"].size == u["sen_slot"].size
    q = 0
    for s in range(k):
        for src in range(int(c["nsrcsurf1"][s])):
            if not group(s):
                assert (u["map_index"][q], u["mode"][q], u["sen_slot"][q]) == (s, 3, s)
                q += 1
            else:
                want = k + (s - kRc) if s < kRc + kRg else k + kRg + (s - kRc - kRg - kLc)
                assert (u["map_index"][q], u["mode"][q], u["map_index"][q + 1], u["mode"][q + 1]) == (s, 1, want, 2)
                assert u["sen_slot"][q] == u["sen_slot"][q + 1] == s and u["data_first"][q] == u["data_first"][q + 1]
                q += 2
    first = u["data_first"][u["mode"] != 2]
    assert (first == np.concatenate([[0], np.cumsum(u["nrec"][u["mode"] != 2])[:-1]])).all()
    n_r = int(sum(c["nrc1"][:int(c["nsrcsurf1"][s]), s].sum() for s in range(kRc + kRg)))
    assert (u["wave"][:n_r] == 2).all() and (u["wave"][n_r:] == 1).all() and 0 < n_r < u["ndata"]


def test_radial_file_round_trips(tmp_path, taipei):
    """<input>Radial.dat is depth.write_radial's table: vsv, vsh, Voigt average and xi of every node"""
    c = dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F))
    rng = np.random.default_rng(3)
    vsv = (3.0 + rng.random((3, 5, 6))).astype(F); vsh = (vsv * (1.0 + 0.05 * rng.random((3, 5, 6)))).astype(F)
    path = str(tmp_path / "DSurfTomo.inRadial.dat")
    depth.write_radial(path, c, vsv, vsh)
    rows = depth.read_radial(path)
    assert len(rows) == 90
    assert [r["vsv"] for r in rows] == vsv.ravel().astype(np.float64).tolist() and [r["vsh"] for r in rows] == vsh.ravel().astype(np.float64).tolist()
    voigt, xi = depth.voigt_xi(vsv, vsh)
    assert [r["xi"] for r in rows] == xi.ravel().tolist() and [r["voigt"] for r in rows] == voigt.ravel().tolist()


def test_resolution_file_round_trips(tmp_path, taipei):
    c = dict(taipei, nx=6, ny=5, nz=3, depz=np.array([0.0, 2.0, 5.0], F), nparpi=24)
    rng = np.random.default_rng(5)
    n = 48
    psf = rng.random((n, 2, 4))
    psf[7, :, 1:] = 0.0                                  # an unknown without data: no energy anywhere
    path = str(tmp_path / "DSurfTomo.inRadialResolution.dat")
    radial.write_radial_resolution(path, c, psf)
    rows = radial.read_radial_resolution(path)
    assert len(rows) == n and [r["block"] for r in rows] == [0] * 24 + [1] * 24
    for j in (0, 7, 23, 24, 47):
        own, other = j // 24, 1 - j // 24
        tot = psf[j, :, 1].sum()
        assert rows[j]["rjj"] == psf[j, own, 0] and rows[j]["colocated"] == psf[j, other, 0]
        assert rows[j]["share"] == (psf[j, other, 1] / tot if tot > 0 else 0.0)
        assert rows[j]["psf_h_km"] == (np.sqrt(psf[j, own, 2] / psf[j, own, 1]) if psf[j, own, 1] > 0 else 0.0)
        assert rows[j]["psf_v_km"] == (np.sqrt(psf[j, own, 3] / psf[j, own, 1]) if psf[j, own, 1] > 0 else 0.0)
    assert (rows[0]["lon"], rows[0]["lat"], rows[0]["depth"]) == (rows[24]["lon"], rows[24]["lat"], rows[24]["depth"]) and rows[12]["depth"] == 2.0
    lk = radial.leakage(psf)
    assert lk["spikes_v"] == 23 and lk["spikes_h"] == 24 and 0 < lk["v_to_h_median"] <= lk["v_to_h_worst"] < 1


def test_update_twin_equals_dsa_model_update_on_each_block():
    """dvmax = 0.5: each block of update_radial_twin is dsa_model_update on that model with that block of dv, bit for bit -- steps beyond
    +-0.5, at exactly +-0.5, values driven to both bounds, a NaN; the ring and the bottom depth untouched"""
    from dsurftomo_amd import build
    from dsurftomo_amd import engine as E
    build.build()
    lib = E.declare_solvers(C.CDLL(E.LIB_PATH))
    nx, ny, nz = 6, 5, 4
    maxvp = (nx - 2) * (ny - 2) * (nz - 1)
    rng = np.random.default_rng(11)
    vsv = (2.0 + 2.0 * rng.random((nz, ny, nx))).astype(F); vsh = (vsv * F(1.05)).astype(F)
    dv = (0.4 * rng.standard_normal(2 * maxvp)).astype(F)
    dv[[0, 1, 2, 3, maxvp, maxvp + 1]] = [0.5, -0.5, 0.9, -0.9, 0.50001, np.nan]
    minvel, maxvel = F(2.3), F(3.9)
    got = radial.update_radial_twin(vsv, vsh, dv, 0.5, minvel, maxvel)
    for B, model in enumerate((vsv, vsh)):
        want = np.array(model, F, copy=True); step = dv[B * maxvp:(B + 1) * maxvp].copy()
        assert lib.dsa_model_update(nx, ny, nz, L.ptr(step), L.ptr(want), minvel, maxvel) == 0
        assert (bits(got[B]) == bits(want)).all(), B
        ring = np.ones((ny, nx), bool); ring[1:-1, 1:-1] = False
        assert (bits(got[B][:, ring]) == bits(model[:, ring])).all() and (bits(got[B][-1]) == bits(model[-1])).all()
        inner = got[B][:-1, 1:-1, 1:-1]
        assert (inner[np.isfinite(inner)] >= minvel).all() and (inner[np.isfinite(inner)] <= maxvel).all()
    assert np.isnan(got[1]).sum() == 1 and (got[0] != vsv).any()
    # a smaller dvmax clips where dsa_model_update's 0.5 does not
    small = radial.update_radial_twin(vsv, vsh, dv, 0.1, F(0.0), F(9.0))
    d = small[0][:-1, 1:-1, 1:-1] - vsv[:-1, 1:-1, 1:-1]
    assert np.abs(d).max() <= 0.1 + 1e-6


def test_system_twin_layout():
    """the twin's rows below the data: two Laplacian blocks with their own weights, then the tie rows and their right-hand side"""
    nx, ny, nz, dall = 6, 5, 4, 8
    maxvp = 4 * 3 * 3
    rng = np.random.default_rng(2)
    vsv = (3.0 + rng.random((nz, ny, nx))).astype(F); vsh = (vsv + F(0.1) * rng.random((nz, ny, nx)).astype(F)).astype(F)
    rw = np.array([0.5, -0.25, 2.0], F); row = np.array([1, 3, 8], np.int32); col = np.array([1, maxvp + 2, 2 * maxvp], np.int32)
    res = np.arange(dall, dtype=F) - 3; dw = np.array([1, 1, 0, 1, 1, 1, 1, 1], F)
    S = radial.radial_system(nx, ny, nz, rw, row, col, res, dw, 2.0, 0.5, 0.3, vsv, vsh)
    assert S["m"] == dall + 3 * maxvp and S["n"] == 2 * maxvp and (S["b"][:dall] == res * dw).all() and not S["b"][dall:dall + 2 * maxvp].any()
    assert (S["rw"][:3] == np.array([0.5, 0.0, 2.0], F)).all()
    lap0 = (S["row"] > dall) & (S["row"] <= dall + maxvp); lap1 = (S["row"] > dall + maxvp) & (S["row"] <= dall + 2 * maxvp)
    assert S["col"][lap0].max() <= maxvp < S["col"][lap1].min() and lap0.sum() == lap1.sum() == maxvp + 6 * 2
    assert set(np.abs(S["rw"][lap0]).tolist()) == {4.0, 12.0, 2.0} and set(np.abs(S["rw"][lap1]).tolist()) == {1.0, 3.0, 0.5}
    node = radial.unknown_nodes(nx, ny, nz)
    want = F(0.0) - (F(0.3) * (vsh.ravel()[node] - vsv.ravel()[node]).astype(F)).astype(F)
    assert (bits(S["b"][dall + 2 * maxvp:]) == bits(want)).all() and (S["b"][dall + 2 * maxvp:] < 0).any()
    with pytest.raises(ValueError):
        radial.radial_system(nx, ny, nz, rw, row, np.array([1, 2, 2 * maxvp + 1], np.int32), res, dw, 2.0, 0.5, 0.3, vsv, vsh)
    with pytest.raises(ValueError):
        radial.radial_system(nx, ny, nz, rw, row, col, res, dw, 2.0, 0.5, -0.3, vsv, vsh)
