"""Inputs of the dispersion tests, shared by the device tests (tests/test_gpu_dispersion.py) and the pin of the oracle to the
reference (tests/test_oracle_vs_ref.py: test_dispersion_envelope): the models, the periods and the table of natural sizes.

Data only: this module imports neither the engine nor pytest, so the CPU pin reads the same inputs as the GPU tests.
"""
import numpy as np

F = np.float32


def layer_count(depz, minthk):
    """rmax of make_layer_geom (csrc/host_geometry.h) in its fp32 arithmetic: sum of the sublayers + the half space"""
    depz = np.asarray(depz, F)
    t = depz[1:] - depz[:-1]
    nsub = ((t + F(1.0e-4)) / (t / F(minthk))).astype(np.int64) + 1
    return int(nsub.sum()) + 1


def depths(nz):
    """nz depth nodes with spacings growing from 2 to ~6 km"""
    return np.concatenate([[0.0], np.cumsum(np.round(2.0 + 4.0 * np.arange(nz - 1) / max(nz - 2, 1)))]).astype(F)


def edge_model(nx, ny, nz):
    """vel (nz, ny, nx): columns cycling through six kinds -- a plain gradient, a low-velocity zone, no contrast at all (its Love
    curve has no root at long periods), a half space slower than the layers above (no Rayleigh root at long periods), a very slow
    surface layer, a fast lid over slower rock; each column scaled a little so that no two are alike"""
    base = np.linspace(2.4, 4.6, nz)
    cols = []
    for c in range(nx * ny):
        v = base.copy()
        kind = c % 6
        if kind == 1:
            v[nz // 4:nz // 2 + 1] = 2.0
        elif kind == 2:
            v[:] = 3.5
        elif kind == 3:
            v[-1] = 2.0
        elif kind == 4:
            v[0] = 1.0
        elif kind == 5:
            v[:max(nz // 4, 1)] = 5.0
        cols.append(v * (1.0 + 0.003 * (c // 6)))
    return np.ascontiguousarray(np.array(cols).T.reshape(nz, ny, nx), F)


def smooth_model(nx, ny, nz):
    i = np.arange(nx)[None, None, :]; j = np.arange(ny)[None, :, None]; k = np.arange(nz)[:, None, None]
    v = (2.6 + 1.9 * k / max(nz - 1, 1)) * (1.0 + 0.05 * np.sin(0.7 * i + 0.3 * k) * np.cos(0.5 * j))
    return np.ascontiguousarray(v, F)


EDGE_T = np.array([0.02, 0.5, 2.0, 5.0, 10.0, 20.0, 40.0, 80.0, 150.0, 400.0, 1000.0])

NATURAL = {
    # name: (nx, ny, nz, minthk, model, periods, kernels, iwave, igr, rmax, (LDS, gshift))
    "rmax64": (3, 2, 22, 2.0, edge_model, EDGE_T[[1, 3, 5, 7, 9]], True, 2, 0, 64, (True, 3)),
    "rmax65": (3, 2, 17, 3.0, edge_model, EDGE_T[[1, 3, 5, 7, 9]], True, 1, 0, 65, (False, 0)),
    "curves_34400": (40, 20, 7, 1.0, smooth_model, np.array([3.0, 8.0, 15.0]), True, 1, 1, 13, (True, 0)),
    "curves_3870": (10, 9, 7, 1.0, edge_model, np.array([2.0, 6.0, 20.0, 90.0]), True, 2, 1, 13, (True, 3)),
    "curves_8600": (20, 10, 7, 1.0, smooth_model, np.array([4.0, 12.0]), True, 2, 0, 13, (True, 2)),
    "nz64": (2, 2, 64, 1.0, edge_model, np.array([5.0, 20.0, 60.0, 200.0]), True, 2, 0, 127, (False, 0)),
    "nper60": (4, 3, 7, 1.0, edge_model, np.geomspace(0.3, 900.0, 60), False, 1, 0, 13, (True, 3)),
}
