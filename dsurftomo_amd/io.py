"""Readers for the reference's on-disk inputs: the parameter file (DSurfTomo.in), the measurement
file (`#`-headed source blocks) and the model file (MOD) -- reference main.f90:134-335.

`load(directory)` builds the argument set of a CalSurfG / synthetic call exactly as the reference's
host program does: fp32 colatitude / longitude in radians with pi = 3.1415926535898, period slots
Rc | Rg | Lc | Lg, sources counted per slot in file order, observed times `dist / velocity` with the
reference's `delsph` distance.  The returned dict is what `call_calsurfg` / `call_synthetic` (ctypes
bindings of the drop-in entries) take.  The reference's Taipei example lives under
tests/golden/taipei/ (BASELINE.json configs[0]).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "taipei")


def delsph(flat1, flon1, flat2, flon2):
    """great-circle distance (km) of the reference's delsph.f90 (haversine on colatitude / longitude in
    radians, R = 6371), in fp32 to the rounding of numpy's single-precision functions"""
    f = np.float32
    pi = f(3.1415926535898)
    dlat, dlon = f(flat2 - flat1), f(flon2 - flon1)
    lat1, lat2 = f(pi / f(2) - flat1), f(pi / f(2) - flat2)
    a = f(np.sin(dlat / f(2)) * np.sin(dlat / f(2)) + np.sin(dlon / f(2)) * np.sin(dlon / f(2)) * np.cos(lat1) * np.cos(lat2))
    return f(f(6371.0) * f(2) * np.arctan2(np.sqrt(a), np.sqrt(f(1) - a)))


def _vals(line):
    return line.split("c:")[0].split()


def load(directory=HERE, model="MOD"):
    f = np.float32
    with open(os.path.join(directory, "DSurfTomo.in")) as fh:
        lines = fh.read().splitlines()[3:]
    it = iter(lines)
    datafile = _vals(next(it))[0]
    nx, ny, nz = (int(v) for v in _vals(next(it))[:3])
    goxd, gozd = (f(v) for v in _vals(next(it))[:2])
    dvxd, dvzd = (f(v) for v in _vals(next(it))[:2])
    nsrc = int(_vals(next(it))[0])
    weight0, damp = (f(v) for v in _vals(next(it))[:2])
    minthk = f(_vals(next(it))[0])             # "sablayers"
    minvel, maxvel = (f(v) for v in _vals(next(it))[:2])
    maxiter = int(_vals(next(it))[0])
    spfra = float(_vals(next(it))[0])
    per = []
    for _ in range(4):
        k = int(_vals(next(it))[0])
        per.append(np.array([float(v) for v in next(it).split()[:k]], np.float64) if k > 0 else np.zeros(0))
    ifsyn = int(_vals(next(it))[0])
    noiselevel = f(_vals(next(it))[0])
    nxt = next(it, None)
    threshold0 = f(_vals(nxt)[0]) if nxt is not None and _vals(nxt) else f(0.0)      # main.f90:210
    kRc, kRg, kLc, kLg = (len(p) for p in per)
    kmax = kRc + kRg + kLc + kLg
    nrc = nsrc
    pi = f(3.1415926535898)
    scxf = np.zeros((nsrc, kmax), f, order="F"); sczf = np.zeros((nsrc, kmax), f, order="F")
    rcxf = np.zeros((nrc, nsrc, kmax), f, order="F"); rczf = np.zeros((nrc, nsrc, kmax), f, order="F")
    periods = np.zeros((nsrc, kmax), np.int32, order="F"); wavetype = np.zeros((nsrc, kmax), np.int32, order="F")
    igrt = np.zeros((nsrc, kmax), np.int32, order="F"); nrc1 = np.zeros((nsrc, kmax), np.int32, order="F")
    nsrc1 = np.zeros(kmax, np.int32)
    vel_obs, dist = [], []
    src_lat = src_lon = f(0)
    istep = istep1 = 0
    knum = 0
    knumo = 12345
    with open(os.path.join(directory, datafile)) as fh:
        for line in fh:
            if not line.strip():
                continue
            if line[0] == "#":
                t = line[1:].split()
                lat, lon, period, wavetp, veltp = f(t[0]), f(t[1]), int(t[2]), int(t[3]), int(t[4])
                if wavetp == 2 and veltp == 0: knum = period
                if wavetp == 2 and veltp == 1: knum = kRc + period
                if wavetp == 1 and veltp == 0: knum = kRg + kRc + period
                if wavetp == 1 and veltp == 1: knum = kLc + kRg + kRc + period
                if knum != knumo:
                    istep = 0
                istep += 1
                istep1 = 0
                src_lat = (f(90.0) - lat) * pi / f(180.0)
                src_lon = lon * pi / f(180.0)
                scxf[istep - 1, knum - 1] = src_lat
                sczf[istep - 1, knum - 1] = src_lon
                periods[istep - 1, knum - 1] = period
                wavetype[istep - 1, knum - 1] = wavetp
                igrt[istep - 1, knum - 1] = veltp
                nsrc1[knum - 1] = istep
                knumo = knum
            else:
                t = line.split()
                lat, lon = f(t[0]), f(t[1])
                istep1 += 1
                rlat = (f(90.0) - lat) * pi / f(180.0)
                rlon = lon * pi / f(180.0)
                rcxf[istep1 - 1, istep - 1, knum - 1] = rlat
                rczf[istep1 - 1, istep - 1, knum - 1] = rlon
                nrc1[istep - 1, knum - 1] = istep1
                vel_obs.append(float(t[2]))
                dist.append(delsph(src_lat, src_lon, rlat, rlon))
    with open(os.path.join(directory, model)) as fh:
        tok = fh.read().split()
    if model == "MOD":
        depz = np.array(tok[:nz], f)
        tok = tok[nz:]
    else:
        depz = load(directory, "MOD")["depz"]
    vels = np.asfortranarray(np.array(tok[:nx * ny * nz], f).reshape(nz, ny, nx).transpose(2, 1, 0))   # vsf(i, j, k)
    return dict(nx=nx, ny=ny, nz=nz, nparpi=(nx - 2) * (ny - 2) * (nz - 1), vels=vels, goxd=goxd, gozd=gozd, dvxd=dvxd, dvzd=dvzd,
                kRc=kRc, kRg=kRg, kLc=kLc, kLg=kLg, tRc=per[0], tRg=per[1], tLc=per[2], tLg=per[3], wavetype=wavetype, igrt=igrt,
                periods=periods, depz=depz, minthk=minthk, scxf=scxf, sczf=sczf, rcxf=rcxf, rczf=rczf, nrc1=nrc1, nsrcsurf1=nsrc1,
                kmax=kmax, nsrcsurf=nsrc, nrcf=nrc, ndata=int(nrc1.sum()), spfra=spfra, ifsyn=ifsyn, noiselevel=noiselevel,
                weight0=weight0, damp=damp, minvel=minvel, maxvel=maxvel, maxiter=maxiter, threshold0=threshold0,
                vel_obs=np.array(vel_obs, f), dist=np.array(dist, f), obst=(np.array(dist, f) / np.array(vel_obs, f)).astype(f))


# ---------------------------------------------------------------------------------------------
# ctypes bindings of the drop-in entries (include/dsurftomo_amd.h), every argument by reference

def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _args(c):
    i32 = lambda v: C.byref(C.c_int(int(v)))
    f32 = lambda v: C.byref(C.c_float(float(v)))
    head = [i32(c["nx"]), i32(c["ny"]), i32(c["nz"]), i32(c["nparpi"]), _ptr(c["vels"])]
    tail = [f32(c["goxd"]), f32(c["gozd"]), f32(c["dvxd"]), f32(c["dvzd"]), i32(c["kRc"]), i32(c["kRg"]), i32(c["kLc"]), i32(c["kLg"]),
            _ptr(c["tRc"]), _ptr(c["tRg"]), _ptr(c["tLc"]), _ptr(c["tLg"]), _ptr(c["wavetype"]), _ptr(c["igrt"]), _ptr(c["periods"]),
            _ptr(c["depz"]), f32(c["minthk"]), _ptr(c["scxf"]), _ptr(c["sczf"]), _ptr(c["rcxf"]), _ptr(c["rczf"]), _ptr(c["nrc1"]),
            _ptr(c["nsrcsurf1"]), i32(c["kmax"]), i32(c["nsrcsurf"]), i32(c["nrcf"])]
    return head, tail


def call_calsurfg(c, capacity=None):
    """dsa_calsurfg on a loaded case -> (dsurf, rw, row, col): COO with 1-based rows (data) and columns"""
    from .engine import load_library
    lib = load_library()
    nd = c["ndata"]
    cap = int(capacity if capacity is not None else c.get("spfra", 1.0) * nd * c["nx"] * c["ny"] * c["nz"])
    iw = np.zeros(cap + 1, np.int32)
    rw = np.zeros(cap, np.float32)
    col = np.zeros(cap, np.int32)
    dsurf = np.zeros(nd, np.float32)
    nar = C.c_int(0)
    head, tail = _args(c)
    lib.dsa_dropin_set_capacity(cap)          # the arrays above: the library refuses to write past them (DSA_ERR_CAPACITY)
    rc = lib.dsa_calsurfg(*head, _ptr(iw), _ptr(rw), _ptr(col), _ptr(dsurf), *tail, C.byref(nar))
    if rc != 0:
        raise RuntimeError("dsa_calsurfg: %s" % lib.dsa_dropin_error().decode())
    n = nar.value
    return dsurf, rw[:n].copy(), iw[1:n + 1].copy(), col[:n].copy()


def call_synthetic(c, noiselevel=0.0):
    from .engine import load_library
    lib = load_library()
    obst = np.zeros(c["ndata"], np.float32)
    head, tail = _args(c)
    rc = lib.dsa_synthetic(*head, _ptr(obst), *tail, C.byref(C.c_float(noiselevel)))
    if rc != 0:
        raise RuntimeError("dsa_synthetic: %s" % lib.dsa_dropin_error().decode())
    return obst


def call_forward_models(c, models, dicing=8, ldd=None, lib=None):
    """dsa_forward_models on a loaded case: `models` is a sequence of K Vs models shaped like c["vels"] (nx, ny, nz).  Times only.
    Returns (dsurf (K, ldd) float32 -- row k holds model k's receiver times in the reference's data order, entries from ndata on are
    left 0 --, failures (K,) int64: dispersion curves without a root per model).  dicing 8: dsa_calsurfg's times, 5: dsa_synthetic's."""
    if lib is None:
        from .engine import load_library
        lib = load_library()
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    K = len(models)
    vels = np.zeros((K, nz, ny, nx), np.float32)                 # C order of Fortran vels(nx, ny, nz, K)
    for k, m in enumerate(models):
        m = np.asarray(m, np.float32)
        if m.shape != (nx, ny, nz):
            raise ValueError("model %d has shape %r, expected %r" % (k, m.shape, (nx, ny, nz)))
        vels[k] = m.transpose(2, 1, 0)
    ldd = c["ndata"] if ldd is None else int(ldd)
    dsurf = np.zeros((K, max(ldd, 1)), np.float32)
    fails = np.zeros(max(K, 1), np.int64)
    i32 = lambda v: C.byref(C.c_int(int(v)))
    _, tail = _args(c)
    rc = lib.dsa_forward_models(i32(nx), i32(ny), i32(nz), i32(K), _ptr(vels), _ptr(dsurf), i32(ldd), i32(dicing), _ptr(fails), *tail)
    if rc != 0:
        raise RuntimeError("dsa_forward_models: %s" % lib.dsa_dropin_error().decode())
    return dsurf[:, :ldd], fails[:K]


def call_forward_steps(c, vsf, steps, alpha=None, dicing=8, obst=None, datweight=None, group=None, ngroups=1, want_dsurf=True, want_models=False, lib=None):
    """dsa_forward_steps on a loaded case: K models built on the device from the base model vsf (nx, ny, nz) and the K steps `steps`
    (K, nparpi) -- or, steps = K (an int), from the K solutions the last batch solve left on the drop-in engine --, each scaled by
    float32(alpha[k]) where alpha is given, clipped as dsa_model_update clips with the case's minvel / maxvel, forward-modelled in one
    call and judged on the device.  Returns dict(dsurf (K, ndata) float32 or None, failures (K,) int64, measures (K, ngroups, 2) float64
    {sum (w r)^2, sum r^2} per group of data or None (it needs obst), models (K, nx, ny, nz) float32 or None)."""
    if lib is None:
        from .engine import load_library
        lib = load_library()
    f = np.float32
    nx, ny, nz, nd, n = c["nx"], c["ny"], c["nz"], c["ndata"], c["nparpi"]
    vsf = np.asarray(vsf, f)
    if vsf.shape != (nx, ny, nz):
        raise ValueError("vsf has shape %r, expected %r" % (vsf.shape, (nx, ny, nz)))
    base = np.ascontiguousarray(vsf.transpose(2, 1, 0))                 # C order of Fortran vsf(nx, ny, nz)
    if isinstance(steps, (int, np.integer)):
        K, steps = int(steps), None
    else:
        steps = np.ascontiguousarray(steps, f).reshape(-1, n)
        K = steps.shape[0]
    opt = lambda a, t: None if a is None else np.ascontiguousarray(a, t)
    alpha, obst, datweight, group = opt(alpha, f), opt(obst, f), opt(datweight, f), opt(group, np.int32)
    for name, a, size in (("alpha", alpha, K), ("obst", obst, nd), ("datweight", datweight, nd), ("group", group, nd)):
        if a is not None and a.size != size:
            raise ValueError("%s has %d values, expected %d" % (name, a.size, size))
    ngroups = int(ngroups)
    dsurf = np.zeros((K, max(nd, 1)), f) if want_dsurf else None
    models = np.zeros((K, nz, ny, nx), f) if want_models else None
    measures = np.zeros((K, max(ngroups, 1), 2)) if obst is not None else None
    fails = np.zeros(max(K, 1), np.int64)
    i32 = lambda v: C.byref(C.c_int(int(v)))
    f32 = lambda v: C.byref(C.c_float(float(v)))
    p = lambda a: None if a is None else _ptr(a)
    _, tail = _args(c)
    rc = lib.dsa_forward_steps(i32(nx), i32(ny), i32(nz), i32(K), _ptr(base), p(steps), p(alpha), f32(c["minvel"]), f32(c["maxvel"]), p(models), p(dsurf),
                               i32(nd), i32(dicing), _ptr(fails), p(obst), p(datweight), p(group), i32(ngroups), p(measures), *tail)
    if rc != 0:
        raise RuntimeError("dsa_forward_steps: %s" % lib.dsa_dropin_error().decode())
    return dict(dsurf=None if dsurf is None else dsurf[:, :nd], failures=fails[:K], measures=measures,
                models=None if models is None else models.transpose(0, 3, 2, 1))


_READ = {"int": int, "flag": int, "f64": float, "f32": lambda t: float(np.float32(t))}           # how a column of a table's kind is read back


def column_names(table):
    return tuple(name for name, _, _ in table[1])


def write_table(path, table, rows):
    """one line per dict of rows in the layout `table` = (header, ((name, format, kind), ...)): the columns in order, each in its format,
    joined by blanks; with header, a first line '# name name ...'.  Kind 'flag' is written as 0 / 1."""
    header, columns = table
    with open(path, "w") as fh:
        if header:
            fh.write("# " + " ".join(column_names(table)) + "\n")
        for r in rows:
            fh.write(" ".join(fmt % (int(bool(r[name])) if kind == "flag" else r[name]) for name, fmt, kind in columns) + "\n")


def read_table(path, table):
    """the rows write_table wrote, as a list of dicts: kinds 'int' and 'flag' as int, 'f64' as float, 'f32' as the float32 value the text
    rounds to.  In a file with a header, blank lines and lines that begin with '#' are skipped."""
    header, columns = table
    rows = []
    with open(path) as fh:
        for line in fh:
            t = line.split()
            if header and (not t or t[0].startswith("#")):
                continue
            if len(t) != len(columns):
                raise ValueError("%s: a line of %d columns, not %d" % (path, len(t), len(columns)))
            rows.append({name: _READ[kind](v) for (name, _, kind), v in zip(columns, t)})
    return rows


def _f64_table(*names):
    """the layout of the two nonlinear files: a header, float64 columns with 17 significant digits and a last integer column"""
    return True, tuple((n, "%.17g", "f64") for n in names[:-1]) + ((names[-1], "%d", "int"),)


TRADEOFF_NONLINEAR_TABLE = _f64_table("weight", "damp", "predicted_rms", "weighted_rms", "rms", "disp_failures")
CROSSVAL_NONLINEAR_TABLE = _f64_table("weight", "damp", "heldout_rms", "full_rms", "cv_rms", "disp_failures")
LINE_SEARCH_TABLE = (True, (("iteration", "%4d", "int"), ("alpha", "%.17g", "f64"), ("weighted_rms", "%.17g", "f64"), ("rms", "%.17g", "f64"),
                            ("disp_failures", "%d", "int"), ("chosen", "%d", "flag")))
TRADEOFF_NONLINEAR_COLUMNS = column_names(TRADEOFF_NONLINEAR_TABLE)
CROSSVAL_NONLINEAR_COLUMNS = column_names(CROSSVAL_NONLINEAR_TABLE)
LINE_SEARCH_COLUMNS = column_names(LINE_SEARCH_TABLE)


def write_tradeoff_nonlinear(path, rows):
    """<input>TradeoffNonlinear.dat: one row per member of the trade-off sweep -- weight, damp, the rms of the weighted residual the
    linearised system predicts for the member's update, the rms of the weighted and of the plain residual of the travel times through
    the member's model (rms = sqrt(sum / ndata)), dispersion curves without a root.  rows: dicts with the keys TRADEOFF_NONLINEAR_COLUMNS.
    17 significant digits: read_tradeoff_nonlinear returns the numbers bit for bit."""
    write_table(path, TRADEOFF_NONLINEAR_TABLE, rows)


def read_tradeoff_nonlinear(path):
    """the rows write_tradeoff_nonlinear wrote, as a list of dicts"""
    return read_table(path, TRADEOFF_NONLINEAR_TABLE)


def write_crossval_nonlinear(path, rows):
    """<input>CrossvalNonlinear.dat: one row per (weight, damp) pair of the cross-validation -- weight, damp, the rms of the held-out weighted
    travel-time residuals through the folds' models, the rms of the weighted residual through the full member's model, the linear cv_rms
    for comparison, dispersion curves without a root summed over the pair's members.  rows: dicts with the keys
    CROSSVAL_NONLINEAR_COLUMNS.  17 significant digits: read_crossval_nonlinear returns the numbers bit for bit."""
    write_table(path, CROSSVAL_NONLINEAR_TABLE, rows)


def read_crossval_nonlinear(path):
    """the rows write_crossval_nonlinear wrote, as a list of dicts"""
    return read_table(path, CROSSVAL_NONLINEAR_TABLE)


def write_line_search(path, rows):
    """<input>LineSearch.dat: one row per (iteration, candidate) -- iteration, alpha, rms of the weighted residual (the score), rms of the
    plain residual, dispersion curves without a root, chosen 0/1.  rows: dicts with the keys LINE_SEARCH_COLUMNS.  The floating-point
    columns are written with 17 significant digits, so that read_line_search returns them bit for bit."""
    write_table(path, LINE_SEARCH_TABLE, rows)


def read_line_search(path):
    """the rows write_line_search wrote, as a list of dicts"""
    return read_table(path, LINE_SEARCH_TABLE)


def write_raypaths(path, paths):
    """raypath.out as the reference's (disabled) dump writes it and its scripts/plotpath.py reads it
    (CalSurfG.f90:2276-2283): '# nrp', then nrp lines 'latitude longitude' in degrees.  paths: Engine.ray_paths()."""
    with open(path, "w") as fh:
        for _, pts in paths:
            fh.write(" # %11d\n" % len(pts))
            for lat, lon in pts:
                fh.write("  %14.7f  %14.7f\n" % (lat, lon))
