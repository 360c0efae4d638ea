"""The NumPy twins of the depth inversion's device headers (dsurftomo_amd/depth.py is the driver; DESIGN.md sections 21 to 33 and 35): the column steps,
their resolutions, the Monte-Carlo sampler and its marginals and the inversion of the maps' 2 psi terms restated operation by operation for the tests, the tools and the golden
scripts.  The driver takes a handful of small rules from here (sample_block_scale, sample_box, sample_rhat, sample_sd); callers reach the
twins as depth.<name>, which imports them back.  csrc/column_*.h is the arithmetic the device runs.  Nothing here touches the GPU."""
import math

import numpy as np


# ---- NumPy twins ----

def column_l(M):
    """The regulariser of one column of M unknowns, row by row: for M >= 2 a top row (1, -1) on unknowns 0, 1 and a bottom row (-1, 1) on
    M-2, M-1; for M >= 3 the rows (-1, 2, -1) centred on 1 .. M-2.  M = 1: no rows.  Returns (rows, M) float64."""
    rows = []
    if M >= 2:
        r = np.zeros(M); r[0], r[1] = 1.0, -1.0; rows.append(r)
        r = np.zeros(M); r[M - 2], r[M - 1] = -1.0, 1.0; rows.append(r)
    for l in range(1, M - 1):
        r = np.zeros(M); r[l - 1], r[l], r[l + 1] = -1.0, 2.0, -1.0; rows.append(r)
    return np.array(rows).reshape(len(rows), M)


def column_ltl(M):
    """L^T L of column_l(M), (M, M) integers"""
    L = column_l(M)
    return np.rint(L.T @ L).astype(np.int64)


def _twin_normal(G, used, rho, lam2, mu2):
    """N = G^T G + lam2 L^T L + mu2 I and b = G^T rho, the sums over the used k ascending from 0.0 (column_system.h: column_assemble)"""
    K, M = G.shape
    N = np.zeros((M, M)); b = np.zeros(M)
    for k in np.flatnonzero(used):
        N = N + np.outer(G[k], G[k])
        b = b + G[k] * rho[k]
    N = N + lam2 * column_ltl(M).astype(np.float64)
    N[np.diag_indices(M)] = N[np.diag_indices(M)] + mu2
    return N, b


def _twin_factor(N):
    """N = L D L^T without a square root, column by column, every sum subtracted term by term with p ascending (column_factor).  Returns
    (L (M, M) strictly lower, d (M)), or None at a pivot that is not finite or <= 0."""
    M = N.shape[0]
    Lm = np.zeros((M, M)); d = np.zeros(M)
    for j in range(M):
        v = Lm[j, :j] * d[:j]
        col = N[j:, j].copy()                                          # (entry 0: the pivot; the others: column j below it)
        for p in range(j):
            col = col - Lm[j:, p] * v[p]
        if not (np.isfinite(col[0]) and col[0] > 0):
            return None
        d[j] = col[0]
        Lm[j + 1:, j] = col[1:] / d[j]
    return Lm, d


def _twin_solve(Lm, d, b):
    """L D L^T x = b (column_solve): forward with p ascending, the division by d, back with i descending and p ascending.  b: (M) or (M, n),
    one right-hand side per column."""
    M = len(d)
    b = np.asarray(b, np.float64)
    x = b.reshape(M, -1).copy()
    for p in range(M - 1):
        x[p + 1:] = x[p + 1:] - Lm[p + 1:, p, None] * x[p]
    x = x / d[:, None]
    for i in range(M - 2, -1, -1):
        s = x[i].copy()
        for p in range(i + 1, M):
            s = s - Lm[p, i] * x[p]
        x[i] = s
    return x.reshape(b.shape)


def _twin_data(obs, wt, pv, S, love=None):
    """The data of one column, as every twin reads them: obs, wt (K) fp32, pv (K) fp64, S (K, M) fp64.  Returns (used, rho (K), chi2, G (K, M)):
    a datum is used where its weight, its observation and its curve are positive; rho = a (obs - pv), 0 where unused; chi2 the sum of rho^2
    over the used k ascending from 0.0 -- two sums [Rayleigh, Love] by love (K) bool where one is given; G = diag(a) S on the used rows (the
    S of an unused datum is never read: it may not be finite)."""
    used = (wt > 0) & (obs > 0) & (pv > 0)
    a = wt.astype(np.float64)
    rho = np.where(used, a * (obs.astype(np.float64) - pv), 0.0)
    chi2 = [0.0, 0.0]
    for k in np.flatnonzero(used):
        q = 0 if love is None else int(love[k])
        chi2[q] = chi2[q] + rho[k] * rho[k]
    G = np.zeros(S.shape)
    G[used] = a[used, None] * S[used]
    return used, rho, chi2[0] if love is None else chi2, G


def _twin_radial_normal(G, used, love, rho, lam2, mu2, gam2, d):
    """column_radial.h's radial_assemble: the 2M x 2M matrix of the unknowns [dVsv ; dVsh] -- _twin_normal of the Rayleigh and of the Love data
    on the diagonal, each with gam2 added to its diagonal, -gam2 I beside them -- and b = [b_v + gam2 d ; b_h - gam2 d], d = vsh - vsv (M)"""
    M = G.shape[1]
    N = np.zeros((2 * M, 2 * M)); b = np.zeros(2 * M)
    for q, sel in enumerate((used & ~love, used & love)):
        Nq, bq = _twin_normal(G, sel, rho, lam2, mu2)
        Nq[np.diag_indices(M)] = Nq[np.diag_indices(M)] + gam2
        N[q * M:(q + 1) * M, q * M:(q + 1) * M] = Nq
        t = gam2 * d
        b[q * M:(q + 1) * M] = bq - t if q else bq + t
    N[M:, :M][np.diag_indices(M)] = 0.0 - gam2
    N[:M, M:] = N[M:, :M].T
    return N, b


def _twin_clip(delta, dvmax):
    """column_clip: the step in fp32, clipped to +- dvmax (a NaN stays)"""
    s = np.asarray(delta).astype(np.float32)
    dvmax = np.float32(dvmax)
    with np.errstate(invalid="ignore"):
        s = np.where(s >= dvmax, dvmax, s)
        return np.where(s <= -dvmax, -dvmax, s).astype(np.float32)


def _twin_stepped(vel, s, minvel, maxvel):
    """column_stepped: vel + s in fp32, clipped to [minvel, maxvel]"""
    with np.errstate(invalid="ignore"):
        v = (vel + s).astype(np.float32)
        v = np.where(v < np.float32(minvel), np.float32(minvel), v)
        return np.where(v > np.float32(maxvel), np.float32(maxvel), v)


def column_step_twin(obs, wt, pv, S, vels, smooth, damp, dvmax, minvel, maxvel, solver="ldlt", n_override=None):
    """dsa_columns_step on one column in NumPy.  obs (K) fp32, wt (K) fp32 or None, pv (K) fp64, S (K, M) fp64 (k_sen_combine's d c / d Vs),
    vels (M or more) fp32: the column's values from the top; only the first M are stepped.  The sums run in column_system.h's order (k
    ascending from 0.0; the factorisation and the substitutions subtract term by term), so solver 'ldlt' follows the device operation by
    operation.  solver 'lstsq': the same step from numpy.linalg.lstsq on the stacked system [diag(a) S; smooth L; damp I] -- another
    algorithm, for the size of the rounding error.  n_override: an (M, M) matrix to factorise in place of the assembled N (tests).
    Returns dict(delta (M) fp64, dv (M) fp32, vels (the stepped copy), nused, chi2, flag)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    vels = np.array(vels, f, copy=True)
    used, rho, chi2, G = _twin_data(obs, wt, pv, S)
    out = dict(delta=np.zeros(M), dv=np.zeros(M, f), vels=vels, nused=int(used.sum()), chi2=float(chi2), flag=0)
    if out["nused"] == 0:
        out["flag"] = 2
        return out
    lam2, mu2 = float(f(smooth)) * float(f(smooth)), float(f(damp)) * float(f(damp))
    if solver == "lstsq":
        A = np.vstack([G[used], float(f(smooth)) * column_l(M), float(f(damp)) * np.eye(M)])
        rhs = np.concatenate([rho[used], np.zeros(A.shape[0] - int(used.sum()))])
        delta = np.linalg.lstsq(A, rhs, rcond=None)[0]
    else:
        N, b = _twin_normal(G, used, rho, lam2, mu2)
        if n_override is not None:
            N = np.array(n_override, np.float64)
        factor = _twin_factor(N)
        if factor is None:
            out["flag"] = 1
            return out
        delta = _twin_solve(*factor, b)
    s = _twin_clip(delta, dvmax)
    vels[:M] = _twin_stepped(vels[:M], s, minvel, maxvel)
    out.update(delta=delta, dv=s)
    return out


def column_radial_twin(obs, wt, pv, S, love, vsv, vsh, smooth, damp, aniso, dvmax, minvel, maxvel, solver="ldlt", n_override=None):
    """dsa_columns_step_radial on one column in NumPy (csrc/column_radial.h).  obs, wt, pv as column_step_twin's; S (K, M): row k the
    sensitivities of datum k to the model its slot was run on (Vsh where love[k], else Vsv); love (K) bool; vsv, vsh (M or more) fp32, of
    which the first M are stepped.  The unknowns are [dVsv ; dVsh].  solver 'ldlt' follows the header operation by operation through
    _twin_factor / _twin_solve on the 2M x 2M matrix; solver 'lstsq': the same step from numpy.linalg.lstsq on the stacked system
    [G; smooth L (+) smooth L; damp I; aniso [-I I]] with right-hand side [rho; 0; 0; -aniso d], d = vsh - vsv -- another algorithm, for the
    size of the rounding error.  n_override: a (2M, 2M) matrix in place of the assembled N (tests).  Returns dict(delta (2M) fp64, dv_sv,
    dv_sh (M) fp32, vsv, vsh (the stepped copies), nused (2) and chi2 (2): Rayleigh, Love; flag)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64); love = np.asarray(love, bool)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    vsv = np.array(vsv, f, copy=True); vsh = np.array(vsh, f, copy=True)
    used, rho, chi2, G = _twin_data(obs, wt, pv, S, love)
    out = dict(delta=np.zeros(2 * M), dv_sv=np.zeros(M, f), dv_sh=np.zeros(M, f), vsv=vsv, vsh=vsh, nused=[int((used & ~love).sum()), int((used & love).sum())],
               chi2=[float(chi2[0]), float(chi2[1])], flag=0)
    if not used.any():
        out["flag"] = 2
        return out
    lam, mu, gam = float(f(smooth)), float(f(damp)), float(f(aniso))
    d = vsh[:M].astype(np.float64) - vsv[:M].astype(np.float64)
    if solver == "lstsq":
        nu = int(used.sum())
        A = np.zeros((nu, 2 * M))
        A[:, :M] = np.where(love[used, None], 0.0, G[used]); A[:, M:] = np.where(love[used, None], G[used], 0.0)
        Lm = column_l(M); Z = np.zeros_like(Lm)
        A = np.vstack([A, lam * np.hstack([Lm, Z]), lam * np.hstack([Z, Lm]), mu * np.eye(2 * M), gam * np.hstack([-np.eye(M), np.eye(M)])])
        rhs = np.concatenate([rho[used], np.zeros(2 * Lm.shape[0] + 2 * M), -gam * d])
        delta = np.linalg.lstsq(A, rhs, rcond=None)[0]
    else:
        N, b = _twin_radial_normal(G, used, love, rho, lam * lam, mu * mu, gam * gam, d)
        if n_override is not None:
            N = np.array(n_override, np.float64)
        factor = _twin_factor(N)
        if factor is None:
            out["flag"] = 1
            return out
        delta = _twin_solve(*factor, b)
    s = _twin_clip(delta, dvmax)
    vsv[:M] = _twin_stepped(vsv[:M], s[:M], minvel, maxvel)
    vsh[:M] = _twin_stepped(vsh[:M], s[M:], minvel, maxvel)
    out.update(delta=delta, dv_sv=s[:M].copy(), dv_sh=s[M:].copy())
    return out


def lateral_sum(part):
    """the global sum of csrc/column_lateral.h: 64 chains -- chain t adds part[t], part[t + 64], ... from 0.0 -- added with t ascending"""
    total = 0.0
    for t in range(64):
        c = 0.0
        for v in part[t::64]:
            c = c + float(v)
        total = total + c
    return total


def _twin_pcg(col, interior, bt, apply, coupled, tol, maxit):
    """column_lateral.h's preconditioned conjugate gradients in its order.  col: {column: dict with "factor"} of the active columns; interior:
    all interior columns in their order (the dots' figures lie in it, 0.0 where not active, then lateral_sum); bt: {column: right-hand
    side}; apply(y) -> {column: (A y)_c}; coupled: False stops at iteration 0 whatever rz is.  Returns (x, itn, istop, rz0, rz)."""
    solve = lambda r: {c: _twin_solve(*col[c]["factor"], r[c]) for c in col}
    dot = lambda u, w: lateral_sum([_chain_dot(u[c], w[c]) if c in col else 0.0 for c in interior])
    x = solve(bt)
    rz0 = dot(bt, x)
    thr = (float(tol) * float(tol)) * rz0
    q = apply(x)
    r = {c: bt[c] - q[c] for c in col}
    z = solve(r)
    rz = dot(r, z)
    itn, istop = 0, 0
    if not coupled or rz <= thr:
        istop = 1
    p_old = {c: np.zeros(len(bt[c])) for c in col}
    beta = 0.0
    while not istop:
        p = {c: z[c] + beta * p_old[c] for c in col}
        q = apply(p)
        alpha = rz / dot(p, q)
        x = {c: x[c] + alpha * p[c] for c in col}
        r = {c: r[c] - alpha * q[c] for c in col}
        z = solve(r)
        new = dot(r, z)
        beta = new / rz
        rz = new
        p_old = p
        itn += 1
        if rz <= thr:
            istop = 1
        elif itn >= maxit:
            istop = 2
    return x, itn, istop, float(rz0), float(rz)


def _twin_stacked(col, edges, B, own, between, matrix=False):
    """The other answer of a coupled twin: numpy.linalg.lstsq on the stacked system of the active columns col, B unknowns each.  own(c) ->
    [(block (rows, B), right-hand side)] of column c alone; between(c, n) -> [(block (rows, B), right-hand side)] of the edge c < n, the
    block applied to c and, negated, to n.  Returns {column: solution (B)} -- or, with matrix, (the stacked matrix, {column: its first
    unknown's place}) and solves nothing."""
    index = {c: q * B for q, c in enumerate(col)}
    rows, rhs = [], []

    def put(parts, right):
        full = np.zeros((len(right), len(col) * B))
        for c, block in parts:
            full[:, index[c]:index[c] + B] = block
        rows.append(full); rhs.append(right)

    for c in col:
        for block, right in own(c):
            put([(c, block)], right)
    for c in col:
        for n in edges[c]:
            if n > c:
                for block, right in between(c, n):
                    put([(c, block), (n, -block)], right)
    if matrix:
        return np.vstack(rows), index
    sol = np.linalg.lstsq(np.vstack(rows), np.concatenate(rhs), rcond=None)[0]
    return {c: sol[index[c]:index[c] + B] for c in col}


def column_lateral_twin(nx, ny, obs, wt, pv, S, vels, smooth, damp, lateral, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
    """dsa_columns_step_lateral in NumPy (csrc/column_lateral.h) on an (ny, nx) grid of columns, the outer ring included as the engine holds
    it: obs, wt (K, ny * nx) fp32 (wt may be None), pv (K, ny * nx), S (M, K, ny * nx), vels (M or more, ny * nx) fp32, of which the first M
    rows of the interior columns are stepped.  Two answers: delta, the preconditioned conjugate gradients in the header's order (the
    columns' N, b and factors through _twin_normal / _twin_factor / _twin_solve, every dot product per column and then lateral_sum), and,
    independently of that, delta_lstsq from numpy.linalg.lstsq on the stacked [blockdiag(G_c); smooth L; damp I; lateral E] of the active
    columns with right-hand side [rho; 0; 0; -lateral E v], E the edge differences -- another algorithm, for the size of the rounding error.
    Returns dict(delta, delta_lstsq (M, ny * nx) fp64, dv (M,
    ny * nx) fp32 and vels (the stepped copy) from delta, nused, chi2, flag (ny * nx), deg (ny * nx), itn, istop, rz0, rz)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    M, K, ncol = S.shape
    assert ncol == nx * ny and obs.shape == (K, ncol)
    wt = np.ones((K, ncol), f) if wt is None else np.asarray(wt, f)
    vels = np.array(vels, f, copy=True)
    lam, mu, lat = float(f(smooth)), float(f(damp)), float(f(lateral))
    lam2, mu2, lat2 = lam * lam, mu * mu, lat * lat
    out = dict(delta=np.zeros((M, ncol)), delta_lstsq=np.zeros((M, ncol)), dv=np.zeros((M, ncol), f), vels=vels, nused=np.zeros(ncol, np.int32), chi2=np.zeros(ncol),
               flag=np.zeros(ncol, np.int32), deg=np.zeros(ncol, np.int32), itn=0, istop=0, rz0=0.0, rz=0.0)
    interior = [j * nx + i for j in range(1, ny - 1) for i in range(1, nx - 1)]
    col = {}                                                            # the active columns: G, used, rho, N, factor, b
    for c in interior:
        used, rho, chi2, G = _twin_data(obs[:, c], wt[:, c], pv[:, c], S[:, :, c].T)
        out["nused"][c] = int(used.sum()); out["chi2"][c] = chi2
        if not used.any() and lat == 0.0:
            out["flag"][c] = 2
            continue
        N, b = _twin_normal(G, used, rho, lam2, mu2)
        factor = _twin_factor(N)
        if factor is None:
            out["flag"][c] = 1
            continue
        col[c] = dict(G=G, used=used, rho=rho, N=N, factor=factor, b=b)
    edges = {c: [n for n in (c - 1, c + 1, c - nx, c + nx) if n in col] if lat > 0.0 else [] for c in col}
    for c in col:
        out["deg"][c] = len(edges[c])
    v64 = vels[:M].astype(np.float64)

    def apply(y):
        q = {}
        for c, d in col.items():
            t = np.zeros(M)
            for j in range(M):
                t = t + d["N"][:, j] * y[c][j]
            s = np.zeros(M)
            for n in edges[c]:
                s = s + y[n]
            q[c] = t + lat2 * (float(len(edges[c])) * y[c] - s)
        return q

    bt = {}
    for c, d in col.items():
        s = np.zeros(M)
        for n in edges[c]:
            s = s + (v64[:, c] - v64[:, n])
        bt[c] = d["b"] - lat2 * s if lat > 0.0 else d["b"].copy()
    x, out["itn"], out["istop"], out["rz0"], out["rz"] = _twin_pcg(col, interior, bt, apply, lat > 0.0, tol, maxit)
    if col:
        Lm = column_l(M)
        own = lambda c: [(col[c]["G"][col[c]["used"]], col[c]["rho"][col[c]["used"]]), (lam * Lm, np.zeros(Lm.shape[0])), (mu * np.eye(M), np.zeros(M))]
        other = _twin_stacked(col, edges, M, own, lambda c, n: [(lat * np.eye(M), -lat * (v64[:, c] - v64[:, n]))])
    for c in col:
        out["delta"][:, c] = x[c]
        out["delta_lstsq"][:, c] = other[c]
    out["dv"] = _twin_clip(out["delta"], dvmax)
    for c in col:
        vels[:M, c] = _twin_stepped(vels[:M, c], out["dv"][:, c], minvel, maxvel)
    return out


def column_lateral_resolution_twin(nx, ny, obs, wt, pv, S, depz, smooth, damp, lateral, kind, index, models=None, tol=1e-8, maxit=500):
    """dsa_columns_resolution_lateral in NumPy (csrc/column_lateral_resolution.h) on an (ny, nx) grid of columns as column_lateral_twin takes
    it; depz: the depths of the unknowns (M or more, fp32); kind, index (nmembers); models None or (rows, M, interior columns).  Two answers.
    The header's: N_c, H_c = G_c^T G_c and the factors through _twin_normal / _twin_factor, every member's right-hand side by the header's
    chain, its solve by _twin_pcg, its measures per column with l ascending and then lateral_sum.  And, independently, a dense one: with B
    the stacked [blockdiag(G_c); smooth L; damp I; lateral E] of the active columns as _twin_stacked builds it and P = numpy.linalg.pinv(B),
    A^-1 = P P^T; x = P [G m; 0] for kinds 0 and 2, x = P (P^T f) for kinds 1 and 3, the measures by plain NumPy sums.  Returns dict(measures
    (nmembers, 7): val, m1, mz, mx, my, own, var; full (nmembers, M, interior columns): u; itn, istop (nmembers) int32; rz0, rz (nmembers);
    measures_dense, full_dense; nused, flag (ny * nx); data_response(rw): A^-1 G^T rw (M, interior columns) of weighted residuals rw (K,
    ny * nx), dense)."""
    f32 = np.float32
    obs = np.asarray(obs, f32); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    M, K, ncol = S.shape
    assert ncol == nx * ny and obs.shape == (K, ncol)
    wt = np.ones((K, ncol), f32) if wt is None else np.asarray(wt, f32)
    kind = np.asarray(kind, np.int64).ravel(); index = np.asarray(index, np.int64).ravel()
    lam, mu, lat = float(f32(smooth)), float(f32(damp)), float(f32(lateral))
    lat2 = lat * lat
    z = np.asarray(depz, f32)[:M].astype(np.float64)
    nvx = nx - 2
    interior = [j * nx + i for j in range(1, ny - 1) for i in range(1, nx - 1)]
    nint, nm = len(interior), len(kind)
    out = dict(measures=np.zeros((nm, 7)), full=np.zeros((nm, M, nint)), itn=np.zeros(nm, np.int32), istop=np.zeros(nm, np.int32), rz0=np.zeros(nm), rz=np.zeros(nm),
               measures_dense=np.zeros((nm, 7)), full_dense=np.zeros((nm, M, nint)), nused=np.zeros(ncol, np.int32), flag=np.zeros(ncol, np.int32))
    col = {}
    for c in interior:
        used, rho, _, G = _twin_data(obs[:, c], wt[:, c], pv[:, c], S[:, :, c].T)
        out["nused"][c] = int(used.sum())
        if not used.any() and lat == 0.0:
            out["flag"][c] = 2
            continue
        N, _ = _twin_normal(G, used, rho, lam * lam, mu * mu)
        factor = _twin_factor(N)
        if factor is None:
            out["flag"][c] = 1
            continue
        col[c] = dict(G=G, used=used, N=N, factor=factor, H=_twin_normal(G, used, rho, 0.0, 0.0)[0])
    edges = {c: [n for n in (c - 1, c + 1, c - nx, c + nx) if n in col] if lat > 0.0 else [] for c in col}

    def apply(y):
        q = {}
        for c, d in col.items():
            t = np.zeros(M)
            for j in range(M):
                t = t + d["N"][:, j] * y[c][j]
            s = np.zeros(M)
            for n in edges[c]:
                s = s + y[n]
            q[c] = t + lat2 * (float(len(edges[c])) * y[c] - s)
        return q

    def gram(c, m):
        t = np.zeros(M)
        for j in range(M):
            t = t + col[c]["H"][:, j] * m[j]
        return t

    def rhs(k, idx):
        f = {c: np.zeros(M) for c in col}
        for b, c in enumerate(interior):
            if c not in col:
                continue
            if k == 0 and idx // M == b:
                f[c] = gram(c, np.eye(M)[idx % M])
            elif k == 1 and idx // M == b:
                f[c] = np.eye(M)[idx % M].copy()
            elif k == 2:
                f[c] = gram(c, models[idx][:, b])
            elif k == 3:
                f[c] = np.array(models[idx][:, b], np.float64)
        return f

    def measure(k, idx, x, u):
        """x, u (M, nint); the figures per column with l ascending, then lateral_sum; plain: NumPy's sums"""
        b0, l0 = idx // M, idx % M
        dz = z - z[l0]
        di = np.array([(b % nvx) - (b0 % nvx) for b in range(nint)], np.float64); dj = np.array([(b // nvx) - (b0 // nvx) for b in range(nint)], np.float64)
        fig = np.zeros((5, nint))
        for l in range(M):
            r2 = u[l] * u[l]
            fig[0] = fig[0] + r2
            fig[1] = fig[1] + r2 * (dz[l] * dz[l])
            fig[2] = fig[2] + r2 * (di * di)
            fig[3] = fig[3] + r2 * (dj * dj)
            if k == 1:
                fig[4] = fig[4] + x[l] * u[l]
        return [u[l0, b0]] + [lateral_sum(fig[q]) for q in range(4)] + [fig[0, b0], lateral_sum(fig[4])]

    if col:
        Lm = column_l(M)
        own = lambda c: [(col[c]["G"][col[c]["used"]], np.zeros(int(col[c]["used"].sum()))), (lam * Lm, np.zeros(Lm.shape[0])), (mu * np.eye(M), np.zeros(M))]
        Bm, place = _twin_stacked(col, edges, M, own, lambda c, n: [(lat * np.eye(M), np.zeros(M))], matrix=True)
        P = np.linalg.pinv(Bm)
        data_rows = {}                                                  # the rows of B that hold column c's used data
        at = 0
        for c in col:
            nu = int(col[c]["used"].sum())
            data_rows[c] = np.arange(at, at + nu)
            at += nu + Lm.shape[0] + M
    pos = {c: b for b, c in enumerate(interior)}

    def spread(sol):
        full = np.zeros((M, nint))
        for c in col:
            full[:, pos[c]] = sol[place[c]:place[c] + M]
        return full

    def data_response(rw):
        if not col:
            return np.zeros((M, nint))
        right = np.zeros(Bm.shape[0])
        for c in col:
            right[data_rows[c]] = np.asarray(rw, np.float64)[col[c]["used"], c]
        return spread(P @ right)

    out["data_response"] = data_response
    for s in range(nm):
        k, idx = int(kind[s]), int(index[s])
        f = rhs(k, idx)
        x, out["itn"][s], out["istop"][s], out["rz0"][s], out["rz"][s] = _twin_pcg(col, interior, f, apply, lat > 0.0, tol, maxit)
        xf = np.zeros((M, nint)); uf = np.zeros((M, nint))
        for c in col:
            xf[:, pos[c]] = x[c]
            uf[:, pos[c]] = gram(c, x[c]) if k == 1 else x[c]
        out["full"][s] = uf
        if k < 2:
            out["measures"][s] = measure(k, idx, xf, uf)
        if not col:
            continue
        if k in (0, 2):
            m = np.zeros((M, nint))
            if k == 0:
                m[idx % M, idx // M] = 1.0
            else:
                m = np.asarray(models[idx], np.float64)
            right = np.zeros(Bm.shape[0])
            for c in col:
                right[data_rows[c]] = col[c]["G"][col[c]["used"]] @ m[:, pos[c]]
            xd = spread(P @ right)
        else:
            fv = np.zeros(Bm.shape[1])
            for c in col:
                fv[place[c]:place[c] + M] = f[c]
            xd = spread(P @ (P.T @ fv))
        ud = xd
        if k == 1:
            ud = np.zeros((M, nint))
            for c in col:
                Gu = col[c]["G"][col[c]["used"]]
                ud[:, pos[c]] = Gu.T @ (Gu @ xd[:, pos[c]])
        out["full_dense"][s] = ud
        if k < 2:
            b0, l0 = idx // M, idx % M
            r2 = ud * ud
            dz = (z - z[l0])[:, None]
            di = np.array([(b % nvx) - (b0 % nvx) for b in range(nint)], np.float64)[None, :]; dj = np.array([(b // nvx) - (b0 // nvx) for b in range(nint)], np.float64)[None, :]
            out["measures_dense"][s] = [ud[l0, b0], r2.sum(), (r2 * dz * dz).sum(), (r2 * di * di).sum(), (r2 * dj * dj).sum(), r2[:, b0].sum(),
                                        float((xd * ud).sum()) if k == 1 else 0.0]
    return out


def column_radial_lateral_twin(nx, ny, obs, wt, pv, S, love, vsv, vsh, smooth, damp, aniso, lateral, lateral_aniso, dvmax, minvel, maxvel, tol=1e-8, maxit=500):
    """dsa_columns_step_radial_lateral in NumPy (csrc/column_radial_lateral.h) on an (ny, nx) grid of columns, the outer ring included as the
    engine holds it: obs, wt (K, ny * nx) fp32 (wt may be None), pv (K, ny * nx), S (M, K, ny * nx) -- slot k's sensitivities to the model it
    was run on, Vsh where love[k], else Vsv, as column_radial_twin's -- love (K) bool, vsv, vsh (M or more, ny * nx) fp32, of which the first M
    rows of the interior columns are stepped.  The unknowns of a column are [dVsv ; dVsh].  Two answers: delta, the preconditioned conjugate
    gradients in the header's order (the columns' N and b as column_radial_twin's, the factors through _twin_factor / _twin_solve, every dot
    product per column and then lateral_sum), and, independently of that, delta_lstsq from numpy.linalg.lstsq on the stacked
    [blockdiag(G_c); smooth L (+) smooth L; damp I; aniso [-I I]; lateral E_v; lateral E_h; lateral_aniso E_a] of the active columns with
    right-hand side [rho; 0; 0; -aniso d; -lateral E vsv; -lateral E vsh; -lateral_aniso E (vsh - vsv)], E the edge differences -- another
    algorithm, for the size of the rounding error.  Returns dict(delta, delta_lstsq (2M, ny * nx) fp64, dv (2, M, ny * nx) fp32, vsv, vsh (the
    stepped copies) from delta, nused, chi2 (2, ny * nx): Rayleigh, Love; flag, deg (ny * nx), itn, istop, rz0, rz)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64); love = np.asarray(love, bool)
    M, K, ncol = S.shape
    B = 2 * M
    assert ncol == nx * ny and obs.shape == (K, ncol) and love.shape == (K,)
    wt = np.ones((K, ncol), f) if wt is None else np.asarray(wt, f)
    vsv = np.array(vsv, f, copy=True); vsh = np.array(vsh, f, copy=True)
    lam, mu, gam, lat, lata = float(f(smooth)), float(f(damp)), float(f(aniso)), float(f(lateral)), float(f(lateral_aniso))
    w2, wa2 = lat * lat, lata * lata
    with_edges = lat > 0.0 or lata > 0.0
    out = dict(delta=np.zeros((B, ncol)), delta_lstsq=np.zeros((B, ncol)), dv=np.zeros((2, M, ncol), f), vsv=vsv, vsh=vsh, nused=np.zeros((2, ncol), np.int32),
               chi2=np.zeros((2, ncol)), flag=np.zeros(ncol, np.int32), deg=np.zeros(ncol, np.int32), itn=0, istop=0, rz0=0.0, rz=0.0)
    interior = [j * nx + i for j in range(1, ny - 1) for i in range(1, nx - 1)]
    v64 = vsv[:M].astype(np.float64); h64 = vsh[:M].astype(np.float64)
    a64 = h64 - v64
    col = {}                                                            # the active columns: G, used, rho, N, factor, b
    for c in interior:
        used, rho, chi2, G = _twin_data(obs[:, c], wt[:, c], pv[:, c], S[:, :, c].T, love)
        out["nused"][:, c] = [int((used & ~love).sum()), int((used & love).sum())]; out["chi2"][:, c] = chi2
        if not used.any() and not with_edges:
            out["flag"][c] = 2
            continue
        N, b = _twin_radial_normal(G, used, love, rho, lam * lam, mu * mu, gam * gam, a64[:, c])
        factor = _twin_factor(N)
        if factor is None:
            out["flag"][c] = 1
            continue
        col[c] = dict(G=G, used=used, rho=rho, N=N, factor=factor, b=b)
    edges = {c: [n for n in (c - 1, c + 1, c - nx, c + nx) if n in col] if with_edges else [] for c in col}
    for c in col:
        out["deg"][c] = len(edges[c])

    def apply(y):
        q = {}
        for c, d in col.items():
            t = np.zeros(B)
            for j in range(B):
                t = t + d["N"][:, j] * y[c][j]
            s = np.zeros(B); su = np.zeros(M)
            for n in edges[c]:
                s = s + y[n]
                su = su + (y[n][M:] - y[n][:M])
            deg = float(len(edges[c]))
            fig = t + w2 * (deg * y[c] - s)
            g = wa2 * (deg * (y[c][M:] - y[c][:M]) - su)
            q[c] = np.concatenate([fig[:M] - g, fig[M:] + g])
        return q

    bt = {}
    for c, d in col.items():
        sv = np.zeros(M); sh = np.zeros(M); sa = np.zeros(M)
        for n in edges[c]:
            sv = sv + (v64[:, c] - v64[:, n])
            sh = sh + (h64[:, c] - h64[:, n])
            sa = sa + (a64[:, c] - a64[:, n])
        bt[c] = np.concatenate([(d["b"][:M] - w2 * sv) + wa2 * sa, (d["b"][M:] - w2 * sh) - wa2 * sa]) if with_edges else d["b"].copy()
    x, out["itn"], out["istop"], out["rz0"], out["rz"] = _twin_pcg(col, interior, bt, apply, with_edges, tol, maxit)
    if col:
        Lm = column_l(M); Z = np.zeros_like(Lm); I = np.eye(M)

        def own(c):
            u = col[c]["used"]
            Gc = np.zeros((int(u.sum()), B))
            Gc[:, :M] = np.where(love[u, None], 0.0, col[c]["G"][u]); Gc[:, M:] = np.where(love[u, None], col[c]["G"][u], 0.0)
            return [(Gc, col[c]["rho"][u]), (lam * np.hstack([Lm, Z]), np.zeros(Lm.shape[0])), (lam * np.hstack([Z, Lm]), np.zeros(Lm.shape[0])),
                    (mu * np.eye(B), np.zeros(B)), (gam * np.hstack([-I, I]), -gam * a64[:, c])]

        between = lambda c, n: [(weight * pick, -weight * (field[:, c] - field[:, n])) for weight, pick, field in
                                ((lat, np.hstack([I, 0 * I]), v64), (lat, np.hstack([0 * I, I]), h64), (lata, np.hstack([-I, I]), a64)) if weight > 0.0]
        other = _twin_stacked(col, edges, B, own, between)
    for c in col:
        out["delta"][:, c] = x[c]
        out["delta_lstsq"][:, c] = other[c]
    s = _twin_clip(out["delta"], dvmax)
    for c in col:
        vsv[:M, c] = _twin_stepped(vsv[:M, c], s[:M, c], minvel, maxvel)
        vsh[:M, c] = _twin_stepped(vsh[:M, c], s[M:, c], minvel, maxvel)
    out["dv"] = np.ascontiguousarray(s.reshape(2, M, ncol))
    return out


def _chain_dot(u, w):
    """sum_l u[l] w[l], l ascending from 0.0"""
    s = 0.0
    for a, b in zip(u, w):
        s = s + float(a) * float(b)
    return s


def _resolution_measures(T, G, used, depz):
    """R = T^T G and what column_resolution.h reduces from it, every sum from 0.0 in the header's order: over the used k ascending, over l
    and j ascending.  Returns dict(R (M, M), measures (4, M): R_jj, m1, m2, var; leverage (K); trace)."""
    K, M = G.shape
    z = np.asarray(depz, np.float32)[:M].astype(np.float64)
    R = np.zeros((M, M)); var = np.zeros(M)
    for k in np.flatnonzero(used):
        R = R + np.outer(T[k], G[k])
        var = var + T[k] * T[k]
    m1 = np.zeros(M); m2 = np.zeros(M)
    for l in range(M):
        r2 = R[l] * R[l]
        dz = z[l] - z
        m1 = m1 + r2
        m2 = m2 + r2 * (dz * dz)
    h = np.zeros(K)
    for l in range(M):
        h = h + G[:, l] * T[:, l]
    h[~used] = 0.0
    trace = 0.0
    for j in range(M):
        trace = trace + R[j, j]
    return dict(R=R, measures=np.stack([np.diag(R).copy(), m1, m2, var]), leverage=h, trace=float(trace))


def column_resolution_twin(obs, wt, pv, S, depz, smooth, damp, n_override=None):
    """dsa_columns_resolution on one column in NumPy (csrc/column_resolution.h).  obs, wt, pv, S as column_step_twin's; depz: the depths of
    the unknowns (M or more, fp32).  N is built as column_step_twin builds it; row k of T (K, M) is the solution of N t = g_k through the
    header's L D L^T order, rows of unused data 0; R = T^T G.  Returns dict(T, R (M, M), measures (4, M): R_jj, m1, m2, var; leverage (K);
    trace; nused; flag; other) -- every array 0 where the flag is 1 or 2.  other: the same figures (T, R, measures, leverage, trace) by
    another algorithm, numpy.linalg.pinv of the stacked [diag(a) S; smooth L; damp I], whose first K columns are N^-1 G^T -- for the size
    of the rounding error; None where the column is flagged.  n_override: an (M, M) matrix in place of the assembled N (tests)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    used, _, _, G = _twin_data(obs, wt, pv, S)
    out = dict(T=np.zeros((K, M)), R=np.zeros((M, M)), measures=np.zeros((4, M)), leverage=np.zeros(K), trace=0.0, nused=int(used.sum()), flag=0, other=None)
    if out["nused"] == 0:
        out["flag"] = 2
        return out
    lam2, mu2 = float(f(smooth)) * float(f(smooth)), float(f(damp)) * float(f(damp))
    N, _ = _twin_normal(G, used, np.zeros(K), lam2, mu2)
    if n_override is not None:
        N = np.array(n_override, np.float64)
    factor = _twin_factor(N)
    if factor is None:
        out["flag"] = 1
        return out
    T = _twin_solve(*factor, G.T).T.copy()
    T[~used] = 0.0
    out.update(T=T, **_resolution_measures(T, G, used, depz))
    if n_override is None:
        A = np.vstack([G, float(f(smooth)) * column_l(M), float(f(damp)) * np.eye(M)])
        T2 = np.linalg.pinv(A)[:, :K].T.copy()
        T2[~used] = 0.0
        out["other"] = dict(T=T2, **_resolution_measures(T2, G, used, depz))
    return out


def azimuthal_factor(svs, vels):
    """The depth factor of the gc / gs unknowns with k_sen_azimuthal's roundings (DESIGN.md sections 18 and 35): Z = svs (double)(0.5f v), one
    fp32 product and one fp64 product.  svs: (nz, K, ncol) fp64, dispersion_fetch's d c / d Vs; vels: the fp32 model, (nz, ...) with ncol
    values per depth.  Returns Z (nz - 1, K, ncol) fp64: the bottom depth carries no unknown."""
    svs = np.asarray(svs, np.float64)
    v = np.asarray(vels, np.float32).reshape(np.shape(vels)[0], -1)
    M = v.shape[0] - 1
    half = (np.float32(0.5) * v[:M]).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return svs[:M] * half[:, None, :]


def column_azimuthal_twin(obs, a1, a2, wt, pv, Z, love, depz, smooth, damp, n_override=None):
    """dsa_columns_azimuthal on one column in NumPy (csrc/column_azimuthal.h).  obs (the c0 values), wt, pv as column_step_twin's; a1, a2 (K)
    fp32, the 2 psi terms; Z (K, M) fp64, azimuthal_factor's rows of this column; love (K) bool or None: a Love slot is a slot of weight 0.
    The operator is column_resolution_twin's on (obs, the effective weights, pv, Z); rhoc = a a1, rhos = a a2, bc = G^T rhoc, bs = G^T rhos
    over the used k ascending; gc and gs through the header's L D L^T order; f = G g with l ascending.  Returns dict(gc, gs (M); chi2 (4):
    before c, before s, after c, after s; measures (4, M); leverage (K); nused; flag; T (K, M); R (M, M); other) -- every array 0 where the
    flag is 1 or 2.  other: gc, gs and chi2 by another algorithm, numpy.linalg.lstsq on the stacked [diag(a) Z; smooth L; damp I], with
    column_resolution_twin's second measures and leverage -- for the size of the rounding error; None where the column is flagged or N is
    overridden."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); Z = np.asarray(Z, np.float64)
    K, M = Z.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    if love is not None:
        wt = np.where(np.asarray(love, bool), f(0.0), wt).astype(f)
    res = column_resolution_twin(obs, wt, pv, Z, depz, smooth, damp, n_override)
    out = dict(gc=np.zeros(M), gs=np.zeros(M), chi2=np.zeros(4), measures=res["measures"], leverage=res["leverage"], nused=res["nused"], flag=res["flag"],
               T=res["T"], R=res["R"], other=None)
    if out["flag"]:
        return out
    used, _, _, G = _twin_data(obs, wt, pv, Z)
    a = wt.astype(np.float64)
    rho = [np.where(used, a * np.where(used, np.asarray(x, f), f(0.0)).astype(np.float64), 0.0) for x in (a1, a2)]
    lam2, mu2 = float(f(smooth)) * float(f(smooth)), float(f(damp)) * float(f(damp))
    rows = np.flatnonzero(used)

    def misfit(r):
        s = 0.0
        for k in rows:
            s = s + r[k] * r[k]
        return s

    def fit(g):
        return np.array([_chain_dot(G[k], g) if used[k] else 0.0 for k in range(K)])

    g, chi2 = [], [misfit(rho[0]), misfit(rho[1]), 0.0, 0.0]
    for q in range(2):
        N, b = _twin_normal(G, used, rho[q], lam2, mu2)
        if n_override is not None:
            N = np.array(n_override, np.float64)
        g.append(_twin_solve(*_twin_factor(N), b))
        chi2[2 + q] = misfit(rho[q] - fit(g[q]))
    out.update(gc=g[0], gs=g[1], chi2=np.array(chi2))
    if n_override is None:
        A = np.vstack([G[used], float(f(smooth)) * column_l(M), float(f(damp)) * np.eye(M)])
        g2 = [np.linalg.lstsq(A, np.concatenate([rho[q][used], np.zeros(A.shape[0] - rows.size)]), rcond=None)[0] for q in range(2)]
        out["other"] = dict(gc=g2[0], gs=g2[1], chi2=np.array(chi2[:2] + [misfit(rho[q] - fit(g2[q])) for q in range(2)]),
                            measures=res["other"]["measures"], leverage=res["other"]["leverage"])
    return out


def _radial_expand(G, love):
    """the expanded G^ (K, 2M): row k is G[k] in the block of its wave type (Vsv for Rayleigh, Vsh for Love) and 0.0 elsewhere"""
    K, M = G.shape
    Gx = np.zeros((K, 2 * M))
    Gx[:, :M] = np.where(love[:, None], 0.0, G); Gx[:, M:] = np.where(love[:, None], G, 0.0)
    return Gx


def _radial_resolution_measures(T, G, used, love, depz):
    """R = T^T G^ and what column_radial_resolution.h reduces from it, every sum from 0.0 in the header's order: over the used k ascending, over
    i ascending within each block.  T (K, 2M), G (K, M) compact.  Returns dict(R (2M, 2M), measures (6, 2M): R_jj, m1_own, m2_own, m1_cross,
    R_cross, var; pair (2, M): cov, vard; leverage (K); trace (2))."""
    K, M = G.shape
    n = 2 * M
    z = np.asarray(depz, np.float32)[:M].astype(np.float64)
    z2 = np.concatenate([z, z])
    block = np.arange(n) >= M
    R = np.zeros((n, n)); var = np.zeros(n); cov = np.zeros(M); vard = np.zeros(M)
    for k in np.flatnonzero(used):
        q = int(love[k])
        R[:, q * M:(q + 1) * M] = R[:, q * M:(q + 1) * M] + np.outer(T[k], G[k])
        var = var + T[k] * T[k]
        cov = cov + T[k, :M] * T[k, M:]
        d = T[k, M:] - T[k, :M]
        vard = vard + d * d
    m1 = np.zeros(n); m2 = np.zeros(n); mx = np.zeros(n)
    for i in range(n):
        r2 = R[i] * R[i]
        dz = z2[i] - z2
        own = block == block[i]
        m1 = np.where(own, m1 + r2, m1)
        m2 = np.where(own, m2 + r2 * (dz * dz), m2)
        mx = np.where(own, mx, mx + r2)
    rx = np.array([R[j - M if j >= M else j + M, j] for j in range(n)])
    h = np.zeros(K)
    first = np.where(love, M, 0)
    for l in range(M):
        h = h + G[:, l] * T[np.arange(K), first + l]
    h[~used] = 0.0
    trace = [0.0, 0.0]
    for j in range(n):
        trace[int(j >= M)] = trace[int(j >= M)] + R[j, j]
    return dict(R=R, measures=np.stack([np.diag(R).copy(), m1, m2, mx, rx, var]), pair=np.stack([cov, vard]), leverage=h, trace=np.array(trace))


def column_radial_resolution_twin(obs, wt, pv, S, love, depz, smooth, damp, aniso, n_override=None):
    """dsa_columns_resolution_radial on one column in NumPy (csrc/column_radial_resolution.h).  obs, wt, pv, S and love as column_radial_twin's;
    depz: the depths of the unknowns (M or more, fp32).  N is built as column_radial_twin builds it (the starting models enter b only, which
    nothing here reads); row k of T (K, 2M) is the solution of N t = g^_k through the header's L D L^T order, rows of unused data 0;
    R = T^T G^.  Returns dict(T, R (2M, 2M), measures (6, 2M), pair (2, M), leverage (K), trace (2), nused [Rayleigh, Love], flag, other) --
    every array 0 where the flag is 1 or 2.  other: the same figures by another algorithm, numpy.linalg.pinv of the stacked
    [G^; smooth L (+) smooth L; damp I; aniso (-I | I)], whose first K columns are N^-1 G^^T -- for the size of the rounding error; None where
    the column is flagged.  n_override: a (2M, 2M) matrix in place of the assembled N (tests)."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64); love = np.asarray(love, bool)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    used, _, _, G = _twin_data(obs, wt, pv, S, love)
    out = dict(T=np.zeros((K, 2 * M)), R=np.zeros((2 * M, 2 * M)), measures=np.zeros((6, 2 * M)), pair=np.zeros((2, M)), leverage=np.zeros(K), trace=np.zeros(2),
               nused=[int((used & ~love).sum()), int((used & love).sum())], flag=0, other=None)
    if not used.any():
        out["flag"] = 2
        return out
    lam, mu, gam = float(f(smooth)), float(f(damp)), float(f(aniso))
    N, _ = _twin_radial_normal(G, used, love, np.zeros(K), lam * lam, mu * mu, gam * gam, np.zeros(M))
    if n_override is not None:
        N = np.array(n_override, np.float64)
    factor = _twin_factor(N)
    if factor is None:
        out["flag"] = 1
        return out
    Gx = _radial_expand(G, love)
    T = _twin_solve(*factor, Gx.T).T.copy()
    T[~used] = 0.0
    out.update(T=T, **_radial_resolution_measures(T, G, used, love, depz))
    if n_override is None:
        Lm = column_l(M); Z = np.zeros_like(Lm)
        A = np.vstack([Gx, lam * np.hstack([Lm, Z]), lam * np.hstack([Z, Lm]), mu * np.eye(2 * M), gam * np.hstack([-np.eye(M), np.eye(M)])])
        T2 = np.linalg.pinv(A)[:, :K].T.copy()
        T2[~used] = 0.0
        out["other"] = dict(T=T2, **_radial_resolution_measures(T2, G, used, love, depz))
    return out


# ---- the Monte-Carlo depth inversion: the twin of csrc/column_sample.h ----

_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15


def sample_mix(x):
    """splitmix64's finaliser on a Python integer, modulo 2^64"""
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _M64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_bits(seed, column, chain, sweep, draw):
    """the 53 bits k of draw (column, chain, sweep, draw): u = k 2^-53"""
    x = int(seed) & _M64
    for w in (column, chain, sweep, draw):
        x = sample_mix((x + _GOLDEN + int(w)) & _M64)
    return x >> 11


def sample_unit(k):
    return float(k) * 2.0 ** -53


def sample_neglog(k):
    """-ln(k 2^-53) for 1 <= k < 2^53 with the header's operations: the mantissa m in [sqrt(1/2), sqrt(2)) by integer operations, ln m = 2 s
    (1 + s^2 / 3 + ... + s^22 / 23), s = (m - 1) / (m + 1), ln 2 in two parts"""
    k = int(k)
    p = k.bit_length() - 1
    frac = (k << (52 - p)) & 0x000FFFFFFFFFFFFF
    n, ex = p - 53, 1023
    if frac > 0x0006A09E667F3BCC:
        ex, n = 1022, n + 1
    m = float(np.array([(ex << 52) | frac], np.uint64).view(np.float64)[0])
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    t = 1.0 / 23.0
    for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0, 1.0):
        t = t * z + 1.0 / d
    lnm = 2.0 * s * t
    dn = float(n)
    return -(dn * 6.93147180369123816490e-01 + (lnm + dn * 1.90821492927058770002e-10))


def _f64_bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def _f64_from_bits(b):
    return float(np.array([b], np.uint64).view(np.float64)[0])


def sample_rsqrt(d):
    """1 / sqrt(d) for a normal positive finite d with the header's operations: d = m 4^h, m in [1, 4), by integer operations, the seed from m's
    bits, six Newton steps y = y (1.5 - (m / 2) y y), the result y 2^-h"""
    b = _f64_bits(float(d))
    e = ((b >> 52) & 0x7FF) - 1023
    odd = e & 1
    h = (e - odd) // 2
    mb = ((1023 + odd) << 52) | (b & 0x000FFFFFFFFFFFFF)
    m = _f64_from_bits(mb)
    hm = 0.5 * m
    y = _f64_from_bits(0x5FE6EB50C7B537A9 - (mb >> 1))
    for _ in range(6):
        y = y * (1.5 - hm * y * y)
    return y * _f64_from_bits((1023 - h) << 52)


def sample_block_scale(M, temperature=1.0):
    """the default scale of a block proposal: 2.38 sqrt(3 T / M) -- the random-walk optimum 2.38^2 / M of a proposal of M unknowns whose
    draws z have variance 1 / 3, at temperature T"""
    return 2.38 * math.sqrt(3.0 * float(temperature) / float(M))


def column_tri(i, j):
    """column_system.h's packed lower triangle, row by row: entry (i, j), j <= i"""
    return i * (i + 1) // 2 + j


def column_shape_twin(obs, wt, pv, S, smooth, damp):
    """The shape of one column for the block proposals (csrc/column_sample.h: sample_shape): N = G^T G + smooth^2 L^T L + damp^2 I of the
    column's data (obs, wt (K) fp32 or None, pv (K), S (K, M): column_step_twin's) factored as L D L^T.  Returns (tri (M (M + 1) / 2): N's
    diagonal and L below it in column_tri's order, r (M) = sample_rsqrt(d), flag); flag 2 without a used datum, 1 at a bad pivot, tri and r
    then zeros."""
    f = np.float32
    obs = np.asarray(obs, f); pv = np.asarray(pv, np.float64); S = np.asarray(S, np.float64)
    K, M = S.shape
    wt = np.ones(K, f) if wt is None else np.asarray(wt, f)
    tri = np.zeros(M * (M + 1) // 2); r = np.zeros(M)
    used, rho, _, G = _twin_data(obs, wt, pv, S)
    if not used.any():
        return tri, r, 2
    N, _ = _twin_normal(G, used, rho, float(f(smooth)) * float(f(smooth)), float(f(damp)) * float(f(damp)))
    factor = _twin_factor(N)
    if factor is None:
        return tri, r, 1
    Lm, d = factor
    for i in range(M):
        for j in range(i):
            tri[column_tri(i, j)] = Lm[i, j]
        tri[column_tri(i, i)] = N[i, i]
        r[i] = sample_rsqrt(d[i])
    return tri, r, 0


def sample_psi(v, lam2):
    """smooth^2 |L v|^2 of one column's M values, the rows in the header's order, every row summed from 0.0 over its unknowns ascending"""
    v = [float(x) for x in v]
    M = len(v)
    if M < 2:
        return 0.0
    s = 0.0
    t = (0.0 + v[0]) - v[1]
    s += t * t
    for l in range(1, M - 1):
        t = ((0.0 - v[l - 1]) + 2.0 * v[l]) - v[l + 1]
        s += t * t
    t = (0.0 - v[M - 2]) + v[M - 1]
    s += t * t
    return lam2 * s


def column_sample_twin(nx, ny, start, obs, wt, forward, nchains, sweeps, burn, smooth, step, spread, width, temperature, minvel, maxvel, seed, after=None,
                       shape=None, block_every=0, block_scale=None):
    """The Monte-Carlo depth inversion in Python integers and NumPy float64 / float32 scalars, the header's operations in the header's order.
    start (nz, ny * nx) fp32; obs / wt (K, ny * nx) fp32, wt may be None (1); forward(models (nz, C, ncol) fp32) -> pv (C, K, ncol) fp64 in
    place of the dispersion stage (a value <= 0: no root); after(sweep, state): a hook after the set-up (sweep 0) and every sweep.  Returns
    dict(models, phi, psi, counters (4, C, ncol): accepted, rejected, out of box, no root; S1, S2, phisum, nkept, best_e, best_v, pnode,
    pold, pmark, reseeded, used, nused, flag, phi_start, and the finish: mean, var, W, B, best (M, ncol), best_energy, mean_phi (ncol)).
    Block proposals: shape = dict(tri (M (M + 1) / 2, ncol), r (M, ncol), flag (ncol)), column_shape_twin's figures of
    every column; sweep s is a block sweep where block_every > 0 and s % block_every == 0; block_scale None: sample_block_scale(M,
    temperature).  The state then also holds pold_all (M, C, ncol) fp32 and block_counters (3, C, ncol): proposed, accepted, out of box.
    With block_every = 0 (the default) the shape is not looked at and every bit is the single-node sampler's."""
    F = np.float32
    start = np.asarray(start, F)
    nz, ncol = start.shape
    M, C = nz - 1, int(nchains)
    obs = np.asarray(obs, F)
    K = obs.shape[0]
    lam2 = float(F(smooth)) * float(F(smooth)); step = float(F(step)); spread = float(F(spread)); two_t = 2.0 * float(F(temperature))
    width, minvel, maxvel = F(width), F(minvel), F(maxvel)
    interior = lambda c: 1 <= c % nx <= nx - 2 and 1 <= c // nx <= ny - 2
    a_of = lambda k, c: 1.0 if wt is None else float(F(wt[k, c]))
    block_every = int(block_every)
    if block_every > 0:
        if shape is None:
            raise ValueError("column_sample_twin: block sweeps need a shape")
        block_scale = sample_block_scale(M, float(F(temperature))) if block_scale is None else float(block_scale)
        tri, rr, sflag = (np.asarray(shape[n]) for n in ("tri", "r", "flag"))

    def box(c, l):
        lo, hi = F(start[l, c] - width), F(start[l, c] + width)
        return (minvel if lo < minvel else lo), (maxvel if hi > maxvel else hi)

    def phi_of(pv, c, q, used):
        phi, bad = 0.0, False
        for k in used:
            p = float(pv[q, k, c])
            if not p > 0.0:
                bad = True
                continue
            rho = a_of(k, c) * (float(obs[k, c]) - p)
            phi += rho * rho
        return phi, bad

    st = dict(models=np.zeros((nz, C, ncol), F), phi=np.zeros((C, ncol)), psi=np.zeros((C, ncol)), counters=np.zeros((4, C, ncol), np.int32),
              S1=np.zeros((M, C, ncol)), S2=np.zeros((M, C, ncol)), phisum=np.zeros((C, ncol)), nkept=np.zeros((C, ncol), np.int32), best_e=np.zeros((C, ncol)),
              best_v=np.zeros((M, C, ncol), F), pnode=np.zeros((C, ncol), np.int32), pold=np.zeros((C, ncol), F), pmark=np.full((C, ncol), -1, np.int32),
              reseeded=np.zeros((C, ncol), np.int32), nused=np.zeros(ncol, np.int32), flag=np.zeros(ncol, np.int32), phi_start=np.zeros(ncol),
              pold_all=np.zeros((M, C, ncol), F), block_counters=np.zeros((3, C, ncol), np.int32))
    v = st["models"]
    for q in range(C):
        for c in range(ncol):
            v[:, q, c] = start[:, c]
            if q > 0 and interior(c):
                for l in range(M):
                    u = sample_unit(sample_bits(seed, c, q, 0, l))
                    lo, hi = box(c, l)
                    x = F(start[l, c] + F(spread * (2.0 * u - 1.0)))
                    v[l, q, c] = lo if x < lo else hi if x > hi else x
    pv = np.asarray(forward(v), np.float64).reshape(C, K, ncol)
    used_of = {}
    for c in range(ncol):
        if not interior(c):
            continue
        used = [k for k in range(K) if a_of(k, c) > 0.0 and obs[k, c] > 0 and pv[0, k, c] > 0.0]
        used_of[c] = used
        st["nused"][c] = len(used)
        st["flag"][c] = 0 if used else 2
        if not used:
            v[:M, :, c] = start[:M, c][:, None]
            continue
        st["phi_start"][c] = phi_of(pv, c, 0, used)[0]
        for q in range(C):
            phi, bad = phi_of(pv, c, q, used)
            if bad:
                v[:M, q, c] = start[:M, c]
                st["reseeded"][q, c] = 1
                phi = st["phi_start"][c]
            st["phi"][q, c] = phi
            st["psi"][q, c] = sample_psi(v[:M, q, c], lam2)
    st["used"] = used_of
    moving = [c for c in range(ncol) if interior(c) and used_of.get(c)]
    if after is not None:
        after(0, st)
    cnt = st["counters"]; bcnt = st["block_counters"]
    for sweep in range(1, int(sweeps) + 1):
        st["pmark"][...] = -1
        blocks = block_every > 0 and sweep % block_every == 0
        for q in range(C):
            for c in moving:
                if blocks and sflag[c] == 0:
                    delta = [0.0] * M
                    for i in range(M - 1, -1, -1):
                        u = sample_unit(sample_bits(seed, c, q, sweep, 3 + i))
                        s = (2.0 * u - 1.0) * float(rr[i, c])
                        for p in range(i + 1, M):
                            s = s - float(tri[column_tri(p, i), c]) * delta[p]
                        delta[i] = s
                    new = [F(v[l, q, c] + F(block_scale * delta[l])) for l in range(M)]
                    if any(new[l] < box(c, l)[0] or new[l] > box(c, l)[1] for l in range(M)):
                        st["pmark"][q, c] = 1
                        continue
                    st["pold_all"][:, q, c] = v[:M, q, c]
                    v[:M, q, c] = new
                    st["pnode"][q, c] = -1
                    st["pmark"][q, c] = 0
                    continue
                u0 = sample_unit(sample_bits(seed, c, q, sweep, 0)); u1 = sample_unit(sample_bits(seed, c, q, sweep, 1))
                l = min(int(u0 * float(M)), M - 1)
                old = v[l, q, c]
                x = F(old + F(step * (2.0 * u1 - 1.0)))
                lo, hi = box(c, l)
                st["pnode"][q, c] = l; st["pold"][q, c] = old
                if x < lo or x > hi:
                    st["pmark"][q, c] = 1
                else:
                    v[l, q, c] = x
                    st["pmark"][q, c] = 0
        pv = np.asarray(forward(v), np.float64).reshape(C, K, ncol)
        for q in range(C):
            for c in moving:
                block = blocks and sflag[c] == 0
                if block:
                    bcnt[0, q, c] += 1
                if st["pmark"][q, c] == 1:
                    cnt[2, q, c] += 1; cnt[1, q, c] += 1
                    if block:
                        bcnt[2, q, c] += 1
                else:
                    phi_new, bad = phi_of(pv, c, q, used_of[c])
                    accepted, psi_new = False, 0.0
                    if not bad:
                        psi_new = sample_psi(v[:M, q, c], lam2)
                        delta = (phi_new + psi_new) - (st["phi"][q, c] + st["psi"][q, c])
                        if delta == delta:
                            if delta <= 0.0:
                                accepted = True
                            else:
                                k = sample_bits(seed, c, q, sweep, 2)
                                accepted = k == 0 or delta / two_t < sample_neglog(k)
                    if accepted:
                        st["phi"][q, c] = phi_new; st["psi"][q, c] = psi_new
                        cnt[0, q, c] += 1
                        st["pmark"][q, c] = 2
                        if block:
                            bcnt[1, q, c] += 1
                    else:
                        if block:
                            v[:M, q, c] = st["pold_all"][:, q, c]
                        else:
                            v[st["pnode"][q, c], q, c] = st["pold"][q, c]
                        cnt[1, q, c] += 1
                        if bad:
                            cnt[3, q, c] += 1
                        st["pmark"][q, c] = 4 if bad else 3
                if sweep <= burn:
                    continue
                for l in range(M):
                    d = float(v[l, q, c]) - float(start[l, c])
                    st["S1"][l, q, c] += d
                    st["S2"][l, q, c] += d * d
                energy = float(st["phi"][q, c]) + float(st["psi"][q, c])
                st["phisum"][q, c] += st["phi"][q, c]
                if st["nkept"][q, c] == 0 or energy < st["best_e"][q, c]:
                    st["best_e"][q, c] = energy
                    st["best_v"][:, q, c] = v[:M, q, c]
                st["nkept"][q, c] += 1
        if after is not None:
            after(sweep, st)
    fin = dict(mean=np.zeros((M, ncol)), var=np.zeros((M, ncol)), W=np.zeros((M, ncol)), B=np.zeros((M, ncol)), best=np.zeros((M, ncol)), best_energy=np.zeros(ncol),
               mean_phi=np.zeros(ncol))
    for c in range(ncol):
        n = int(st["nkept"][0, c])
        if n == 0:
            continue
        dn, dc = float(n), float(C)
        best_q = 0
        for q in range(1, C):
            if st["best_e"][q, c] < st["best_e"][best_q, c]:
                best_q = q
        for l in range(M):
            s1 = s2 = sw = sm = 0.0
            for q in range(C):
                a, b = float(st["S1"][l, q, c]), float(st["S2"][l, q, c])
                m = a / dn
                s1 += a; s2 += b; sw += b / dn - m * m; sm += m
            pm, mbar = s1 / (dn * dc), sm / dc
            sb = 0.0
            for q in range(C):
                d = float(st["S1"][l, q, c]) / dn - mbar
                sb += d * d
            fin["mean"][l, c] = float(start[l, c]) + pm
            fin["var"][l, c] = s2 / (dn * dc) - pm * pm
            fin["W"][l, c] = sw / dc
            fin["B"][l, c] = sb / (dc - 1.0) if C > 1 else 0.0
            fin["best"][l, c] = float(st["best_v"][l, best_q, c])
        phis = 0.0
        for q in range(C):
            phis += float(st["phisum"][q, c])
        fin["best_energy"][c] = st["best_e"][best_q, c]
        fin["mean_phi"][c] = phis / (dn * dc)
    st.update(fin)
    return st


def sample_rhat(W, B, nkept):
    """the convergence figure sqrt((W (n - 1) / n + B) / W) of every unknown, 1 where W = 0 (nothing moved) or nothing was kept"""
    W = np.asarray(W, np.float64); B = np.asarray(B, np.float64)
    n = np.broadcast_to(np.asarray(nkept, np.float64), W.shape)
    ok = (W > 0) & (n > 0)
    ratio = np.divide(W * (n - 1.0) / np.where(n > 0, n, 1.0) + B, W, out=np.ones(W.shape), where=ok)
    return np.sqrt(ratio)


def sample_sd(var):
    """sqrt of the pooled variance, a rounding-negative variance taken as 0"""
    return np.sqrt(np.maximum(np.asarray(var, np.float64), 0.0))


# ---- the posterior marginals: the twin of csrc/column_sample.h's bin, mode and quantile rules ----

def sample_box(v0, width, minvel, maxvel):
    """the box of every node in fp32, as sample_box: (max(minvel, v0 - width), min(maxvel, v0 + width))"""
    F = np.float32
    v0 = np.asarray(v0, F)
    return np.maximum(v0 - F(width), F(minvel)), np.minimum(v0 + F(width), F(maxvel))


def sample_marginal_bin(v, lo, hi, nbins):
    """sample_bin of every value of v (fp32) in the box [lo, hi] (fp32, broadcast against v) cut into nbins bins: int32.  Bin 0 in a box
    without width; a value outside the box falls into an end bin."""
    v, lo, hi = (np.asarray(a, np.float32).astype(np.float64) for a in (v, lo, hi))
    v, lo, hi = np.broadcast_arrays(v, lo, hi)
    w = hi - lo
    ok = w > 0
    with np.errstate(all="ignore"):
        x = ((v - lo) / np.where(ok, w, 1.0)) * float(nbins)
    b = np.where(x < 0, 0.0, np.where(x >= nbins, float(nbins - 1), np.floor(x)))      # ((int)x of an x >= 0 is its floor)
    return np.where(ok, b, 0.0).astype(np.int32)


def sample_marginal_counts(models, start, width, minvel, maxvel, nbins):
    """what one kept sweep adds to the pooled histogram: models (nz, C, ncol) fp32, the chains' states, start (nz, ncol) fp32.  Returns
    (nbins, nz - 1, ncol) int64, the chains of every node per bin.  The caller leaves out the columns whose chains are idle."""
    models = np.asarray(models, np.float32)
    nz, Cn, ncol = models.shape
    M = nz - 1
    lo, hi = sample_box(np.asarray(start, np.float32).reshape(nz, ncol)[:M], width, minvel, maxvel)
    b = sample_marginal_bin(models[:M], lo[:, None, :], hi[:, None, :], nbins)
    out = np.zeros((nbins, M, ncol), np.int64)
    li, ci = np.meshgrid(np.arange(M), np.arange(ncol), indexing="ij")
    for q in range(Cn):
        np.add.at(out, (b[:, q], li, ci), 1)
    return out


def sample_marginal_mode(h, lo, hi):
    """sample_marginal_finish's mode of the pooled counts h (nbins) of one node: the centre of the first fullest bin; 0.0 without a count"""
    h = [int(x) for x in h]
    nb = len(h)
    if sum(h) == 0:
        return 0.0
    dlo = float(np.float32(lo)); w = float(np.float32(hi)) - dlo
    b = h.index(max(h))
    return dlo + ((float(b) + 0.5) / float(nb)) * w


def sample_marginal_quantile(h, lo, hi, p):
    """sample_marginal_finish's quantile of level p of the pooled counts h (nbins) of one node, linear inside the bin that reaches p of the
    total; 0.0 without a count"""
    h = [int(x) for x in h]
    nb, N = len(h), sum(h)
    if N == 0:
        return 0.0
    dlo = float(np.float32(lo)); w = float(np.float32(hi)) - dlo
    target = float(p) * float(N)
    cum = 0
    for b in range(nb):
        if h[b] > 0 and float(cum + h[b]) >= target:
            frac = (target - float(cum)) / float(h[b])
            return dlo + ((float(b) + frac) / float(nb)) * w
        cum += h[b]
    return 0.0


class SampleMarginalTwin:
    """The marginals' state beside column_sample_twin: pass `after` as its hook.  hist (nbins, M, C, ncol) uint32 and, with_cov, P
    (M (M + 1) / 2, C, ncol): after every sweep > burn the state of every chain that is not idle is counted and its products are added,
    as sample_marginal_hist and sample_marginal_cov do.  finish(state, levels): dict(hist: the pooled counts, mode, quantiles, cov)."""

    def __init__(self, start, nchains, width, minvel, maxvel, burn, nbins, with_cov=False):
        self.start = np.asarray(start, np.float32)
        nz, ncol = self.start.shape
        self.M, self.C, self.ncol, self.burn, self.nbins = nz - 1, int(nchains), ncol, int(burn), int(nbins)
        self.box = (width, minvel, maxvel)
        self.lo, self.hi = sample_box(self.start[:self.M], width, minvel, maxvel)
        self.hist = np.zeros((self.nbins, self.M, self.C, ncol), np.uint32)
        self.P = np.zeros((self.M * (self.M + 1) // 2, self.C, ncol)) if with_cov else None

    def after(self, sweep, st):
        if sweep <= self.burn:
            return
        M = self.M
        v = np.asarray(st["models"], np.float32)[:M]
        kept = np.asarray(st["pmark"]) != -1                                         # (C, ncol)
        b = sample_marginal_bin(v, self.lo[:, None, :], self.hi[:, None, :], self.nbins)
        li, qi, ci = np.nonzero(np.broadcast_to(kept[None], b.shape))
        np.add.at(self.hist, (b[li, qi, ci], li, qi, ci), 1)
        if self.P is not None:
            d = v.astype(np.float64) - self.start[:M].astype(np.float64)[:, None, :]
            for i in range(M):
                for j in range(i + 1):
                    e = column_tri(i, j)
                    self.P[e] = np.where(kept, self.P[e] + d[i] * d[j], self.P[e])

    def finish(self, st, levels):
        M, C = self.M, self.C
        pooled = np.zeros((self.nbins, M, self.ncol), np.uint32)
        for q in range(C):
            pooled += self.hist[:, :, q]
        mode, quant = sample_marginal_twin(pooled, self.start, *self.box, levels)
        out = dict(hist=pooled, mode=mode, quantiles=quant)
        if self.P is not None:
            n = np.asarray(st["nkept"])[0].astype(np.float64)
            ok = n > 0
            den = np.where(ok, n, 1.0) * float(C)
            s1 = np.zeros((M, self.ncol)); sp = np.zeros(self.P.shape[::2])
            for q in range(C):
                s1 = s1 + np.asarray(st["S1"])[:, q]
                sp = sp + self.P[:, q]
            pm = s1 / den
            cov = np.zeros(sp.shape)
            for i in range(M):
                for j in range(i + 1):
                    e = column_tri(i, j)
                    cov[e] = np.where(ok, sp[e] / den - pm[i] * pm[j], 0.0)
            out["cov"] = cov
        return out


def sample_marginal_twin(hist, start, width, minvel, maxvel, levels):
    """mode (M, ncol) and quantiles (len(levels), M, ncol) of the pooled counts hist (nbins, M, ncol) by the two rules above"""
    hist = np.asarray(hist)
    nb, M, ncol = hist.shape
    lo, hi = sample_box(np.asarray(start, np.float32).reshape(-1, ncol)[:M], width, minvel, maxvel)
    mode = np.zeros((M, ncol)); quant = np.zeros((len(levels), M, ncol))
    for l in range(M):
        for c in range(ncol):
            mode[l, c] = sample_marginal_mode(hist[:, l, c], lo[l, c], hi[l, c])
            for k, p in enumerate(levels):
                quant[k, l, c] = sample_marginal_quantile(hist[:, l, c], lo[l, c], hi[l, c], p)
    return mode, quant


# ---- the Monte-Carlo radial depth inversion: the twin of csrc/column_sample_radial.h ----

RADIAL_SAMPLE_NODES = ("mean_v", "var_v", "W_v", "B_v", "mean_h", "var_h", "W_h", "B_h", "mean_xi", "var_xi", "W_xi", "B_xi", "best_v", "best_h", "cov_vh", "p_pos")


def sample_radial_psi(vv, vh, lam2, gam2):
    """psi of one chain: (sample_psi(Vsv) + sample_psi(Vsh)) + gam2 sum_l ((double)vh_l - (double)vv_l)^2, l ascending from 0.0"""
    s = 0.0
    for a, b in zip(vv, vh):
        t = float(b) - float(a)
        s += t * t
    return (sample_psi(vv, lam2) + sample_psi(vh, lam2)) + gam2 * s


def column_sample_radial_twin(nx, ny, start_v, start_h, obs, wt, love, forward, nchains, sweeps, burn, smooth, aniso, step, spread, width, temperature, minvel,
                              maxvel, seed, pairs=True, after=None):
    """The Monte-Carlo radial depth inversion in Python integers and NumPy float64 / float32 scalars, the header's operations in the header's
    order.  start_v, start_h (nz, ny * nx) fp32; obs / wt (K, ny * nx) fp32, wt may be None (1); love (K) bool; forward(vsv, vsh (nz, C, ncol)
    fp32) -> pv (C, K, ncol) fp64 in place of the dispersion stage (a value <= 0: no root); after(sweep, state): a hook after the set-up
    (sweep 0) and every sweep.  Returns dict(vsv, vsh, phi, psi, counters (4, C, ncol), kinds (6, C, ncol): proposed per kind (Vsv, Vsh, pair),
    accepted per kind; S1v, S2v, S1h, S2h, Pvh, X1, X2, npos, phisum, nkept, best_e, best_vsv, best_vsh, pnode, pold_v, pold_h, pmark,
    reseeded, used, nused_r, nused_l, flag, phi_start, and the finish: RADIAL_SAMPLE_NODES (M, ncol), best_energy, mean_phi (ncol))."""
    F = np.float32
    start_v = np.asarray(start_v, F); start_h = np.asarray(start_h, F)
    nz, ncol = start_v.shape
    M, C = nz - 1, int(nchains)
    obs = np.asarray(obs, F)
    K = obs.shape[0]
    love = [bool(x) for x in love]
    lam2 = float(F(smooth)) * float(F(smooth)); gam2 = float(F(aniso)) * float(F(aniso))
    step = float(F(step)); spread = float(F(spread)); two_t = 2.0 * float(F(temperature))
    width, minvel, maxvel = F(width), F(minvel), F(maxvel)
    interior = lambda c: 1 <= c % nx <= nx - 2 and 1 <= c // nx <= ny - 2
    a_of = lambda k, c: 1.0 if wt is None else float(F(wt[k, c]))
    starts = (start_v, start_h)

    def box(b):
        lo, hi = F(b - width), F(b + width)
        return (minvel if lo < minvel else lo), (maxvel if hi > maxvel else hi)

    def phi_of(pv, c, q, used):
        phi, bad = 0.0, False
        for k in used:
            p = float(pv[q, k, c])
            if not p > 0.0:
                bad = True
                continue
            rho = a_of(k, c) * (float(obs[k, c]) - p)
            phi += rho * rho
        return phi, bad

    f64 = lambda *s: np.zeros(s)
    i32 = lambda *s: np.zeros(s, np.int32)
    f32 = lambda *s: np.zeros(s, F)
    st = dict(vsv=f32(nz, C, ncol), vsh=f32(nz, C, ncol), phi=f64(C, ncol), psi=f64(C, ncol), counters=i32(4, C, ncol), kinds=i32(6, C, ncol), S1v=f64(M, C, ncol),
              S2v=f64(M, C, ncol), S1h=f64(M, C, ncol), S2h=f64(M, C, ncol), Pvh=f64(M, C, ncol), X1=f64(M, C, ncol), X2=f64(M, C, ncol), npos=i32(M, C, ncol),
              phisum=f64(C, ncol), nkept=i32(C, ncol), best_e=f64(C, ncol), best_vsv=f32(M, C, ncol), best_vsh=f32(M, C, ncol), pnode=i32(C, ncol), pold_v=f32(C, ncol),
              pold_h=f32(C, ncol), pmark=np.full((C, ncol), -1, np.int32), reseeded=i32(C, ncol), nused_r=i32(ncol), nused_l=i32(ncol), flag=i32(ncol),
              phi_start=f64(ncol))
    vs = (st["vsv"], st["vsh"])
    for q in range(C):
        for c in range(ncol):
            for b in range(2):
                vs[b][:, q, c] = starts[b][:, c]
                if q > 0 and interior(c):
                    for l in range(M):
                        u = sample_unit(sample_bits(seed, c, q, 0, b * M + l))
                        lo, hi = box(starts[b][l, c])
                        x = F(starts[b][l, c] + F(spread * (2.0 * u - 1.0)))
                        vs[b][l, q, c] = lo if x < lo else hi if x > hi else x
    vv, vh = vs
    pv = np.asarray(forward(vv, vh), np.float64).reshape(C, K, ncol)
    used_of = {}
    for c in range(ncol):
        if not interior(c):
            continue
        used = [k for k in range(K) if a_of(k, c) > 0.0 and obs[k, c] > 0 and pv[0, k, c] > 0.0]
        used_of[c] = used
        st["nused_l"][c] = sum(1 for k in used if love[k])
        st["nused_r"][c] = len(used) - st["nused_l"][c]
        st["flag"][c] = 0 if used else 2
        if not used:
            for b in range(2):
                vs[b][:M, :, c] = starts[b][:M, c][:, None]
            continue
        st["phi_start"][c] = phi_of(pv, c, 0, used)[0]
        for q in range(C):
            phi, bad = phi_of(pv, c, q, used)
            if bad:
                for b in range(2):
                    vs[b][:M, q, c] = starts[b][:M, c]
                st["reseeded"][q, c] = 1
                phi = st["phi_start"][c]
            st["phi"][q, c] = phi
            st["psi"][q, c] = sample_radial_psi(vv[:M, q, c], vh[:M, q, c], lam2, gam2)
    st["used"] = used_of
    moving = [c for c in range(ncol) if interior(c) and used_of.get(c)]
    if after is not None:
        after(0, st)
    cnt, kcnt = st["counters"], st["kinds"]
    n = (3 if pairs else 2) * M
    for sweep in range(1, int(sweeps) + 1):
        st["pmark"][...] = -1
        for q in range(C):
            for c in moving:
                u0 = sample_unit(sample_bits(seed, c, q, sweep, 0)); u1 = sample_unit(sample_bits(seed, c, q, sweep, 1))
                i = min(int(u0 * float(n)), n - 1)
                kind = i // M
                l = i - kind * M
                fd = F(step * (2.0 * u1 - 1.0))
                old_v, old_h = vv[l, q, c], vh[l, q, c]
                new_v, new_h = F(old_v + fd), F(old_h + fd)
                kcnt[kind, q, c] += 1
                outside = False
                if kind != 1:
                    lo, hi = box(start_v[l, c])
                    outside = outside or new_v < lo or new_v > hi
                if kind != 0:
                    lo, hi = box(start_h[l, c])
                    outside = outside or new_h < lo or new_h > hi
                if outside:
                    st["pmark"][q, c] = 1
                    continue
                st["pnode"][q, c] = i; st["pold_v"][q, c] = old_v; st["pold_h"][q, c] = old_h
                if kind != 1:
                    vv[l, q, c] = new_v
                if kind != 0:
                    vh[l, q, c] = new_h
                st["pmark"][q, c] = 0
        pv = np.asarray(forward(vv, vh), np.float64).reshape(C, K, ncol)
        for q in range(C):
            for c in moving:
                if st["pmark"][q, c] == 1:
                    cnt[2, q, c] += 1; cnt[1, q, c] += 1
                else:
                    kind = int(st["pnode"][q, c]) // M
                    l = int(st["pnode"][q, c]) - kind * M
                    phi_new, bad = phi_of(pv, c, q, used_of[c])
                    accepted, psi_new = False, 0.0
                    if not bad:
                        psi_new = sample_radial_psi(vv[:M, q, c], vh[:M, q, c], lam2, gam2)
                        delta = (phi_new + psi_new) - (st["phi"][q, c] + st["psi"][q, c])
                        if delta == delta:
                            if delta <= 0.0:
                                accepted = True
                            else:
                                k = sample_bits(seed, c, q, sweep, 2)
                                accepted = k == 0 or delta / two_t < sample_neglog(k)
                    if accepted:
                        st["phi"][q, c] = phi_new; st["psi"][q, c] = psi_new
                        cnt[0, q, c] += 1
                        kcnt[3 + kind, q, c] += 1
                        st["pmark"][q, c] = 2
                    else:
                        if kind != 1:
                            vv[l, q, c] = st["pold_v"][q, c]
                        if kind != 0:
                            vh[l, q, c] = st["pold_h"][q, c]
                        cnt[1, q, c] += 1
                        if bad:
                            cnt[3, q, c] += 1
                        st["pmark"][q, c] = 4 if bad else 3
                if sweep <= burn:
                    continue
                for l in range(M):
                    fv, fh = vv[l, q, c], vh[l, q, c]
                    s_v, s_h = float(start_v[l, c]), float(start_h[l, c])
                    dv, dh = float(fv) - s_v, float(fh) - s_h
                    st["S1v"][l, q, c] += dv; st["S2v"][l, q, c] += dv * dv
                    st["S1h"][l, q, c] += dh; st["S2h"][l, q, c] += dh * dh
                    st["Pvh"][l, q, c] += dv * dh
                    x, x0 = float(fh) / float(fv), s_h / s_v
                    dx = x * x - x0 * x0
                    st["X1"][l, q, c] += dx; st["X2"][l, q, c] += dx * dx
                    if fh > fv:
                        st["npos"][l, q, c] += 1
                energy = float(st["phi"][q, c]) + float(st["psi"][q, c])
                st["phisum"][q, c] += st["phi"][q, c]
                if st["nkept"][q, c] == 0 or energy < st["best_e"][q, c]:
                    st["best_e"][q, c] = energy
                    st["best_vsv"][:, q, c] = vv[:M, q, c]
                    st["best_vsh"][:, q, c] = vh[:M, q, c]
                st["nkept"][q, c] += 1
        if after is not None:
            after(sweep, st)
    fin = {name: np.zeros((M, ncol)) for name in RADIAL_SAMPLE_NODES}
    fin.update(best_energy=np.zeros(ncol), mean_phi=np.zeros(ncol))

    def pool(s1, s2, l, c, dn, dc):
        a1 = a2 = sw = sm = 0.0
        for q in range(C):
            a, b = float(s1[l, q, c]), float(s2[l, q, c])
            m = a / dn
            a1 += a; a2 += b; sw += b / dn - m * m; sm += m
        pm, mbar = a1 / (dn * dc), sm / dc
        sb = 0.0
        for q in range(C):
            d = float(s1[l, q, c]) / dn - mbar
            sb += d * d
        return pm, a2 / (dn * dc) - pm * pm, sw / dc, (sb / (dc - 1.0) if C > 1 else 0.0)

    for c in range(ncol):
        nk = int(st["nkept"][0, c])
        if nk == 0:
            continue
        dn, dc = float(nk), float(C)
        best_q = 0
        for q in range(1, C):
            if st["best_e"][q, c] < st["best_e"][best_q, c]:
                best_q = q
        for l in range(M):
            s_v, s_h = float(start_v[l, c]), float(start_h[l, c])
            x0 = s_h / s_v
            pmv, fin["var_v"][l, c], fin["W_v"][l, c], fin["B_v"][l, c] = pool(st["S1v"], st["S2v"], l, c, dn, dc)
            pmh, fin["var_h"][l, c], fin["W_h"][l, c], fin["B_h"][l, c] = pool(st["S1h"], st["S2h"], l, c, dn, dc)
            pmx, fin["var_xi"][l, c], fin["W_xi"][l, c], fin["B_xi"][l, c] = pool(st["X1"], st["X2"], l, c, dn, dc)
            fin["mean_v"][l, c] = s_v + pmv; fin["mean_h"][l, c] = s_h + pmh; fin["mean_xi"][l, c] = x0 * x0 + pmx
            sp, npos = 0.0, 0
            for q in range(C):
                sp += float(st["Pvh"][l, q, c])
                npos += int(st["npos"][l, q, c])
            fin["best_v"][l, c] = float(st["best_vsv"][l, best_q, c]); fin["best_h"][l, c] = float(st["best_vsh"][l, best_q, c])
            fin["cov_vh"][l, c] = sp / (dn * dc) - pmv * pmh
            fin["p_pos"][l, c] = float(npos) / (dn * dc)
        phis = 0.0
        for q in range(C):
            phis += float(st["phisum"][q, c])
        fin["best_energy"][c] = st["best_e"][best_q, c]
        fin["mean_phi"][c] = phis / (dn * dc)
    st.update(fin)
    return st
