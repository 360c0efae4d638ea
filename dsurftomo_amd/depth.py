"""Depth inversion of the period maps: per-column Vs(z) Gauss-Newton steps on the device.

    python -m dsurftomo_amd.depth <directory with DSurfTomo.in, the data file and MOD> [--maps FILE] [--iterations N] [--smooth L] [--damp D]
                                  [--dvmax V] [--min-dws X] [--out DIR] [--resolution [--sigma S]] [--radial [--aniso G]]
                                  [--lateral W [--lateral-tol T] [--lateral-maxit N]] [--radial-resolution]
                                  [--lateral-resolution [--lateral-resolution-stride N] [--lateral-checkerboard NX,NY,NZ[,AMP]]]
                                  [--sample C,SWEEPS[,BURN] [--sample-step S] [--sample-spread P] [--sample-width W] [--sample-seed N]
                                   [--sample-temperature T] [--sample-block EVERY [--sample-block-scale S]]
                                   [--sample-bins NB [--sample-quantiles P1,P2,...] [--sample-covariance]]]

The second step of the "two-step" method: the phase- and group-velocity maps of dsurftomo_amd.maps (<input>Maps.dat, --maps; read with
maps.read_maps) are inverted, column by column, for the Vs model the direct inversion is compared with.  The maps' period order -- Rayleigh
phase, Rayleigh group, Love phase, Love group -- is the slot order of the dispersion stage: map k and depth-kernel slot k belong to period k.

The model starts as the input's MOD.  Each of --iterations N (default 4) iterations runs, on one engine and without the model leaving the
device: one dispersion_run with kernels per wave type present, then columns_step -- per interior column the K map values against the
column's own curve, (G^T G + smooth^2 L^T L + damp^2 I) delta = G^T rho with the first-difference Laplacian L over depth (--smooth L, default
0.5; --damp D, default 0.1 -- both in units of the weighted sensitivities, which are dimensionless), the step clipped to +- --dvmax V km/s
(default 0.5) and the model to the input file's [minvel, maxvel].  A datum is used where its weight, its map value and the column's curve are
positive; the weights are 1, or 0 where the map's column DWS is below --min-dws X (default 0: every vertex of the maps counts).  The columns
do not see each other: the lateral smoothness of the result is that of the maps.

The log gives, per iteration, the data used, the flagged columns (1: the factorisation met a pivot <= 0; 2: no datum) and the rms
sqrt(sum chi2 / sum nused) before the step.  <input>Depth.dat (write_depth / read_depth): longitude, latitude, depth, Vs of every node, 17
significant digits.  <input>DepthFit.dat (write_fit / read_fit): per column longitude, latitude, the data used, the rms before the first and
before the last step, and the flag of the last step.

--resolution: after the last step the runs are done once more on the final model and columns_resolution asks the
regularised normal matrix of every column, with the loop's weights, --smooth and --damp, how far its answer can be trusted.
<input>DepthResolution.dat (write_resolution / read_resolution): per node above the bottom depth longitude, latitude, depth, R_jj (the
diagonal of the model resolution matrix), the vertical length sqrt(m2 / m1) of the node's point-spread function in km (0 where m1 = 0),
sd_unit = sqrt(var) (the standard deviation for unit variance of the weighted data) and sd = S sd_unit, S = --sigma in km/s or, by default,
the rms before the last step.  <input>DepthLeverage.dat (write_leverage / read_leverage): per column and period in slot order longitude,
latitude, wave type, velocity kind, period and the leverage h_k.  The log gives the flagged columns, the median and range of the trace of R
over the others, and the depth below which the median R_jj falls under 0.1.  column_resolution_twin is the NumPy twin
(csrc/column_resolution.h is the arithmetic).

--radial: radial anisotropy.  The Rayleigh maps are explained by Vsv(z) and the Love maps by Vsh(z); both models start
as the input's MOD and are stepped together by columns_step_radial, 2 (nz - 1) unknowns per column, tied by --aniso G (default 0.2, in the
units of --damp): the weight of the penalty on the change of Vsh - Vsv, 0 for two independent inversions.  The input must list Rayleigh and
Love periods; --resolution is refused (the resolution of the coupled system is not computed).  The log gives per iteration the rms per wave
type and at the end the median and range of xi = (Vsh / Vsv)^2 over the nodes above the bottom depth of the interior columns that are not
flagged.  <input>DepthRadial.dat (write_radial / read_radial): longitude, latitude, depth, Vsv, Vsh, the Voigt average
sqrt((2 Vsv^2 + Vsh^2) / 3) and xi of every node.  <input>DepthRadialFit.dat (write_radial_fit / read_radial_fit): per column the data used
and the rms before the first and the last step per wave type, and the flag of the last step.  Depth.dat and DepthFit.dat are not written.
column_radial_twin is the NumPy twin (csrc/column_radial.h is the arithmetic).

--lateral W: the interior columns are stepped together by columns_step_lateral, tied by a penalty of weight W (in the
units of --damp) on the difference of the stepped model between neighbouring columns -- the noise of the maps no longer goes straight into
column-to-column speckle, and a column without a used datum (masked by --min-dws, or without roots) is carried by its neighbours in place
of keeping its starting values.  The coupled system is solved by preconditioned conjugate gradients to the relative tolerance
--lateral-tol T (default 1e-8) in at most --lateral-maxit N iterations (default 500).  --radial and --resolution are refused with it.
Depth.dat and DepthFit.dat keep their formats; the log adds per iteration the conjugate-gradient iterations, how they stopped (1: the
tolerance was met, 2: N was reached) and the number of columns without data that were carried.  Without the flag nothing changes.
column_lateral_twin is the NumPy twin (csrc/column_lateral.h is the arithmetic).

--radial --radial-lateral W [--radial-lateral-aniso A]: the radial step of all interior columns together, by
columns_step_radial_lateral (also at W = 0).  W is --lateral's weight on the differences of the stepped Vsv and of the stepped Vsh between
neighbouring columns, A (default W) the weight on the differences of the stepped anisotropy field Vsh - Vsv, so that xi can be smoothed more
strongly than the velocities; a column without a used datum gets its xi from its neighbours in place of staying at 1.  --lateral-tol and
--lateral-maxit apply.  --radial-lateral without --radial, --radial-lateral-aniso without --radial-lateral, and either with --lateral or
--resolution are refused (--lateral with --radial stays refused as it was).  DepthRadial.dat and DepthRadialFit.dat keep their formats; the
log adds per iteration what --lateral's adds.  column_radial_lateral_twin is the NumPy twin (csrc/column_radial_lateral.h is the arithmetic).

--radial --radial-resolution [--sigma S]: after the last radial step the runs are done once more on the final models
and columns_resolution_radial asks the 2 (nz - 1) x 2 (nz - 1) normal matrix of every column, with the loop's weights, --smooth, --damp and
--aniso, how far Vsv, Vsh and xi can be trusted.  <input>DepthRadialResolution.dat (write_radial_resolution / read_radial_resolution): per
node above the bottom depth longitude, latitude, depth; for Vsv and for Vsh R_jj, the vertical length sqrt(m2_own / m1_own) of the node's
point-spread function inside its model in km, the leak share m1_cross / (m1_own + m1_cross) of a spike's answer that lies in the other
model (0 where the denominator is 0) and sd = S sqrt(var); R_aniso = (R_vv + R_hh - R_hv - R_vh) / 2, the resolution of Vsh - Vsv at the
node; sd_diff = S sqrt(vard), the standard deviation of Vsh - Vsv; sd_xi = 2 xi S sqrt(var_v / Vsv^2 + var_h / Vsh^2 - 2 cov / (Vsv Vsh)).
S is --sigma in km/s or, by default, the rms before the last step.  <input>DepthRadialLeverage.dat (write_radial_leverage /
read_radial_leverage): DepthLeverage.dat's layout.  The log gives the flagged columns, the median and range of each block's trace, the
median leak share per block and how many unflagged nodes have |xi - 1| > 2 sd_xi.  --radial --resolution stays refused; the flag without
--radial and the flag with --radial-lateral (the resolution of the laterally coupled system is not computed) are refused.  Without the flag
nothing changes.  column_radial_resolution_twin is the NumPy twin (csrc/column_radial_resolution.h is the arithmetic).

--lateral W --lateral-resolution [--lateral-resolution-stride N] [--lateral-checkerboard NX,NY,NZ[,AMP]] [--sigma S]:
after the last coupled step the runs are done once more on the final model and columns_resolution_lateral solves, with the loop's weights,
--smooth, --damp, W, --lateral-tol and --lateral-maxit, the coupled system once per resolved unknown for its point-spread function and once
for its row of the averaging kernel -- every N-th unknown (default 1: all), all in one batched call.  <input>DepthLateralResolution.dat
(write_lateral_resolution / read_lateral_resolution): per resolved node longitude, latitude, depth, R_jj, the vertical length
sqrt(mz / m1) of its point-spread function in km, its lateral lengths sqrt(mx / m1) and sqrt(my / m1) in cells, the share own / m1 of the
function that stays in the node's own column, sd_unit = sqrt(var) and sd = S sd_unit, S by --resolution's rule.  With
--lateral-checkerboard a test model of blocks of NX x NY interior columns and NZ depths of alternating sign and amplitude AMP (default 0.1
km/s) is recovered in the same way; <input>DepthLateralChecker.dat (write_lateral_checker / read_lateral_checker): per interior node above
the bottom depth longitude, latitude, depth, the input and the recovered perturbation.  The log gives the median own share and lateral
length, the range of the conjugate-gradient iterations and every member that stopped at --lateral-maxit.  The flag needs --lateral and
refuses --radial; --resolution with --lateral stays refused.  Without the flag nothing changes.  column_lateral_resolution_twin is the NumPy
twin (csrc/column_lateral_resolution.h is the arithmetic).

--sample C,SWEEPS[,BURN] [--sample-step S] [--sample-spread P] [--sample-width W] [--sample-seed N] [--sample-temperature T] [--sigma S]
(DESIGN.md section 29): after the last step (and --resolution) the posterior of every interior column is sampled on the device by C
Metropolis chains of SWEEPS sweeps, started at the loop's result (chain 0) and scattered by up to P km/s about it (default 0.05); a sweep
proposes one node per chain, moved by up to S km/s (default 0.05), inside a box of half width W km/s about the start (default 0.5) and the
input's [minvel, maxvel].  The weights are 1 / sigma where --min-dws keeps a datum, sigma = --sigma or, by default, the rms before the last
step; --smooth is divided by sigma too, so that the prior keeps the step's balance between data and smoothing.  The first BURN sweeps
(default SWEEPS / 2) are left out of the moments.  <input>DepthPosterior.dat (write_posterior / read_posterior): per node above the bottom
depth longitude, latitude, depth, the start, the posterior mean, its standard deviation, the best model and R-hat, the Gelman-Rubin
convergence figure of the C chains.  <input>DepthPosteriorFit.dat (write_posterior_fit / read_posterior_fit): per column longitude,
latitude, the data used, phi of the start, the best phi + psi, the mean kept phi, the shares of the proposals that were accepted, fell
out of the box and lost a root, the chains put back to the start at the set-up, and the flag (2: no datum, never moved).  The log gives the
median and the worst R-hat and the share of the unknowns above 1.1.  --sample is refused with --radial and --lateral.  Without the flag
nothing changes.  column_sample_twin is the Python twin (csrc/column_sample.h is the arithmetic).

--sample-block EVERY [--sample-block-scale S], with --sample: every EVERY-th sweep proposes all nodes of a column at
once, along the column's linearised posterior -- delta = S L^-T D^-1/2 z, z uniform in [-1, 1], L D L^T the factor of the step's normal matrix
of the final model under the sampler's weights (columns_sample_shape, after the plan's runs with kernels once more).  S defaults to
2.38 sqrt(3 T / M) for the M unknowns of a column.  A column whose factorisation fails keeps the single-node proposal.  The log gives the
acceptance of the block and of the single-node proposals separately.  EVERY = 0 (the default) is the single-node sampler, bit for bit.

--sample-bins NB [--sample-quantiles P1,P2,...] [--sample-covariance], with --sample: in every kept sweep the device
counts each chain's value at each node in one of NB (2 to 256) equal bins of the node's box, and with --sample-covariance adds the products
of the offsets of a column's depths; the sampler's own figures keep their bits.  <input>DepthPosteriorQuantiles.dat (write_ / read_
posterior_quantiles): per node longitude, latitude, depth, the box, the mode and the quantiles of the levels (default 0.025, 0.16, 0.5,
0.84, 0.975), linear inside a bin.  <input>DepthPosteriorMarginals.dat (write_ / read_posterior_marginals): per node the NB counts pooled
over the chains.  <input>DepthPosteriorCorrelation.dat (write_ / read_posterior_correlation), with --sample-covariance: per column the
correlations between its depths.  The log gives the median width of the interval between the outermost levels and the median and largest
share of a node's states in the end bins of its box -- the sign of a posterior that leans on the prior box.  NB = 0 (the default) launches
nothing.  sample_marginal_bin, sample_marginal_mode and sample_marginal_quantile restate the rules in NumPy.

column_l, column_ltl and column_step_twin restate the regulariser and the step in NumPy for the tests (csrc/column_system.h is the arithmetic
the device runs).  Every precondition is checked before the library is loaded.  There is no CPU path.
"""
import argparse
import math
import os
import sys

import numpy as np

from . import io, maps
from .analyses.common import _lonlat

DEFAULT_ITERATIONS = 4
DEFAULT_SMOOTH = 0.5
DEFAULT_DAMP = 0.1
DEFAULT_DVMAX = 0.5
DEFAULT_ANISO = 0.2
DEFAULT_LATERAL_TOL = 1e-8
DEFAULT_LATERAL_MAXIT = 500

_F64 = lambda *names: tuple((n, "%.17g", "f64") for n in names)
DEPTH_TABLE = (True, _F64("lon", "lat", "depth", "vs"))
RESOLUTION_TABLE = (True, _F64("lon", "lat", "depth", "rjj", "length", "sd_unit", "sd"))
LEVERAGE_TABLE = (True, _F64("lon", "lat") + (("wave", "%d", "int"), ("kind", "%d", "int")) + _F64("period", "leverage"))
FIT_TABLE = (True, _F64("lon", "lat") + (("nused", "%d", "int"),) + _F64("rms_first", "rms_last") + (("flag", "%d", "int"),))
RADIAL_TABLE = (True, _F64("lon", "lat", "depth", "vsv", "vsh", "voigt", "xi"))
LATERAL_RESOLUTION_TABLE = (True, _F64("lon", "lat", "depth", "rjj", "length_z", "length_x", "length_y", "own", "sd_unit", "sd"))
LATERAL_CHECKER_TABLE = (True, _F64("lon", "lat", "depth", "input", "recovered"))
DEFAULT_CHECKER_AMP = 0.1
POSTERIOR_TABLE = (True, _F64("lon", "lat", "depth", "start", "mean", "sd", "best", "rhat"))
POSTERIOR_FIT_TABLE = (True, _F64("lon", "lat") + (("nused", "%d", "int"),) + _F64("phi_start", "phi_best", "phi_mean", "accepted", "out_of_box", "no_root") +
                       (("reseeded", "%d", "int"), ("flag", "%d", "int")))
DEFAULT_SAMPLE_STEP = 0.05
DEFAULT_SAMPLE_SPREAD = 0.05
DEFAULT_SAMPLE_WIDTH = 0.5
DEFAULT_SAMPLE_SEED = 1
DEFAULT_SAMPLE_TEMPERATURE = 1.0
DEFAULT_SAMPLE_QUANTILES = "0.025,0.16,0.5,0.84,0.975"
RADIAL_FIT_TABLE = (True, _F64("lon", "lat") + (("nused_r", "%d", "int"), ("nused_l", "%d", "int")) + _F64("rms_first_r", "rms_last_r", "rms_first_l", "rms_last_l") +
                    (("flag", "%d", "int"),))


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


# ---- the plan ----

def slot_plan(c):
    """[(wave type, velocity kind, periods, first slot)] of the wave types present, in the maps' period order Rc | Rg | Lc | Lg: one
    dispersion_run with kernels each, map_first = sen_slot = first slot"""
    out, first = [], 0
    for wave, kind, key in maps.WAVES:
        t = np.asarray(c[key], np.float64)
        if t.size:
            out.append((wave, kind, t, first))
            first += t.size
    return out


def maps_to_obs(rows, c):
    """The rows of <input>Maps.dat (maps.read_maps) as the step's observations: (obs, dws), both (nmaps, ny * nx) in get_maps' layout, fp32
    map values and fp64 DWS, 0 on the outer ring (which the step does not touch).  ValueError unless the file holds exactly the case's
    periods, in its order, with all interior vertices of each."""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    layer = nvx * nvz
    per = maps.period_list(c)
    if len(rows) != len(per) * layer:
        raise ValueError("depth: the maps file holds %d lines, %d periods of %d x %d interior vertices need %d" % (len(rows), len(per), nvx, nvz, len(per) * layer))
    obs = np.zeros((len(per), ny, nx), np.float32); dws = np.zeros((len(per), ny, nx))
    for m, (wave, kind, t) in enumerate(per):
        block = rows[m * layer:(m + 1) * layer]
        if any((r["wave"], r["kind"], r["period"]) != (wave, kind, t) for r in block):
            raise ValueError("depth: map %d of the maps file is not wave %d kind %d period %g of the input" % (m, wave, kind, t))
        obs[m, 1:-1, 1:-1] = np.array([r["c0"] for r in block]).reshape(nvz, nvx)
        dws[m, 1:-1, 1:-1] = np.array([r["dws"] for r in block]).reshape(nvz, nvx)
    return obs.reshape(len(per), ny * nx), dws.reshape(len(per), ny * nx)


def dws_weights(dws, min_dws):
    """the step's weights: 1, or 0 where the map's column DWS is below min_dws"""
    return np.where(np.asarray(dws, np.float64) < float(min_dws), 0.0, 1.0).astype(np.float32)


# ---- the loop ----

def check(iterations=None, smooth=None, damp=None, dvmax=None, min_dws=None, sigma=None, aniso=None, lateral=None, lateral_tol=None, lateral_maxit=None,
          radial_lateral=None, radial_lateral_aniso=None):
    """the driver's preconditions, checked before the library is loaded (ValueError); the lateral ones come after the others"""
    if iterations is not None and iterations < 1:
        raise ValueError("--iterations must be at least 1, not %r" % (iterations,))
    for name, v in (("--smooth", smooth), ("--min-dws", min_dws), ("--aniso", aniso)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    for name, v in (("--damp", damp), ("--dvmax", dvmax), ("--sigma", sigma)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, not %r" % (name, v))
    if lateral is not None and not (np.isfinite(lateral) and lateral >= 0):
        raise ValueError("--lateral must be finite and >= 0, not %r" % (lateral,))
    for name, v in (("--radial-lateral", radial_lateral), ("--radial-lateral-aniso", radial_lateral_aniso)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    if lateral_tol is not None and not (np.isfinite(lateral_tol) and lateral_tol > 0):
        raise ValueError("--lateral-tol must be finite and > 0, not %r" % (lateral_tol,))
    if lateral_maxit is not None and lateral_maxit < 1:
        raise ValueError("--lateral-maxit must be at least 1, not %r" % (lateral_maxit,))


def rms_of(chi2, nused):
    """sqrt(sum chi2 / sum nused), 0 without data"""
    n = int(np.sum(nused))
    return float(np.sqrt(np.sum(np.asarray(chi2, np.float64)) / n)) if n > 0 else 0.0


def check_lateral(radial=False, resolution=False):
    """what --lateral asks of the other flags, before the library is loaded (ValueError)"""
    if radial or resolution:
        raise ValueError("--lateral and %s exclude each other: the lateral coupling of the %s is not computed" %
                         (("--radial", "radial step") if radial else ("--resolution", "resolution")))


def check_flags(iterations, smooth, damp, dvmax, min_dws, sigma, aniso, radial, resolution, lateral, lateral_tol, lateral_maxit, radial_lateral, radial_lateral_aniso,
                radial_resolution=False, lateral_resolution=False, lateral_resolution_stride=1, lateral_checkerboard=None):
    """every precondition on the flags, in the order run() and main() both refuse in (ValueError), before the library is loaded.  aniso None:
    not looked at; --lateral-tol and --lateral-maxit are looked at only with a coupling; --radial-resolution's come after the others, then
    --lateral-resolution's.  Returns the parsed --lateral-checkerboard, or None."""
    with_cg = lateral is not None or radial_lateral is not None
    check(iterations, smooth, damp, dvmax, min_dws, sigma, aniso, lateral, lateral_tol if with_cg else None, lateral_maxit if with_cg else None, radial_lateral,
          radial_lateral_aniso)
    if lateral is not None:
        check_lateral(radial, resolution)
    if radial:
        check_radial(None, resolution)
    check_radial_lateral(radial_lateral, radial_lateral_aniso, radial, lateral, resolution)
    check_radial_resolution(radial_resolution, radial, radial_lateral)
    return check_lateral_resolution(lateral_resolution, lateral_resolution_stride, lateral_checkerboard, lateral, radial)


def _iterate(eng, plan, iterations, step, entry, log, coupling):
    """the loop of iterate and iterate_radial: per iteration the runs of plan, out = step(), h = entry(iteration, out) (the history's dict; it
    logs the iteration's first line), and with coupling (the words in the second line's brackets; None: no coupling) itn, istop and carried"""
    history, steps = [], []
    for it in range(1, iterations + 1):
        for wave, kind, t, first in plan:
            eng.dispersion_run(wave, kind, t, True, first, first)
        out = step()
        h = entry(it, out)
        if coupling is not None:
            h.update(itn=out["itn"], istop=out["istop"], carried=out["carried"])
            log(" depth iteration %d (%s): %d conjugate-gradient iterations, istop %d (%s), %d columns without data carried by their neighbours" %
                (it, coupling, h["itn"], h["istop"], "the tolerance was met" if h["istop"] == 1 else "--lateral-maxit was reached", h["carried"]))
        history.append(h)
        steps.append(out)
    return dict(history=history, steps=steps)


def iterate(eng, plan, obs, wt, iterations, smooth, damp, dvmax, minvel, maxvel, log=print, lateral=None, lateral_tol=DEFAULT_LATERAL_TOL,
            lateral_maxit=DEFAULT_LATERAL_MAXIT):
    """The loop on an engine whose dispersion stage holds the starting model (dispersion_begin with as many maps as kernel slots): per
    iteration one dispersion_run with kernels per entry of plan (slot_plan), then columns_step -- or, with lateral (not None),
    columns_step_lateral.  Returns dict(history: one dict per iteration {iteration, nused, chi2, rms (before the step), flagged1, flagged2;
    with lateral also itn, istop, carried (the step's own count)}, steps: the step's result per iteration)."""
    if lateral is None:
        step = lambda: eng.columns_step(obs, wt, smooth, damp, dvmax, minvel, maxvel)
    else:
        step = lambda: eng.columns_step_lateral(obs, wt, smooth, damp, lateral, dvmax, minvel, maxvel, lateral_tol, lateral_maxit)

    def entry(it, out):
        h = dict(iteration=it, nused=int(out["nused"].sum()), chi2=float(out["chi2"].sum()), rms=rms_of(out["chi2"], out["nused"]),
                 flagged1=int((out["flag"] == 1).sum()), flagged2=int((out["flag"] == 2).sum()))
        log(" depth iteration %d: %d data used, rms %.6f km/s before the step, %d columns flagged (%d not positive definite, %d without data)" %
            (it, h["nused"], h["rms"], h["flagged1"] + h["flagged2"], h["flagged1"], h["flagged2"]))
        return h

    return _iterate(eng, plan, iterations, step, entry, log, None if lateral is None else "lateral %g" % lateral)


# ---- the files ----

def write_depth(path, c, vels):
    """<input>Depth.dat: vels (nz, ny, nx), every node: depth slowest, then j, then i"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.asarray(vels, np.float64).reshape(nz, ny, nx)
    rows = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                rows.append(dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]), vs=v[k, j, i]))
    io.write_table(path, DEPTH_TABLE, rows)


def read_depth(path):
    return io.read_table(path, DEPTH_TABLE)


def write_fit(path, c, first, last):
    """<input>DepthFit.dat: first / last = columns_step's results of the first and the last iteration; one line per column, j then i"""
    nx, ny = c["nx"], c["ny"]
    col_rms = lambda s: np.sqrt(np.divide(s["chi2"], s["nused"], out=np.zeros(nx * ny), where=s["nused"] > 0))
    r0, r1 = col_rms(first), col_rms(last)
    rows = []
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            q = j * nx + i
            rows.append(dict(lon=float(lon), lat=float(lat), nused=int(last["nused"][q]), rms_first=float(r0[q]), rms_last=float(r1[q]), flag=int(last["flag"][q])))
    io.write_table(path, FIT_TABLE, rows)


def read_fit(path):
    return io.read_table(path, FIT_TABLE)


def psf_length(m1, m2):
    """the vertical length sqrt(m2 / m1) of the point-spread functions, 0 where m1 = 0"""
    m1 = np.asarray(m1, np.float64); m2 = np.asarray(m2, np.float64)
    return np.sqrt(np.divide(m2, m1, out=np.zeros(m1.shape), where=m1 > 0))


def write_resolution(path, c, measures, sigma):
    """<input>DepthResolution.dat: measures (4, nz - 1, ny * nx) of columns_resolution, every node above the bottom depth: depth slowest,
    then j, then i; sigma: the data's standard deviation S in km/s"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    m = np.asarray(measures, np.float64).reshape(4, nz - 1, ny, nx)
    length = psf_length(m[1], m[2]); sd_unit = np.sqrt(m[3])
    rows = []
    for k in range(nz - 1):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                rows.append(dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]), rjj=m[0, k, j, i], length=length[k, j, i], sd_unit=sd_unit[k, j, i],
                                 sd=float(sigma) * sd_unit[k, j, i]))
    io.write_table(path, RESOLUTION_TABLE, rows)


def read_resolution(path):
    return io.read_table(path, RESOLUTION_TABLE)


def write_leverage(path, c, leverage):
    """<input>DepthLeverage.dat: leverage (nmaps, ny * nx) of columns_resolution; one line per column (j, then i) and period in slot order"""
    nx, ny = c["nx"], c["ny"]
    per = maps.period_list(c)
    h = np.asarray(leverage, np.float64).reshape(len(per), ny, nx)
    rows = []
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            for k, (wave, kind, t) in enumerate(per):
                rows.append(dict(lon=float(lon), lat=float(lat), wave=int(wave), kind=int(kind), period=float(t), leverage=h[k, j, i]))
    io.write_table(path, LEVERAGE_TABLE, rows)


def read_leverage(path):
    return io.read_table(path, LEVERAGE_TABLE)


def resolution_summary(c, res):
    """what the log says of columns_resolution's result: dict(flagged1, flagged2, columns (interior and not flagged), trace (median, min, max)
    over them, depth: the shallowest depth from which the median R_jj over them stays under 0.1, or None)"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    inner = np.zeros((ny, nx), bool); inner[1:-1, 1:-1] = True
    flag = np.asarray(res["flag"]).reshape(ny * nx)
    ok = inner.ravel() & (flag == 0)
    out = dict(flagged1=int((flag == 1).sum()), flagged2=int(((flag == 2) & inner.ravel()).sum()), columns=int(ok.sum()), trace=None, depth=None)
    if ok.any():
        tr = np.asarray(res["trace"])[ok]
        out["trace"] = (float(np.median(tr)), float(tr.min()), float(tr.max()))
        med = np.median(np.asarray(res["measures"])[0][:, ok], axis=1)
        below = med < 0.1
        k = nz - 1
        while k > 0 and below[k - 1]:
            k -= 1
        out["depth"] = float(c["depz"][k]) if k < nz - 1 else None
    return out


def resolve(eng, c, plan, obs, wt, smooth, damp, sigma, out_dir, log=print):
    """--resolution on an engine whose stage holds the final model: the runs of plan once more, columns_resolution, the two files, the log.
    Returns dict(resolution: the call's result, sigma, summary, resolution_path, leverage_path)."""
    for wave, kind, t, first in plan:
        eng.dispersion_run(wave, kind, t, True, first, first)
    res = eng.columns_resolution(obs, wt, smooth, damp)
    rpath = os.path.join(out_dir, "DSurfTomo.inDepthResolution.dat")
    lpath = os.path.join(out_dir, "DSurfTomo.inDepthLeverage.dat")
    write_resolution(rpath, c, res["measures"], sigma)
    write_leverage(lpath, c, res["leverage"])
    sm = resolution_summary(c, res)
    log(" depth resolution: %d columns resolved, %d flagged (%d not positive definite, %d without data)" %
        (sm["columns"], sm["flagged1"] + sm["flagged2"], sm["flagged1"], sm["flagged2"]))
    if sm["trace"] is not None:
        log(" depth resolution: trace of R per column median %.4f, range %.4f to %.4f, of %d unknowns; the median R_jj %s" %
            (sm["trace"] + (c["nz"] - 1, "stays under 0.1 from %g km down" % sm["depth"] if sm["depth"] is not None else "is 0.1 or more at the deepest unknown")))
    log(" depth resolution: written to %s (sd for a data standard deviation of %.6f km/s), the leverages to %s" % (rpath, sigma, lpath))
    return dict(resolution=res, sigma=float(sigma), summary=sm, resolution_path=rpath, leverage_path=lpath)


# ---- the Monte-Carlo depth inversion: the driver's side ----

def parse_sample(text):
    """--sample C,SWEEPS[,BURN]: (chains, sweeps, burn) -- at least one chain and one sweep, 0 <= BURN <= SWEEPS, BURN by default SWEEPS // 2"""
    parts = str(text).split(",")
    try:
        vals = [int(x) for x in parts]
    except ValueError:
        vals = None
    if vals is None or len(vals) not in (2, 3):
        raise ValueError("--sample takes C,SWEEPS[,BURN] in whole numbers, not %r" % (text,))
    chains, sweeps = vals[:2]
    burn = vals[2] if len(vals) == 3 else sweeps // 2
    if chains < 1 or sweeps < 1 or burn < 0 or burn > sweeps:
        raise ValueError("--sample needs C >= 1, SWEEPS >= 1 and 0 <= BURN <= SWEEPS, not %r" % (text,))
    return chains, sweeps, burn


def check_sample(sample=None, radial=False, lateral=None, step=None, spread=None, width=None, temperature=None, seed=None, block=0, block_scale=None):
    """what --sample, --sample-block and --sample-block-scale ask of the other flags, before the library is loaded (ValueError).  Returns
    parse_sample's tuple, or None."""
    if block is not None and block < 0:
        raise ValueError("--sample-block must be >= 0, not %r" % (block,))
    if block_scale is not None and not (np.isfinite(block_scale) and block_scale > 0):
        raise ValueError("--sample-block-scale must be finite and > 0, not %r" % (block_scale,))
    if sample is None:
        if block:
            raise ValueError("--sample-block needs --sample: the block proposals are the sampler's")
        return None
    if radial or lateral is not None:
        raise ValueError("--sample and %s exclude each other: the %s is not sampled" % (("--radial", "radial model") if radial else ("--lateral", "laterally coupled model")))
    parsed = parse_sample(sample)
    for name, v in (("--sample-step", step), ("--sample-width", width), ("--sample-temperature", temperature)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, not %r" % (name, v))
    if spread is not None and not (np.isfinite(spread) and spread >= 0):
        raise ValueError("--sample-spread must be finite and >= 0, not %r" % (spread,))
    if seed is not None and seed < 0:
        raise ValueError("--sample-seed must be >= 0, not %r" % (seed,))
    return parsed


def sample_scaling(wt, smooth, sigma, shape):
    """The sampler's weights and prior weight for a data standard deviation sigma: (wt / sigma (1 / sigma where wt is None), smooth / sigma)
    -- phi becomes the chi-square of the data and the prior keeps the balance between data and smoothing the step had at unit weights."""
    sigma = float(sigma)
    w = np.ones(shape, np.float32) if wt is None else np.asarray(wt, np.float32).reshape(shape)
    return (w.astype(np.float64) / sigma).astype(np.float32), float(smooth) / sigma


def _rate(count, total):
    return np.divide(np.asarray(count, np.float64), total, out=np.zeros(np.shape(count)), where=np.asarray(total) > 0)


def write_posterior(path, c, start, res):
    """<input>DepthPosterior.dat: start (nz, ny, nx) and columns_sample_fetch's result; every node above the bottom depth: depth slowest, then
    j, then i.  Where no sweep was kept (the ring, a column without data) mean and best are the start, sd 0 and rhat 1."""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    M = nz - 1
    v0 = np.asarray(start, np.float64).reshape(nz, ny, nx)[:M]
    kept = (np.asarray(res["nkept"]).reshape(ny, nx) > 0)[None]
    grid = lambda a: np.asarray(a, np.float64).reshape(M, ny, nx)
    mean = np.where(kept, grid(res["mean"]), v0); best = np.where(kept, grid(res["best"]), v0)
    sd = np.where(kept, grid(sample_sd(res["var"])), 0.0)
    rhat = grid(sample_rhat(res["W"], res["B"], np.asarray(res["nkept"])[None]))
    rows = []
    for k in range(M):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                rows.append(dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]), start=v0[k, j, i], mean=mean[k, j, i], sd=sd[k, j, i], best=best[k, j, i],
                                 rhat=rhat[k, j, i]))
    io.write_table(path, POSTERIOR_TABLE, rows)


def read_posterior(path):
    return io.read_table(path, POSTERIOR_TABLE)


def write_posterior_fit(path, c, res):
    """<input>DepthPosteriorFit.dat: per column (j, then i) the data used, phi of the start, the best phi + psi, the mean kept phi,
    the shares of the proposals (chains x sweeps) that were accepted, fell out of the box, lost a root; the chains put back; the flag"""
    nx, ny = c["nx"], c["ny"]
    total = np.asarray(res["accepted"], np.float64) + np.asarray(res["rejected"], np.float64)
    acc, oob, noroot = (_rate(res[n], total) for n in ("accepted", "out_of_box", "no_root"))
    rows = []
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            q = j * nx + i
            rows.append(dict(lon=float(lon), lat=float(lat), nused=int(res["nused"][q]), phi_start=float(res["phi_start"][q]), phi_best=float(res["best_energy"][q]),
                             phi_mean=float(res["mean_phi"][q]), accepted=float(acc[q]), out_of_box=float(oob[q]), no_root=float(noroot[q]),
                             reseeded=int(res["reseeded"][q]), flag=int(res["flag"][q])))
    io.write_table(path, POSTERIOR_FIT_TABLE, rows)


def read_posterior_fit(path):
    return io.read_table(path, POSTERIOR_FIT_TABLE)


def parse_quantiles(text):
    """--sample-quantiles P1,P2,...: a tuple of 1 to 16 probabilities, each finite and inside (0, 1) (ValueError)"""
    try:
        vals = tuple(float(x) for x in str(text).split(","))
    except ValueError:
        vals = ()
    if not 1 <= len(vals) <= 16 or not all(np.isfinite(p) and 0.0 < p < 1.0 for p in vals):
        raise ValueError("--sample-quantiles takes 1 to 16 probabilities inside (0, 1) separated by commas, not %r" % (text,))
    return vals


def check_marginals(sample=None, bins=0, quantiles=DEFAULT_SAMPLE_QUANTILES, covariance=False):
    """what --sample-bins, --sample-quantiles and --sample-covariance ask of the other flags, before the library is loaded (ValueError).
    Returns None while the marginals are off, else (bins, the levels, covariance)."""
    if bins is None or int(bins) != bins or bins < 0 or bins == 1 or bins > 256:
        raise ValueError("--sample-bins must be 0 (off) or 2 to 256, not %r" % (bins,))
    given = quantiles is not None and str(quantiles) != DEFAULT_SAMPLE_QUANTILES
    levels = parse_quantiles(DEFAULT_SAMPLE_QUANTILES if quantiles is None else quantiles)
    if sample is None and (bins or given or covariance):
        raise ValueError("%s needs --sample: the marginals are the sampler's" % ("--sample-bins" if bins else "--sample-quantiles" if given else "--sample-covariance"))
    if not bins and (given or covariance):
        raise ValueError("%s needs --sample-bins: the marginals are off without it" % ("--sample-quantiles" if given else "--sample-covariance"))
    return (int(bins), levels, bool(covariance)) if bins else None


def posterior_quantiles_table(levels):
    return (True, _F64("lon", "lat", "depth", "lo", "hi", "mode") + _F64(*("q%.17g" % p for p in levels)))


def posterior_marginals_table(nbins):
    return (True, _F64("lon", "lat", "depth") + tuple(("n%d" % b, "%d", "int") for b in range(nbins)))


def posterior_correlation_table(M):
    return (True, _F64("lon", "lat") + _F64(*("r%d_%d" % (i, j) for i in range(M) for j in range(M))))


def _header_names(path):
    with open(path) as fh:
        return fh.readline().lstrip("#").split()


def _node_rows(c, M):
    """lon, lat, depth of every node above the bottom depth: depth slowest, then j, then i -- with its place (k, j * nx + i)"""
    nx, ny = c["nx"], c["ny"]
    for k in range(M):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                yield k, j * nx + i, dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]))


def write_posterior_quantiles(path, c, start, width, levels, mg):
    """<input>DepthPosteriorQuantiles.dat: per node above the bottom depth (depth slowest, then j, then i) longitude, latitude, depth, the
    box [lo, hi] of the node, the mode and the quantile of every level of columns_sample_marginals_fetch's result mg (zeros where no sweep
    was kept)"""
    M = c["nz"] - 1
    lo, hi = sample_box(np.asarray(start, np.float32).reshape(c["nz"], -1)[:M], width, float(c["minvel"]), float(c["maxvel"]))
    rows = []
    for k, q, row in _node_rows(c, M):
        row.update(lo=float(lo[k, q]), hi=float(hi[k, q]), mode=float(mg["mode"][k, q]))
        row.update(("q%.17g" % p, float(mg["quantiles"][n, k, q])) for n, p in enumerate(levels))
        rows.append(row)
    io.write_table(path, posterior_quantiles_table(levels), rows)


def read_posterior_quantiles(path):
    """the rows of write_posterior_quantiles; the levels are read from the header's names"""
    return io.read_table(path, posterior_quantiles_table([float(n[1:]) for n in _header_names(path)[6:]]))


def write_posterior_marginals(path, c, hist):
    """<input>DepthPosteriorMarginals.dat: per node (as the quantiles' file) longitude, latitude, depth and the nbins pooled counts n0 ..,
    bin b the b-th of the nbins equal parts of the node's box"""
    hist = np.asarray(hist)
    rows = []
    for k, q, row in _node_rows(c, c["nz"] - 1):
        row.update(("n%d" % b, int(hist[b, k, q])) for b in range(hist.shape[0]))
        rows.append(row)
    io.write_table(path, posterior_marginals_table(hist.shape[0]), rows)


def read_posterior_marginals(path):
    return io.read_table(path, posterior_marginals_table(len(_header_names(path)) - 3))


def sample_correlation(cov, M):
    """the M x M correlation of every column from the packed lower triangle cov (M (M + 1) / 2, ncol): cov_ij / sqrt(cov_ii cov_jj), 0
    where a variance is not positive.  Returns (M, M, ncol)."""
    cov = np.asarray(cov, np.float64)
    full = np.zeros((M, M, cov.shape[1]))
    for i in range(M):
        for j in range(i + 1):
            full[i, j] = full[j, i] = cov[i * (i + 1) // 2 + j]
    var = np.stack([full[i, i] for i in range(M)])
    den = var[:, None] * var[None, :]
    ok = (var[:, None] > 0) & (var[None, :] > 0)
    return np.divide(full, np.sqrt(np.where(ok, den, 1.0)), out=np.zeros(full.shape), where=ok)


def write_posterior_correlation(path, c, cov):
    """<input>DepthPosteriorCorrelation.dat: per column (j, then i) longitude, latitude and the (nz - 1)^2 correlations r<i>_<j> between its
    depths, row by row"""
    nx, ny, M = c["nx"], c["ny"], c["nz"] - 1
    corr = sample_correlation(cov, M)
    rows = []
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            row = dict(lon=float(lon), lat=float(lat))
            row.update(("r%d_%d" % (a, b), float(corr[a, b, j * nx + i])) for a in range(M) for b in range(M))
            rows.append(row)
    io.write_table(path, posterior_correlation_table(M), rows)


def read_posterior_correlation(path):
    return io.read_table(path, posterior_correlation_table(int(round(math.sqrt(len(_header_names(path)) - 2)))))


def marginals_summary(levels, mg, nkept):
    """what the log says of the marginals: dict(nodes, width: the median over the nodes with a kept sweep of the distance between the
    quantiles of the smallest and the largest level (None with fewer than two levels), end_median, end_max: the median and the largest
    share of a node's counts in the two end bins), or None without a kept sweep"""
    kept = np.asarray(nkept) > 0
    if not kept.any():
        return None
    h = np.asarray(mg["hist"], np.float64)[:, :, kept]
    share = (h[0] + h[-1]) / h.sum(axis=0)
    width = None
    if len(levels) >= 2:
        q = np.asarray(mg["quantiles"])[:, :, kept]
        width = float(np.median(q[int(np.argmax(levels))] - q[int(np.argmin(levels))]))
    return dict(nodes=int(share.size), width=width, end_median=float(np.median(share)), end_max=float(share.max()))


def rhat_summary(res):
    """what the log says of the convergence: dict(unknowns, median, worst, share of them above 1.1) over the unknowns of the columns with a kept
    sweep, or None without one"""
    kept = np.asarray(res["nkept"]) > 0
    if not kept.any():
        return None
    r = sample_rhat(res["W"], res["B"], np.asarray(res["nkept"])[None])[:, kept]
    return dict(unknowns=int(r.size), median=float(np.median(r)), worst=float(r.max()), above=float((r > 1.1).mean()))


def run_sample(eng, c, plan, start, obs, wt, smooth, sigma, sample, out_dir, step=DEFAULT_SAMPLE_STEP, spread=DEFAULT_SAMPLE_SPREAD, width=DEFAULT_SAMPLE_WIDTH,
               seed=DEFAULT_SAMPLE_SEED, temperature=DEFAULT_SAMPLE_TEMPERATURE, log=print, block_every=0, block_scale=None, damp=DEFAULT_DAMP, marginals=None):
    """--sample from the model start (nz, ny, nx): columns_sample_begin with the weights 1 / sigma where wt keeps a datum and smooth / sigma,
    the sweeps, the two files, the log.  With block_every > 0 (--sample-block), on an engine whose stage holds start: first the runs of plan
    once more with kernels and columns_sample_shape with the same weights and prior weight and damp / sigma, then, after the begin,
    columns_sample_blocks(block_every, block_scale; None: sample_block_scale(nz - 1, temperature)).  Returns dict(posterior:
    columns_sample_fetch's result, sample_sigma, rhat, posterior_path, posterior_fit_path; with block_every > 0 also block: dict(every, scale,
    flagged: the columns whose shape was flagged, proposed, accepted, out_of_box: the block proposals summed over chains and columns)).
    With marginals = (bins, levels, covariance) (check_marginals'; --sample-bins): columns_sample_marginals(bins, covariance) after the
    begin and the blocks, before the sweeps; after them columns_sample_marginals_fetch(levels), DepthPosteriorQuantiles.dat,
    DepthPosteriorMarginals.dat and, with the covariance, DepthPosteriorCorrelation.dat; the result gains marginals: the fetch's result,
    marginals_summary: its figures in the log, quantiles_path, marginals_path and correlation_path (None without the covariance)."""
    chains, sweeps, burn = sample
    w, lam = sample_scaling(wt, smooth, sigma, np.shape(obs))
    block = None
    if block_every > 0:
        for wave, kind, t, first in plan:
            eng.dispersion_run(wave, kind, t, True, first, first)
        shape = eng.columns_sample_shape(obs, w, lam, float(damp) / float(sigma))
        scale = sample_block_scale(c["nz"] - 1, temperature) if block_scale is None else float(block_scale)
        block = dict(every=int(block_every), scale=scale, flagged=int((shape["flag"] == 1).sum()))
    eng.columns_sample_begin(start, c["depz"], c["minthk"], plan, obs, w, chains, lam, step, spread, width, temperature, float(c["minvel"]), float(c["maxvel"]), seed, burn)
    if block is not None:
        eng.columns_sample_blocks(block["every"], block["scale"])
    if marginals is not None:
        eng.columns_sample_marginals(marginals[0], marginals[2])
    eng.columns_sample_run(sweeps)
    res = eng.columns_sample_fetch()
    mg = eng.columns_sample_marginals_fetch(marginals[1]) if marginals is not None else None
    if block is not None:
        bc = eng.columns_sample_block_state()["block_counters"]
        block.update(proposed=int(bc[0].sum()), accepted=int(bc[1].sum()), out_of_box=int(bc[2].sum()))
    ppath = os.path.join(out_dir, "DSurfTomo.inDepthPosterior.dat")
    fpath = os.path.join(out_dir, "DSurfTomo.inDepthPosteriorFit.dat")
    write_posterior(ppath, c, start, res)
    write_posterior_fit(fpath, c, res)
    moved = res["nkept"] > 0
    tried = float(res["accepted"].sum() + res["rejected"].sum())
    log(" depth sample: %d chains x %d sweeps (%d kept) on %d columns, data standard deviation %.6f km/s, %d columns without data, %d chains put back at the set-up" %
        (chains, sweeps, sweeps - burn, int(moved.sum()), sigma, int((res["flag"] == 2).sum()), int(res["reseeded"].sum())))
    if tried > 0:
        log(" depth sample: %.1f %% of the proposals accepted, %.1f %% out of the box, %.1f %% without a root" %
            tuple(100.0 * float(res[n].sum()) / tried for n in ("accepted", "out_of_box", "no_root")))
    if block is not None:
        single = tried - block["proposed"]
        log(" depth sample: block proposals of scale %.4f every %s, %d columns with a flagged shape propose single nodes" %
            (block["scale"], "sweep" if block["every"] == 1 else "%d sweeps" % block["every"], block["flagged"]))
        log(" depth sample: %.1f %% of %d block proposals accepted (%.1f %% out of the box), %.1f %% of %d single-node proposals" %
            (100.0 * float(_rate(block["accepted"], block["proposed"])), block["proposed"], 100.0 * float(_rate(block["out_of_box"], block["proposed"])),
             100.0 * float(_rate(float(res["accepted"].sum()) - block["accepted"], single)), int(single)))
    if moved.any():
        log(" depth sample: phi per column from %.4g at the start to %.4g on average over the kept sweeps (median over the columns)" %
            (float(np.median(res["phi_start"][moved])), float(np.median(res["mean_phi"][moved]))))
    sm = rhat_summary(res)
    if sm is not None:
        log(" depth sample: R-hat of %d unknowns median %.4f, worst %.4f, %.1f %% above 1.1" % (sm["unknowns"], sm["median"], sm["worst"], 100.0 * sm["above"]))
    log(" depth sample: the posterior written to %s, the fit of the columns to %s" % (ppath, fpath))
    out = dict(posterior=res, sample_sigma=float(sigma), rhat=sm, posterior_path=ppath, posterior_fit_path=fpath)
    if mg is not None:
        bins, levels, covariance = marginals
        qpath = os.path.join(out_dir, "DSurfTomo.inDepthPosteriorQuantiles.dat")
        mpath = os.path.join(out_dir, "DSurfTomo.inDepthPosteriorMarginals.dat")
        cpath = os.path.join(out_dir, "DSurfTomo.inDepthPosteriorCorrelation.dat") if covariance else None
        write_posterior_quantiles(qpath, c, start, width, levels, mg)
        write_posterior_marginals(mpath, c, mg["hist"])
        if covariance:
            write_posterior_correlation(cpath, c, mg["cov"])
        ms = marginals_summary(levels, mg, res["nkept"])
        if ms is not None:
            if ms["width"] is not None:
                log(" depth sample: marginals of %d nodes in %d bins; the %g to %g interval is %.4f km/s wide (median over the nodes)" %
                    (ms["nodes"], bins, min(levels), max(levels), ms["width"]))
            log(" depth sample: share of a node's kept states in the end bins of its box: median %.2f %%, largest %.2f %%" % (100.0 * ms["end_median"], 100.0 * ms["end_max"]))
        log(" depth sample: the quantiles written to %s, the marginals to %s%s" % (qpath, mpath, ", the correlations of the depths to %s" % cpath if covariance else ""))
        out.update(marginals=mg, marginals_summary=ms, quantiles_path=qpath, marginals_path=mpath, correlation_path=cpath)
    if block is not None:
        out["block"] = block
    return out


# ---- the resolution of the laterally coupled step ----

def parse_checkerboard(text):
    """--lateral-checkerboard NX,NY,NZ[,AMP]: (nx, ny, nz, amp) -- block sizes in interior columns and depths, at least 1; AMP in km/s, finite
    and not 0, default DEFAULT_CHECKER_AMP (ValueError)"""
    parts = str(text).split(",")
    try:
        if len(parts) not in (3, 4):
            raise ValueError
        nx, ny, nz = (int(p) for p in parts[:3])
        amp = float(parts[3]) if len(parts) == 4 else DEFAULT_CHECKER_AMP
    except ValueError:
        raise ValueError("--lateral-checkerboard takes NX,NY,NZ[,AMP], not %r" % (text,)) from None
    if min(nx, ny, nz) < 1 or not np.isfinite(amp) or amp == 0:
        raise ValueError("--lateral-checkerboard: the blocks must be at least 1 x 1 x 1 and AMP finite and not 0, not %r" % (text,))
    return nx, ny, nz, amp


def check_lateral_resolution(lateral_resolution=False, stride=1, checkerboard=None, lateral=None, radial=False):
    """what --lateral-resolution and its companions ask of the other flags, before the library is loaded (ValueError).  Returns the parsed
    checkerboard, or None."""
    if not lateral_resolution:
        if stride != 1 or checkerboard is not None:
            raise ValueError("%s needs --lateral-resolution" % ("--lateral-resolution-stride" if stride != 1 else "--lateral-checkerboard"))
        return None
    if radial:
        raise ValueError("--lateral-resolution and --radial exclude each other: the resolution of the laterally coupled radial system is not computed")
    if lateral is None:
        raise ValueError("--lateral-resolution needs --lateral: it is the resolution of that coupled step (--resolution is that of the columns alone)")
    if stride < 1:
        raise ValueError("--lateral-resolution-stride must be at least 1, not %r" % (stride,))
    return None if checkerboard is None else parse_checkerboard(checkerboard)


def checkerboard_model(nvx, nvy, M, spec):
    """blocks of spec = (nx, ny, nz, amp): (M, nvy * nvx), +amp where the block indices add up to an even number"""
    bx, by, bz, amp = spec
    l = np.arange(M)[:, None, None] // bz; j = np.arange(nvy)[None, :, None] // by; i = np.arange(nvx)[None, None, :] // bx
    return (amp * np.where((l + j + i) % 2 == 0, 1.0, -1.0)).reshape(M, nvy * nvx)


def _ratio(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return np.divide(a, b, out=np.zeros(a.shape), where=b > 0)


def lateral_resolution_columns(index, psf, unit, sigma):
    """The node figures of DepthLateralResolution.dat: index (n) the resolved unknowns, psf and unit (n, 7) the measures of their members of
    kind 0 and of kind 1 (val, m1, mz, mx, my, own, var).  Returns dict(rjj, length_z, length_x, length_y, own, sd_unit, sd), each (n); a
    length and the share are 0 where m1 = 0."""
    psf = np.asarray(psf, np.float64).reshape(-1, 7); unit = np.asarray(unit, np.float64).reshape(-1, 7)
    sd_unit = np.sqrt(np.maximum(unit[:, 6], 0.0))
    return dict(rjj=psf[:, 0].copy(), length_z=np.sqrt(_ratio(psf[:, 2], psf[:, 1])), length_x=np.sqrt(_ratio(psf[:, 3], psf[:, 1])),
                length_y=np.sqrt(_ratio(psf[:, 4], psf[:, 1])), own=_ratio(psf[:, 5], psf[:, 1]), sd_unit=sd_unit, sd=float(sigma) * sd_unit)


def _interior_node(c, unknown):
    """(lon, lat, depth) of unknown = b (nz - 1) + l of interior column b"""
    M, nvx = c["nz"] - 1, c["nx"] - 2
    b, l = divmod(int(unknown), M)
    lon, lat = _lonlat(c, b % nvx, b // nvx)
    return float(lon), float(lat), float(c["depz"][l])


def write_lateral_resolution(path, c, index, columns):
    """<input>DepthLateralResolution.dat: one line per resolved unknown in index's order; columns: lateral_resolution_columns' dict"""
    rows = []
    for q, unknown in enumerate(index):
        lon, lat, dep = _interior_node(c, unknown)
        rows.append(dict(lon=lon, lat=lat, depth=dep, **{name: float(columns[name][q]) for name, _, _ in LATERAL_RESOLUTION_TABLE[1][3:]}))
    io.write_table(path, LATERAL_RESOLUTION_TABLE, rows)


def read_lateral_resolution(path):
    return io.read_table(path, LATERAL_RESOLUTION_TABLE)


def write_lateral_checker(path, c, model, recovered):
    """<input>DepthLateralChecker.dat: model and recovered (nz - 1, interior columns), every interior node above the bottom depth: depth
    slowest, then the interior columns in their order"""
    M, nint = c["nz"] - 1, (c["nx"] - 2) * (c["ny"] - 2)
    m = np.asarray(model, np.float64).reshape(M, nint); r = np.asarray(recovered, np.float64).reshape(M, nint)
    rows = []
    for l in range(M):
        for b in range(nint):
            lon, lat, dep = _interior_node(c, b * M + l)
            rows.append(dict(lon=lon, lat=lat, depth=dep, input=m[l, b], recovered=r[l, b]))
    io.write_table(path, LATERAL_CHECKER_TABLE, rows)


def read_lateral_checker(path):
    return io.read_table(path, LATERAL_CHECKER_TABLE)


def lateral_resolution_log(columns, psf, res):
    """the log's lines: the median own share and lateral length sqrt((mx + my) / m1) over the resolved nodes whose m1 > 0, the range of itn over
    all members, and the members that stopped at --lateral-maxit"""
    psf = np.asarray(psf, np.float64).reshape(-1, 7)
    ok = psf[:, 1] > 0
    lines = []
    if ok.any():
        length = np.sqrt(_ratio(psf[:, 3] + psf[:, 4], psf[:, 1]))
        lines.append(" depth lateral resolution: %d of %d resolved nodes answer; median own share %.4f, median lateral length %.4f cells" %
                     (int(ok.sum()), len(ok), float(np.median(np.asarray(columns["own"])[ok])), float(np.median(length[ok]))))
    else:
        lines.append(" depth lateral resolution: none of the %d resolved nodes answers" % len(ok))
    itn = np.asarray(res["itn"]); istop = np.asarray(res["istop"])
    lines.append(" depth lateral resolution: %d members, %d to %d conjugate-gradient iterations" % (len(itn), int(itn.min()), int(itn.max())))
    late = np.flatnonzero(istop == 2)
    if late.size:
        lines.append(" depth lateral resolution: %d members stopped at --lateral-maxit (istop 2), the first: member %d (kind %d, index %d)" %
                     (late.size, int(late[0]), int(res["kind"][late[0]]), int(res["index"][late[0]])))
    return lines


def resolve_lateral(eng, c, plan, obs, wt, smooth, damp, lateral, lateral_tol, lateral_maxit, sigma, out_dir, stride=1, checker=None, log=print):
    """--lateral-resolution on an engine whose stage holds the final model: the runs of plan once more, then one columns_resolution_lateral
    with every stride-th unknown as kind 0 and as kind 1 and, with checker (parse_checkerboard's tuple), the test model as kind 2 last; the
    files, the log.  Returns dict(lateral_resolution: the call's result with kind and index added, sigma, columns, lateral_resolution_path,
    and with checker lateral_checker_path, checker_model, checker_recovered)."""
    for wave, kind, t, first in plan:
        eng.dispersion_run(wave, kind, t, True, first, first)
    M, nvx, nvy = c["nz"] - 1, c["nx"] - 2, c["ny"] - 2
    unknowns = np.arange(0, nvx * nvy * M, stride, dtype=np.int32)
    n = len(unknowns)
    kind = np.concatenate([np.zeros(n, np.int32), np.ones(n, np.int32)]); index = np.concatenate([unknowns, unknowns])
    models = None
    if checker is not None:
        models = checkerboard_model(nvx, nvy, M, checker)[None]
        kind = np.append(kind, np.int32(2)); index = np.append(index, np.int32(0))
    res = eng.columns_resolution_lateral(obs, wt, smooth, damp, lateral, kind, index, models, lateral_tol, lateral_maxit, full=checker is not None)
    res = dict(res, kind=kind, index=index)
    psf, unit = res["measures"][:n], res["measures"][n:2 * n]
    columns = lateral_resolution_columns(unknowns, psf, unit, sigma)
    rpath = os.path.join(out_dir, "DSurfTomo.inDepthLateralResolution.dat")
    write_lateral_resolution(rpath, c, unknowns, columns)
    for line in lateral_resolution_log(columns, psf, res):
        log(line)
    log(" depth lateral resolution: %d nodes written to %s (sd for a data standard deviation of %.6f km/s)" % (n, rpath, sigma))
    out = dict(lateral_resolution=res, sigma=float(sigma), columns=columns, lateral_resolution_path=rpath)
    if checker is not None:
        cpath = os.path.join(out_dir, "DSurfTomo.inDepthLateralChecker.dat")
        recovered = res["full"][2 * n]
        write_lateral_checker(cpath, c, models[0], recovered)
        log(" depth lateral resolution: checkerboard of %d x %d x %d blocks, amplitude %g km/s: recovered amplitude median %.4f of the input, written to %s" %
            (checker[0], checker[1], checker[2], checker[3], float(np.median(recovered / models[0])), cpath))
        out.update(lateral_checker_path=cpath, checker_model=models[0], checker_recovered=recovered)
    return out


# ---- radial anisotropy ----

def check_radial(c, resolution=False):
    """what --radial asks of the other flags and of the input c (None: not read yet), before the engine is created (ValueError)"""
    if resolution:
        raise ValueError("--radial and --resolution exclude each other: the resolution of the coupled Vsv / Vsh system is not computed")
    if c is None:
        return
    nr = len(c["tRc"]) + len(c["tRg"]); nl = len(c["tLc"]) + len(c["tLg"])
    if nr == 0 or nl == 0:
        raise ValueError("--radial needs Rayleigh and Love periods, the input lists %d and %d" % (nr, nl))


def check_radial_lateral(radial_lateral=None, radial_lateral_aniso=None, radial=False, lateral=None, resolution=False):
    """what --radial-lateral and --radial-lateral-aniso ask of the other flags, before the library is loaded (ValueError)"""
    if radial_lateral is None and radial_lateral_aniso is None:
        return
    if radial_lateral is None:
        raise ValueError("--radial-lateral-aniso needs --radial-lateral: it is the weight of that coupling on Vsh - Vsv")
    if not radial:
        raise ValueError("--radial-lateral needs --radial: it couples the columns of the radial step (--lateral couples those of the isotropic one)")
    if lateral is not None or resolution:
        raise ValueError("--radial-lateral and %s exclude each other: %s" % (("--lateral", "--lateral couples the columns of the isotropic step") if lateral is not None
                                                                            else ("--resolution", "the resolution of the coupled system is not computed")))


def iterate_radial(eng, plan, obs, wt, iterations, smooth, damp, aniso, dvmax, minvel, maxvel, log=print, lateral=None, lateral_aniso=None,
                   lateral_tol=DEFAULT_LATERAL_TOL, lateral_maxit=DEFAULT_LATERAL_MAXIT):
    """iterate on an engine whose stage is radial (dispersion_begin_radial): per iteration the runs of plan -- the Love runs read Vsh, the
    Rayleigh runs Vsv -- then columns_step_radial -- or, with lateral (not None), columns_step_radial_lateral with the weights lateral and
    lateral_aniso (None: lateral).  Returns dict(history: one dict per iteration {iteration, nused, chi2, rms, nused_r, nused_l, rms_r, rms_l
    (before the step), flagged1, flagged2; with lateral also itn, istop, carried (the step's own count)}, steps: the step's result per
    iteration)."""
    if lateral is not None and lateral_aniso is None:
        lateral_aniso = lateral
    if lateral is None:
        step = lambda: eng.columns_step_radial(obs, wt, smooth, damp, aniso, dvmax, minvel, maxvel)
    else:
        step = lambda: eng.columns_step_radial_lateral(obs, wt, smooth, damp, aniso, lateral, lateral_aniso, dvmax, minvel, maxvel, lateral_tol, lateral_maxit)

    def entry(it, out):
        h = dict(iteration=it, nused=int(out["nused"].sum()), chi2=float(out["chi2"].sum()), rms=rms_of(out["chi2"], out["nused"]),
                 nused_r=int(out["nused"][0].sum()), nused_l=int(out["nused"][1].sum()), rms_r=rms_of(out["chi2"][0], out["nused"][0]),
                 rms_l=rms_of(out["chi2"][1], out["nused"][1]), flagged1=int((out["flag"] == 1).sum()), flagged2=int((out["flag"] == 2).sum()))
        log(" depth iteration %d (radial): %d Rayleigh data rms %.6f km/s, %d Love data rms %.6f km/s before the step, %d columns flagged (%d not positive definite, %d without data)" %
            (it, h["nused_r"], h["rms_r"], h["nused_l"], h["rms_l"], h["flagged1"] + h["flagged2"], h["flagged1"], h["flagged2"]))
        return h

    return _iterate(eng, plan, iterations, step, entry, log, None if lateral is None else "radial, lateral %g, on Vsh - Vsv %g" % (lateral, lateral_aniso))


def voigt_xi(vsv, vsh):
    """the Voigt average sqrt((2 Vsv^2 + Vsh^2) / 3) and xi = (Vsh / Vsv)^2, fp64 (xi 0 where Vsv is 0)"""
    v = np.asarray(vsv, np.float64); h = np.asarray(vsh, np.float64)
    r = np.divide(h, v, out=np.zeros(v.shape), where=v != 0)
    return np.sqrt((2.0 * v * v + h * h) / 3.0), r * r


def xi_summary(c, vsv, vsh, flag):
    """(median, min, max) of xi over the nodes above the bottom depth of the interior columns whose flag is 0, or None without any"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    inner = np.zeros((ny, nx), bool); inner[1:-1, 1:-1] = True
    ok = inner.ravel() & (np.asarray(flag).reshape(ny * nx) == 0)
    if not ok.any():
        return None
    xi = voigt_xi(np.asarray(vsv).reshape(nz, ny * nx)[:nz - 1, ok], np.asarray(vsh).reshape(nz, ny * nx)[:nz - 1, ok])[1]
    return float(np.median(xi)), float(xi.min()), float(xi.max())


def write_radial(path, c, vsv, vsh):
    """<input>DepthRadial.dat: vsv, vsh (nz, ny, nx), every node in Depth.dat's order"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.asarray(vsv, np.float64).reshape(nz, ny, nx); h = np.asarray(vsh, np.float64).reshape(nz, ny, nx)
    voigt, xi = voigt_xi(v, h)
    rows = []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                rows.append(dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]), vsv=v[k, j, i], vsh=h[k, j, i], voigt=voigt[k, j, i], xi=xi[k, j, i]))
    io.write_table(path, RADIAL_TABLE, rows)


def read_radial(path):
    return io.read_table(path, RADIAL_TABLE)


def write_radial_fit(path, c, first, last):
    """<input>DepthRadialFit.dat: first / last = columns_step_radial's results of the first and the last iteration; one line per column, j then i"""
    nx, ny = c["nx"], c["ny"]
    col_rms = lambda s, q: np.sqrt(np.divide(s["chi2"][q], s["nused"][q], out=np.zeros(nx * ny), where=s["nused"][q] > 0))
    rows = []
    r = [[col_rms(first, q), col_rms(last, q)] for q in range(2)]
    for j in range(ny):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            q = j * nx + i
            rows.append(dict(lon=float(lon), lat=float(lat), nused_r=int(last["nused"][0][q]), nused_l=int(last["nused"][1][q]), rms_first_r=float(r[0][0][q]),
                             rms_last_r=float(r[0][1][q]), rms_first_l=float(r[1][0][q]), rms_last_l=float(r[1][1][q]), flag=int(last["flag"][q])))
    io.write_table(path, RADIAL_FIT_TABLE, rows)


def read_radial_fit(path):
    return io.read_table(path, RADIAL_FIT_TABLE)


def run_radial(eng, c, plan, obs, wt, iterations, smooth, damp, aniso, dvmax, out_dir, log=print, lateral=None, lateral_aniso=None,
               lateral_tol=DEFAULT_LATERAL_TOL, lateral_maxit=DEFAULT_LATERAL_MAXIT):
    """--radial on a fresh engine: both models start as the input's, the loop (iterate_radial, to which lateral and its companions go), the
    two files, the log's xi.  Returns (iterate_radial's result with vsv, vsh (nz, ny, nx) and xi (xi_summary) added, the paths of
    DepthRadial.dat and DepthRadialFit.dat)."""
    kmax = c["kmax"]
    start = np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0))
    eng.dispersion_begin_radial(start, start, c["depz"], c["minthk"], kmax, kmax)
    out = iterate_radial(eng, plan, obs, wt, iterations, smooth, damp, aniso, dvmax, float(c["minvel"]), float(c["maxvel"]), log, lateral, lateral_aniso, lateral_tol,
                         lateral_maxit)
    out["vsv"], out["vsh"] = eng.dispersion_get_model_radial()
    out["xi"] = xi_summary(c, out["vsv"], out["vsh"], out["steps"][-1]["flag"])
    path = os.path.join(out_dir, "DSurfTomo.inDepthRadial.dat")
    fit = os.path.join(out_dir, "DSurfTomo.inDepthRadialFit.dat")
    write_radial(path, c, out["vsv"], out["vsh"])
    write_radial_fit(fit, c, out["steps"][0], out["steps"][-1])
    if out["xi"] is not None:
        log(" depth (radial): xi = (Vsh / Vsv)^2 median %.4f, range %.4f to %.4f over the unflagged interior nodes above the bottom depth" % out["xi"])
    log(" depth (radial): %d x %d x %d nodes of Vsv, Vsh, Voigt average and xi written to %s, the fit of %d columns to %s" % (c["nx"], c["ny"], c["nz"], path, c["nx"] * c["ny"], fit))
    return out, path, fit


# ---- the resolution of the radial step ----

def check_radial_resolution(radial_resolution=False, radial=False, radial_lateral=None):
    """what --radial-resolution asks of the other flags, before the library is loaded (ValueError)"""
    if not radial_resolution:
        return
    if not radial:
        raise ValueError("--radial-resolution needs --radial: it is the resolution of the radial step (--resolution is that of the isotropic one)")
    if radial_lateral is not None:
        raise ValueError("--radial-resolution and --radial-lateral exclude each other: the resolution of the laterally coupled system is not computed")


def leak_share(m1_own, m1_cross):
    """m1_cross / (m1_own + m1_cross): the share of a spike's answer that lies in the other model, 0 where the denominator is 0"""
    own = np.asarray(m1_own, np.float64); cross = np.asarray(m1_cross, np.float64)
    total = own + cross
    return np.divide(cross, total, out=np.zeros(total.shape), where=total > 0)


def radial_resolution_columns(res, vsv, vsh, sigma):
    """The node figures of DepthRadialResolution.dat from columns_resolution_radial's result res, the models vsv, vsh ((nz, ...) with the
    columns in res's order) and the data's standard deviation sigma (S, km/s).  Returns a dict of (nz - 1, columns) arrays: for q in v, h
    rjj_q, length_q = sqrt(m2_own / m1_own), leak_q (leak_share), sd_q = S sqrt(var); r_aniso = (R_vv + R_hh - R_hv - R_vh) / 2 from R_jj
    and R_cross; sd_diff = S sqrt(vard); sd_xi = 2 xi S sqrt(var_v / Vsv^2 + var_h / Vsh^2 - 2 cov / (Vsv Vsh)), the radicand clamped at 0
    (0 where a velocity is 0); xi."""
    m = np.asarray(res["measures"], np.float64)
    M = m.shape[1] // 2
    ncol = m.shape[2]
    pair = np.asarray(res["pair"], np.float64)
    v = np.asarray(vsv, np.float64).reshape(M + 1, ncol)[:M]; h = np.asarray(vsh, np.float64).reshape(M + 1, ncol)[:M]
    S = float(sigma)
    out = {}
    for q, blk in (("v", slice(0, M)), ("h", slice(M, 2 * M))):
        out["rjj_" + q] = m[0][blk]
        out["length_" + q] = psf_length(m[1][blk], m[2][blk])
        out["leak_" + q] = leak_share(m[1][blk], m[3][blk])
        out["sd_" + q] = S * np.sqrt(m[5][blk])
    out["r_aniso"] = 0.5 * (m[0][:M] + m[0][M:] - m[4][:M] - m[4][M:])
    out["sd_diff"] = S * np.sqrt(pair[1])
    xi = voigt_xi(v, h)[1]
    ok = (v != 0) & (h != 0)
    vs = np.where(ok, v, 1.0); hs = np.where(ok, h, 1.0)
    rad = np.maximum(m[5][:M] / (vs * vs) + m[5][M:] / (hs * hs) - 2.0 * pair[0] / (vs * hs), 0.0)
    out["sd_xi"] = np.where(ok, 2.0 * xi * S * np.sqrt(rad), 0.0)
    out["xi"] = xi
    return out


RADIAL_RESOLUTION_NAMES = ("rjj_v", "length_v", "leak_v", "sd_v", "rjj_h", "length_h", "leak_h", "sd_h", "r_aniso", "sd_diff", "sd_xi")
RADIAL_RESOLUTION_TABLE = (True, _F64("lon", "lat", "depth", *RADIAL_RESOLUTION_NAMES))


def write_radial_resolution(path, c, res, vsv, vsh, sigma):
    """<input>DepthRadialResolution.dat: radial_resolution_columns of every node above the bottom depth: depth slowest, then j, then i"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    cols = radial_resolution_columns(res, np.asarray(vsv).reshape(nz, ny * nx), np.asarray(vsh).reshape(nz, ny * nx), sigma)
    rows = []
    for k in range(nz - 1):
        for j in range(ny):
            for i in range(nx):
                lon, lat = _lonlat(c, i - 1, j - 1)
                row = dict(lon=float(lon), lat=float(lat), depth=float(c["depz"][k]))
                row.update((name, cols[name][k, j * nx + i]) for name in RADIAL_RESOLUTION_NAMES)
                rows.append(row)
    io.write_table(path, RADIAL_RESOLUTION_TABLE, rows)


def read_radial_resolution(path):
    return io.read_table(path, RADIAL_RESOLUTION_TABLE)


def write_radial_leverage(path, c, leverage):
    """<input>DepthRadialLeverage.dat: leverage (nmaps, ny * nx) of columns_resolution_radial, in DepthLeverage.dat's layout"""
    write_leverage(path, c, leverage)


def read_radial_leverage(path):
    return io.read_table(path, LEVERAGE_TABLE)


def radial_resolution_summary(c, res, vsv, vsh, sigma):
    """what the log says of columns_resolution_radial's result: dict(flagged1, flagged2, columns (interior and not flagged), trace_v, trace_h
    ((median, min, max) of each block's trace over them), leak_v, leak_h (the median leak share of each block's nodes over them),
    significant: how many of their nodes have |xi - 1| > 2 sd_xi, nodes: how many nodes they have)"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    inner = np.zeros((ny, nx), bool); inner[1:-1, 1:-1] = True
    flag = np.asarray(res["flag"]).reshape(ny * nx)
    ok = inner.ravel() & (flag == 0)
    out = dict(flagged1=int((flag == 1).sum()), flagged2=int(((flag == 2) & inner.ravel()).sum()), columns=int(ok.sum()), trace_v=None, trace_h=None, leak_v=None,
               leak_h=None, significant=0, nodes=int(ok.sum()) * (nz - 1))
    if ok.any():
        cols = radial_resolution_columns(res, np.asarray(vsv).reshape(nz, ny * nx), np.asarray(vsh).reshape(nz, ny * nx), sigma)
        for q, name in enumerate(("v", "h")):
            tr = np.asarray(res["trace"])[q][ok]
            out["trace_" + name] = (float(np.median(tr)), float(tr.min()), float(tr.max()))
            out["leak_" + name] = float(np.median(cols["leak_" + name][:, ok]))
        out["significant"] = int((np.abs(cols["xi"][:, ok] - 1.0) > 2.0 * cols["sd_xi"][:, ok]).sum())
    return out


def resolve_radial(eng, c, plan, obs, wt, smooth, damp, aniso, sigma, out_dir, log=print):
    """--radial-resolution on an engine whose radial stage holds the final models: the runs of plan once more, columns_resolution_radial, the
    two files, the log.  Returns dict(resolution: the call's result, sigma, summary, resolution_path, leverage_path)."""
    for wave, kind, t, first in plan:
        eng.dispersion_run(wave, kind, t, True, first, first)
    res = eng.columns_resolution_radial(obs, wt, smooth, damp, aniso)
    vsv, vsh = eng.dispersion_get_model_radial()
    rpath = os.path.join(out_dir, "DSurfTomo.inDepthRadialResolution.dat")
    lpath = os.path.join(out_dir, "DSurfTomo.inDepthRadialLeverage.dat")
    write_radial_resolution(rpath, c, res, vsv, vsh, sigma)
    write_radial_leverage(lpath, c, res["leverage"])
    sm = radial_resolution_summary(c, res, vsv, vsh, sigma)
    for line in radial_resolution_log(c, sm):
        log(line)
    log(" depth radial resolution: written to %s (sd for a data standard deviation of %.6f km/s), the leverages to %s" % (rpath, sigma, lpath))
    return dict(resolution=res, sigma=float(sigma), summary=sm, resolution_path=rpath, leverage_path=lpath)


def radial_resolution_log(c, sm):
    """the log's lines for radial_resolution_summary's dict"""
    lines = [" depth radial resolution: %d columns resolved, %d flagged (%d not positive definite, %d without data)" %
             (sm["columns"], sm["flagged1"] + sm["flagged2"], sm["flagged1"], sm["flagged2"])]
    if sm["trace_v"] is not None:
        for name, q in (("Vsv", "v"), ("Vsh", "h")):
            lines.append(" depth radial resolution: trace of the %s block of R per column median %.4f, range %.4f to %.4f, of %d unknowns; median leak share %.4f" %
                         (name, sm["trace_" + q][0], sm["trace_" + q][1], sm["trace_" + q][2], c["nz"] - 1, sm["leak_" + q]))
        lines.append(" depth radial resolution: |xi - 1| > 2 sd_xi at %d of %d unflagged nodes" % (sm["significant"], sm["nodes"]))
    return lines


def run(directory, maps_file=None, iterations=DEFAULT_ITERATIONS, smooth=DEFAULT_SMOOTH, damp=DEFAULT_DAMP, dvmax=DEFAULT_DVMAX, min_dws=0.0, out_dir=".",
        log=print, resolution=False, sigma=None, radial=False, aniso=DEFAULT_ANISO, lateral=None, lateral_tol=DEFAULT_LATERAL_TOL,
        lateral_maxit=DEFAULT_LATERAL_MAXIT, radial_lateral=None, radial_lateral_aniso=None, radial_resolution=False, lateral_resolution=False,
        lateral_resolution_stride=1, lateral_checkerboard=None, sample=None, sample_step=DEFAULT_SAMPLE_STEP, sample_spread=DEFAULT_SAMPLE_SPREAD,
        sample_width=DEFAULT_SAMPLE_WIDTH, sample_seed=DEFAULT_SAMPLE_SEED, sample_temperature=DEFAULT_SAMPLE_TEMPERATURE, sample_block=0,
        sample_block_scale=None, sample_bins=0, sample_quantiles=DEFAULT_SAMPLE_QUANTILES, sample_covariance=False):
    """the driver behind main(); returns (iterate's result with vels (nz, ny, nx) added, the paths of Depth.dat and DepthFit.dat).  With
    resolution the first item also holds resolve's entries (resolution_path and leverage_path among them); sigma None: the rms before the
    last step.  With radial: run_radial's result (DepthRadial.dat and DepthRadialFit.dat in place of the two files).  With lateral (not
    None): the loop steps with columns_step_lateral; the files are the same two.  With radial and radial_lateral (not None): the radial loop
    steps with columns_step_radial_lateral, radial_lateral_aniso (None: radial_lateral) the weight on Vsh - Vsv; the files are --radial's.
    With radial and radial_resolution: after the loop resolve_radial's entries are added to the first item (DepthRadialResolution.dat and
    DepthRadialLeverage.dat beside --radial's files); sigma as with resolution.  With lateral and lateral_resolution: after the loop
    resolve_lateral's entries are added to the first item (DepthLateralResolution.dat and, with lateral_checkerboard, DepthLateralChecker.dat
    beside the two files); sigma as with resolution.  With sample ("C,SWEEPS[,BURN]"): after the loop (and the resolution) run_sample's entries
    are added to the first item (DepthPosterior.dat and DepthPosteriorFit.dat beside the two files); sigma as with resolution; sample_block
    (EVERY > 0) makes every EVERY-th sweep a block proposal of scale sample_block_scale (None: sample_block_scale(nz - 1, temperature));
    sample_bins (2 .. 256) adds the posterior marginals at the levels sample_quantiles ("P1,P2,...") and, with sample_covariance, the
    correlations between a column's depths (run_sample's three files)."""
    sampling = check_sample(sample, radial, lateral, sample_step, sample_spread, sample_width, sample_temperature, sample_seed, sample_block, sample_block_scale)
    marginals = check_marginals(sample, sample_bins, sample_quantiles, sample_covariance)
    checker = check_flags(iterations, smooth, damp, dvmax, min_dws, sigma, aniso if radial else None, radial, resolution, lateral, lateral_tol, lateral_maxit,
                          radial_lateral, radial_lateral_aniso, radial_resolution, lateral_resolution, lateral_resolution_stride, lateral_checkerboard)
    c = io.load(directory)
    if radial:
        check_radial(c)
    maps_file = os.path.join(out_dir, "DSurfTomo.inMaps.dat") if maps_file is None else maps_file
    obs, dws = maps_to_obs(maps.read_maps(maps_file), c)
    plan = slot_plan(c)
    kmax = c["kmax"]
    if not plan or kmax > 60:
        raise ValueError("depth: %d periods; the step takes 1 to 60" % kmax)
    wt = dws_weights(dws, min_dws) if min_dws > 0 else None
    from .engine import Engine
    eng = Engine(0)
    if radial:
        try:
            result = run_radial(eng, c, plan, obs, wt, iterations, smooth, damp, aniso, dvmax, out_dir, log, radial_lateral, radial_lateral_aniso, lateral_tol, lateral_maxit)
            if radial_resolution:
                rms = result[0]["history"][-1]["rms"]
                log(" depth radial resolution: the data's standard deviation is %s" % ("--sigma %.6f km/s" % sigma if sigma is not None else "the rms before the last step, %.6f km/s" % rms))
                result[0].update(resolve_radial(eng, c, plan, obs, wt, smooth, damp, aniso, rms if sigma is None else sigma, out_dir, log))
            return result
        finally:
            eng.close()
    try:
        eng.dispersion_begin(np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0)), c["depz"], c["minthk"], kmax, kmax)
        out = iterate(eng, plan, obs, wt, iterations, smooth, damp, dvmax, float(c["minvel"]), float(c["maxvel"]), log, lateral, lateral_tol, lateral_maxit)
        out["vels"] = eng.dispersion_get_model()
        if resolution:
            rms = out["history"][-1]["rms"]
            log(" depth resolution: the data's standard deviation is %s" % ("--sigma %.6f km/s" % sigma if sigma is not None else "the rms before the last step, %.6f km/s" % rms))
            out.update(resolve(eng, c, plan, obs, wt, smooth, damp, rms if sigma is None else sigma, out_dir, log))
        if lateral_resolution:
            rms = out["history"][-1]["rms"]
            log(" depth lateral resolution: the data's standard deviation is %s" % ("--sigma %.6f km/s" % sigma if sigma is not None else "the rms before the last step, %.6f km/s" % rms))
            out.update(resolve_lateral(eng, c, plan, obs, wt, smooth, damp, lateral, lateral_tol, lateral_maxit, rms if sigma is None else sigma, out_dir,
                                       lateral_resolution_stride, checker, log))
        if sampling is not None:
            rms = out["history"][-1]["rms"]
            log(" depth sample: the data's standard deviation is %s" % ("--sigma %.6f km/s" % sigma if sigma is not None else "the rms before the last step, %.6f km/s" % rms))
            out.update(run_sample(eng, c, plan, out["vels"], obs, wt, smooth, rms if sigma is None else sigma, sampling, out_dir, sample_step, sample_spread,
                                  sample_width, sample_seed, sample_temperature, log, sample_block, sample_block_scale, damp, marginals))
    finally:
        eng.close()
    path = os.path.join(out_dir, "DSurfTomo.inDepth.dat")
    fit = os.path.join(out_dir, "DSurfTomo.inDepthFit.dat")
    write_depth(path, c, out["vels"])
    write_fit(fit, c, out["steps"][0], out["steps"][-1])
    log(" depth: %d x %d x %d nodes written to %s, the fit of %d columns to %s" % (c["nx"], c["ny"], c["nz"], path, c["nx"] * c["ny"], fit))
    return out, path, fit


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--maps", default=None, metavar="FILE", help="the maps file of dsurftomo_amd.maps (default: DSurfTomo.inMaps.dat in --out)")
    ap.add_argument("--iterations", type=int, default=DEFAULT_ITERATIONS, metavar="N")
    ap.add_argument("--smooth", type=float, default=DEFAULT_SMOOTH, metavar="L", help="weight of the depth Laplacian (default %g)" % DEFAULT_SMOOTH)
    ap.add_argument("--damp", type=float, default=DEFAULT_DAMP, metavar="D", help="damping of a column's step, > 0 (default %g)" % DEFAULT_DAMP)
    ap.add_argument("--dvmax", type=float, default=DEFAULT_DVMAX, metavar="V", help="largest change of a node per iteration in km/s (default %g)" % DEFAULT_DVMAX)
    ap.add_argument("--min-dws", type=float, default=0.0, metavar="X", help="map vertices whose column DWS is below X get weight 0 (default 0: all count)")
    ap.add_argument("--out", default=".")
    ap.add_argument("--resolution", action="store_true", help="after the last step write the resolution measures and the leverages of the final model")
    ap.add_argument("--sigma", type=float, default=None, metavar="S", help="standard deviation of the map values in km/s for the sd column (default: the rms before the last step)")
    ap.add_argument("--radial", action="store_true", help="radial anisotropy: invert the Rayleigh maps for Vsv(z) and the Love maps for Vsh(z) together")
    ap.add_argument("--aniso", type=float, default=DEFAULT_ANISO, metavar="G", help="with --radial: weight of the tie between Vsh and Vsv, >= 0 (default %g)" % DEFAULT_ANISO)
    ap.add_argument("--lateral", type=float, default=None, metavar="W", help="couple neighbouring columns: weight of the penalty on their differences, >= 0 (default: columns alone)")
    ap.add_argument("--lateral-tol", type=float, default=DEFAULT_LATERAL_TOL, metavar="T", help="with --lateral: relative tolerance of the conjugate gradients, > 0 (default %g)" % DEFAULT_LATERAL_TOL)
    ap.add_argument("--lateral-maxit", type=int, default=DEFAULT_LATERAL_MAXIT, metavar="N", help="with --lateral: most conjugate-gradient iterations per step (default %d)" % DEFAULT_LATERAL_MAXIT)
    ap.add_argument("--radial-lateral", type=float, default=None, metavar="W", help="with --radial: couple neighbouring columns, weight of the penalty on the differences of Vsv and of Vsh, >= 0 (default: columns alone); --lateral-tol and --lateral-maxit apply")
    ap.add_argument("--radial-lateral-aniso", type=float, default=None, metavar="A", help="with --radial-lateral: weight of the penalty on the differences of Vsh - Vsv between neighbours, >= 0 (default: W)")
    ap.add_argument("--radial-resolution", action="store_true", help="with --radial: after the last step write the resolution measures of Vsv, Vsh and xi and the leverages of the final models (--sigma applies)")
    ap.add_argument("--lateral-resolution", action="store_true", help="with --lateral: after the last step write the point-spread lengths, own shares and standard deviations of the coupled system (--sigma applies)")
    ap.add_argument("--lateral-resolution-stride", type=int, default=1, metavar="N", help="with --lateral-resolution: resolve every N-th unknown (default 1: all)")
    ap.add_argument("--lateral-checkerboard", default=None, metavar="NX,NY,NZ[,AMP]", help="with --lateral-resolution: recover a checkerboard of NX x NY x NZ blocks of amplitude AMP km/s (default %g)" % DEFAULT_CHECKER_AMP)
    ap.add_argument("--sample", default=None, metavar="C,SWEEPS[,BURN]", help="after the last step sample the posterior of every column with C Metropolis chains for SWEEPS sweeps, the first BURN (default SWEEPS / 2) left out (--sigma applies)")
    ap.add_argument("--sample-step", type=float, default=DEFAULT_SAMPLE_STEP, metavar="S", help="with --sample: half width of the single-node proposal in km/s (default %g)" % DEFAULT_SAMPLE_STEP)
    ap.add_argument("--sample-spread", type=float, default=DEFAULT_SAMPLE_SPREAD, metavar="P", help="with --sample: half width of the scatter of the chains' starts in km/s (default %g)" % DEFAULT_SAMPLE_SPREAD)
    ap.add_argument("--sample-width", type=float, default=DEFAULT_SAMPLE_WIDTH, metavar="W", help="with --sample: half width of the prior box about the step's result in km/s (default %g)" % DEFAULT_SAMPLE_WIDTH)
    ap.add_argument("--sample-seed", type=int, default=DEFAULT_SAMPLE_SEED, metavar="N", help="with --sample: seed of the counter-based generator (default %d)" % DEFAULT_SAMPLE_SEED)
    ap.add_argument("--sample-temperature", type=float, default=DEFAULT_SAMPLE_TEMPERATURE, metavar="T", help="with --sample: the chains sample exp(-(phi + psi) / 2T) (default %g)" % DEFAULT_SAMPLE_TEMPERATURE)
    ap.add_argument("--sample-block", type=int, default=0, metavar="EVERY", help="with --sample: every EVERY-th sweep proposes all nodes of a column at once, along its linearised posterior (default 0: single nodes only)")
    ap.add_argument("--sample-block-scale", type=float, default=None, metavar="S", help="with --sample-block: scale of the block proposal (default 2.38 sqrt(3 T / M) for M unknowns per column at temperature T)")
    ap.add_argument("--sample-bins", type=int, default=0, metavar="NB", help="with --sample: histogram every node's kept states in NB (2 to 256) equal bins of its box and write mode, quantiles and marginals (default 0: off)")
    ap.add_argument("--sample-quantiles", default=DEFAULT_SAMPLE_QUANTILES, metavar="P1,P2,...", help="with --sample-bins: the levels of the quantiles, at most 16 inside (0, 1) (default %s)" % DEFAULT_SAMPLE_QUANTILES)
    ap.add_argument("--sample-covariance", action="store_true", help="with --sample-bins: also accumulate the covariance between the depths of a column and write their correlations")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check_flags(a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.sigma, a.aniso, a.radial, a.resolution, a.lateral, a.lateral_tol, a.lateral_maxit,
                    a.radial_lateral, a.radial_lateral_aniso, a.radial_resolution, a.lateral_resolution, a.lateral_resolution_stride, a.lateral_checkerboard)
        check_sample(a.sample, a.radial, a.lateral, a.sample_step, a.sample_spread, a.sample_width, a.sample_temperature, a.sample_seed, a.sample_block,
                     a.sample_block_scale)
        check_marginals(a.sample, a.sample_bins, a.sample_quantiles, a.sample_covariance)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.maps, a.iterations, a.smooth, a.damp, a.dvmax, a.min_dws, a.out, resolution=a.resolution, sigma=a.sigma, radial=a.radial, aniso=a.aniso,
        lateral=a.lateral, lateral_tol=a.lateral_tol, lateral_maxit=a.lateral_maxit, radial_lateral=a.radial_lateral, radial_lateral_aniso=a.radial_lateral_aniso,
        radial_resolution=a.radial_resolution, lateral_resolution=a.lateral_resolution, lateral_resolution_stride=a.lateral_resolution_stride,
        lateral_checkerboard=a.lateral_checkerboard, sample=a.sample, sample_step=a.sample_step, sample_spread=a.sample_spread, sample_width=a.sample_width,
        sample_seed=a.sample_seed, sample_temperature=a.sample_temperature, sample_block=a.sample_block, sample_block_scale=a.sample_block_scale,
        sample_bins=a.sample_bins, sample_quantiles=a.sample_quantiles, sample_covariance=a.sample_covariance)
    return 0


if __name__ == "__main__":
    sys.exit(main())
