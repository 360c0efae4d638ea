"""Depth inversion of the period maps: per-column Vs(z) Gauss-Newton steps on the device.

    python -m dsurftomo_amd.depth <directory with DSurfTomo.in, the data file and MOD> [--maps FILE] [--iterations N] [--smooth L] [--damp D]
                                  [--dvmax V] [--min-dws X] [--out DIR] [--resolution [--sigma S]] [--radial [--aniso G]]
                                  [--lateral W [--lateral-tol T] [--lateral-maxit N]] [--radial-resolution]
                                  [--lateral-resolution [--lateral-resolution-stride N] [--lateral-checkerboard NX,NY,NZ[,AMP]]]
                                  [--sample C,SWEEPS[,BURN] [--sample-step S] [--sample-spread P] [--sample-width W] [--sample-seed N]
                                   [--sample-temperature T] [--sample-block EVERY [--sample-block-scale S]]
                                   [--sample-bins NB [--sample-quantiles P1,P2,...] [--sample-covariance]]]
                                  [--azimuthal [--azimuthal-smooth L] [--azimuthal-damp D] [--azimuthal-sigma S]]

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

--azimuthal [--azimuthal-smooth L] [--azimuthal-damp D] [--azimuthal-sigma S]: the maps file must be one of
maps --azimuthal, whose A1(T), A2(T) of c(psi) = c0 + A1 cos 2psi + A2 sin 2psi are inverted for gc(z) = Gc/L and gs(z) = Gs/L.  After the
last step (and the resolutions, before --sample) the runs are done once more on the final model and columns_azimuthal solves, per interior
column and with the loop's weights, (G^T G + L^2 L^T L + D^2 I) g = G^T rho for gc (rho from A1) and gs (rho from A2), G the Rayleigh data's
depth factor (Vs / 2) dc/dVs (Love periods are dropped), L and D defaulting to --smooth and --damp.  <input>DepthAzim.dat (write_azimuthal /
read_azimuthal): per node above the bottom depth longitude, latitude, depth, Vs, gc, gs, the strength 50 sqrt(gc^2 + gs^2) in per cent of
Vs, the fast axis 0.5 atan2(gs, gc) in degrees from north, R_jj, the vertical length of the point-spread function in km, sd_g = S sqrt(var),
sd_strength = 50 sd_g and sd_axis = (90 / pi) sd_g / sqrt(gc^2 + gs^2) degrees, capped at 90 / sqrt(3) (an axis uniform on a half circle);
S = --azimuthal-sigma in km/s or, by default, the rms of the fit's residual sqrt((chi2c + chi2s) / (2 nused)).  <input>DepthAzimFit.dat
(write_azimuthal_fit / read_azimuthal_fit): per column longitude, latitude, the data used, the rms of (A1, A2) before and after, the flag.
The log gives the columns solved and flagged, the rms before and after, S and where it came from, the median and largest strength, the
share of nodes whose amplitude exceeds 2 sd_g and the median R_jj per depth.  Refused with --radial and, for the three sub-options, without
--azimuthal; a maps file without the A1, A2 columns is refused by name.  Without the flag nothing changes.  column_azimuthal_twin is the
NumPy twin (csrc/column_azimuthal.h is the arithmetic).

column_l, column_ltl and column_step_twin restate the regulariser and the step in NumPy for the tests (csrc/column_system.h is the arithmetic
the device runs).  Every precondition is checked before the library is loaded.  There is no CPU path.
"""
import argparse
import math
import os
import sys
import types

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


from .depth_twins import (       # the NumPy twins of the device headers, under the names callers reach them by: depth.<name>
    SampleMarginalTwin, _radial_expand, azimuthal_factor, column_azimuthal_twin, _twin_data, _twin_factor, _twin_normal, column_l, column_lateral_resolution_twin, column_lateral_twin, column_ltl,
    column_radial_lateral_twin, column_radial_resolution_twin, column_radial_twin, column_resolution_twin, column_sample_twin, column_shape_twin, column_step_twin,
    column_tri, lateral_sum, sample_bits, sample_block_scale, sample_box, sample_marginal_bin, sample_marginal_counts, sample_marginal_mode, sample_marginal_quantile,
    sample_marginal_twin, sample_mix, sample_neglog, sample_psi, sample_rhat, sample_rsqrt, sample_sd, sample_unit)


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


def map_sigma_weights(rows, c, min_dws_mask=None, azimuthal=False):
    """The step's weights from the rows of <input>MapsResolution.dat (maps.read_maps_resolution): (wt, sigma_ref).  wt
    (nmaps, ny * nx) fp32 in maps_to_obs's layout = sigma_ref / sd where min_dws_mask (the same shape, None: all) keeps the datum, sd > 0 and
    the map's flag is 0; 0 elsewhere and on the outer ring.  sigma_ref: the median sd over the kept data (0 without any), so that a typical
    weight is 1 and --smooth and --damp keep their meaning.  azimuthal: the weights of the 2psi stage, from sqrt((sd_a1^2 + sd_a2^2) / 2).
    ValueError as maps_to_obs when the file does not hold the case's periods and vertices."""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    layer = nvx * nvz
    per = maps.period_list(c)
    if len(rows) != len(per) * layer:
        raise ValueError("depth: the map sigma file holds %d lines, %d periods of %d x %d interior vertices need %d" % (len(rows), len(per), nvx, nvz, len(per) * layer))
    sd = np.zeros((len(per), ny, nx)); ok = np.zeros((len(per), ny, nx), bool)
    for m, (wave, kind, t) in enumerate(per):
        block = rows[m * layer:(m + 1) * layer]
        if any((r["wave"], r["kind"], r["period"]) != (wave, kind, t) for r in block):
            raise ValueError("depth: map %d of the map sigma file is not wave %d kind %d period %g of the input" % (m, wave, kind, t))
        if azimuthal:
            v = np.sqrt(0.5 * (np.array([r["sd_a1"] for r in block]) ** 2 + np.array([r["sd_a2"] for r in block]) ** 2))
        else:
            v = np.array([r["sd"] for r in block])
        sd[m, 1:-1, 1:-1] = v.reshape(nvz, nvx)
        ok[m, 1:-1, 1:-1] = np.array([r["flag"] == 0 for r in block]).reshape(nvz, nvx)
    sd = sd.reshape(len(per), ny * nx); ok = ok.reshape(len(per), ny * nx)
    keep = ok & (sd > 0) & np.isfinite(sd)
    if min_dws_mask is not None:
        keep &= np.asarray(min_dws_mask, bool).reshape(keep.shape)
    sigma_ref = float(np.median(sd[keep])) if keep.any() else 0.0
    wt = np.divide(sigma_ref, sd, out=np.zeros(sd.shape), where=keep)
    return wt.astype(np.float32), sigma_ref


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

def _column_rows(c):
    """lon, lat of every column: j, then i -- with its place j * nx + i"""
    nx = c["nx"]
    for j in range(c["ny"]):
        for i in range(nx):
            lon, lat = _lonlat(c, i - 1, j - 1)
            yield j * nx + i, dict(lon=float(lon), lat=float(lat))


def _node_rows(c, depths):
    """lon, lat, depth of every node of the first `depths` depths (nz: all of them, nz - 1: those above the bottom depth): depth slowest, then
    j, then i -- with its place (k, j * nx + i)"""
    for k in range(depths):
        for q, row in _column_rows(c):
            yield k, q, dict(row, depth=float(c["depz"][k]))


def write_depth(path, c, vels):
    """<input>Depth.dat: vels (nz, ny, nx), every node: depth slowest, then j, then i"""
    v = np.asarray(vels, np.float64).reshape(c["nz"], c["ny"] * c["nx"])
    io.write_table(path, DEPTH_TABLE, [dict(row, vs=v[k, q]) for k, q, row in _node_rows(c, c["nz"])])


def read_depth(path):
    return io.read_table(path, DEPTH_TABLE)


def write_fit(path, c, first, last):
    """<input>DepthFit.dat: first / last = columns_step's results of the first and the last iteration; one line per column, j then i"""
    nx, ny = c["nx"], c["ny"]
    col_rms = lambda s: np.sqrt(np.divide(s["chi2"], s["nused"], out=np.zeros(nx * ny), where=s["nused"] > 0))
    r0, r1 = col_rms(first), col_rms(last)
    io.write_table(path, FIT_TABLE, [dict(row, nused=int(last["nused"][q]), rms_first=float(r0[q]), rms_last=float(r1[q]), flag=int(last["flag"][q]))
                                     for q, row in _column_rows(c)])


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
    m = np.asarray(measures, np.float64).reshape(4, nz - 1, ny * nx)
    length = psf_length(m[1], m[2]); sd_unit = np.sqrt(m[3])
    io.write_table(path, RESOLUTION_TABLE, [dict(row, rjj=m[0, k, q], length=length[k, q], sd_unit=sd_unit[k, q], sd=float(sigma) * sd_unit[k, q])
                                            for k, q, row in _node_rows(c, nz - 1)])


def read_resolution(path):
    return io.read_table(path, RESOLUTION_TABLE)


def write_leverage(path, c, leverage):
    """<input>DepthLeverage.dat: leverage (nmaps, ny * nx) of columns_resolution; one line per column (j, then i) and period in slot order"""
    nx, ny = c["nx"], c["ny"]
    per = maps.period_list(c)
    h = np.asarray(leverage, np.float64).reshape(len(per), ny * nx)
    io.write_table(path, LEVERAGE_TABLE, [dict(row, wave=int(wave), kind=int(kind), period=float(t), leverage=h[k, q])
                                          for q, row in _column_rows(c) for k, (wave, kind, t) in enumerate(per)])


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


# ---- the depth inversion of the maps' 2 psi terms: the driver's side ----

AZIMUTHAL_TABLE = (True, _F64("lon", "lat", "depth", "vs", "gc", "gs", "strength", "axis", "rjj", "length", "sd_g", "sd_strength", "sd_axis"))
AZIMUTHAL_FIT_TABLE = (True, _F64("lon", "lat") + (("nused", "%d", "int"),) + _F64("rms_before", "rms_after") + (("flag", "%d", "int"),))
SD_AXIS_CAP = 90.0 / math.sqrt(3.0)                 # the sd in degrees of an axis uniform on a half circle


def check_azimuthal(azimuthal=False, radial=False, smooth=None, damp=None, sigma=None):
    """what --azimuthal and its three sub-options ask, before the library is loaded (ValueError)"""
    if not azimuthal:
        for name, v in (("--azimuthal-smooth", smooth), ("--azimuthal-damp", damp), ("--azimuthal-sigma", sigma)):
            if v is not None:
                raise ValueError("%s needs --azimuthal" % name)
        return
    if radial:
        raise ValueError("--azimuthal and --radial exclude each other: the 2 psi terms are not inverted on the radial stage")
    if smooth is not None and not (np.isfinite(smooth) and smooth >= 0):
        raise ValueError("--azimuthal-smooth must be finite and >= 0, not %r" % (smooth,))
    for name, v in (("--azimuthal-damp", damp), ("--azimuthal-sigma", sigma)):
        if v is not None and not (np.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and > 0, not %r" % (name, v))


def maps_to_azimuthal(rows, c):
    """The A1, A2 columns of <input>Maps.dat (maps.read_maps of a file maps --azimuthal wrote) in maps_to_obs's layout: (a1, a2), both
    (nmaps, ny * nx) fp32, 0 on the outer ring.  ValueError as maps_to_obs, and when the rows carry no a1 / a2."""
    nx, ny = c["nx"], c["ny"]
    nvx, nvz = nx - 2, ny - 2
    layer = nvx * nvz
    per = maps.period_list(c)
    if len(rows) != len(per) * layer:
        raise ValueError("depth: the maps file holds %d lines, %d periods of %d x %d interior vertices need %d" % (len(rows), len(per), nvx, nvz, len(per) * layer))
    if any("a1" not in r or "a2" not in r for r in rows):
        raise ValueError("depth: the maps file has no a1 / a2 columns; write it with maps --azimuthal")
    out = np.zeros((2, len(per), ny, nx), np.float32)
    for m, (wave, kind, t) in enumerate(per):
        block = rows[m * layer:(m + 1) * layer]
        if any((r["wave"], r["kind"], r["period"]) != (wave, kind, t) for r in block):
            raise ValueError("depth: map %d of the maps file is not wave %d kind %d period %g of the input" % (m, wave, kind, t))
        for q, key in enumerate(("a1", "a2")):
            out[q, m, 1:-1, 1:-1] = np.array([r[key] for r in block]).reshape(nvz, nvx)
    return out[0].reshape(len(per), ny * nx), out[1].reshape(len(per), ny * nx)


def azimuthal_sigma(chi2, nused):
    """the rms of the weighted residual of the fit of A1 and A2 together: sqrt((chi2c_after + chi2s_after) / (2 sum nused)), 0 without data"""
    chi2 = np.asarray(chi2, np.float64)
    return rms_of(chi2[2] + chi2[3], 2 * np.asarray(nused, np.int64))


def azimuthal_sd_axis(gc, gs, sd_g):
    """the standard deviation of the fast axis in degrees, (90 / pi) sd_g / sqrt(gc^2 + gs^2), capped at SD_AXIS_CAP -- also where the
    amplitude is 0"""
    amp = np.hypot(np.asarray(gc, np.float64), np.asarray(gs, np.float64))
    sd = np.full(amp.shape, SD_AXIS_CAP)
    np.divide((90.0 / math.pi) * np.asarray(sd_g, np.float64), amp, out=sd, where=amp > 0)
    return np.minimum(sd, SD_AXIS_CAP)


def azimuthal_columns(res, sigma):
    """The node figures of DepthAzim.dat from columns_azimuthal's result and the standard deviation sigma of the weighted A1, A2: dict(strength,
    axis, rjj, length, sd_g, sd_strength, sd_axis), each (nz - 1, ny * nx).  Every root and atan2 is taken here."""
    from .analyses.azimuthal import azimuthal_axis, azimuthal_strength
    gc, gs, m = np.asarray(res["gc"], np.float64), np.asarray(res["gs"], np.float64), np.asarray(res["measures"], np.float64)
    sd_g = float(sigma) * np.sqrt(m[3])
    return dict(strength=azimuthal_strength(gc, gs), axis=azimuthal_axis(gc, gs), rjj=m[0], length=psf_length(m[1], m[2]), sd_g=sd_g, sd_strength=50.0 * sd_g,
                sd_axis=azimuthal_sd_axis(gc, gs, sd_g))


def write_azimuthal(path, c, vels, res, sigma):
    """<input>DepthAzim.dat: per node above the bottom depth (depth slowest, then j, then i) longitude, latitude, depth, Vs, gc, gs, the
    strength 50 sqrt(gc^2 + gs^2) in per cent of Vs, the fast axis 0.5 atan2(gs, gc) in degrees from north, R_jj, the vertical length of the
    point-spread function in km, sd_g = sigma sqrt(var), sd_strength = 50 sd_g and sd_axis (azimuthal_sd_axis)"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    v = np.asarray(vels, np.float64).reshape(nz, ny * nx)
    col = azimuthal_columns(res, sigma)
    io.write_table(path, AZIMUTHAL_TABLE, [dict(row, vs=v[k, q], gc=float(res["gc"][k, q]), gs=float(res["gs"][k, q]), **{n: float(a[k, q]) for n, a in col.items()})
                                           for k, q, row in _node_rows(c, nz - 1)])


def read_azimuthal(path):
    return io.read_table(path, AZIMUTHAL_TABLE)


def azimuthal_column_rms(chi2, nused):
    """per column the rms of (A1, A2) before and after: sqrt((chi2c + chi2s) / (2 nused)), 0 without data.  Returns (before, after)."""
    chi2 = np.asarray(chi2, np.float64); n = 2.0 * np.asarray(nused, np.float64)
    rms = lambda s: np.sqrt(np.divide(s, n, out=np.zeros(n.shape), where=n > 0))
    return rms(chi2[0] + chi2[1]), rms(chi2[2] + chi2[3])


def write_azimuthal_fit(path, c, res):
    """<input>DepthAzimFit.dat: per column (j, then i) longitude, latitude, the data used, the rms of (A1, A2) before and after, the flag"""
    r0, r1 = azimuthal_column_rms(res["chi2"], res["nused"])
    io.write_table(path, AZIMUTHAL_FIT_TABLE, [dict(row, nused=int(res["nused"][q]), rms_before=float(r0[q]), rms_after=float(r1[q]), flag=int(res["flag"][q]))
                                               for q, row in _column_rows(c)])


def read_azimuthal_fit(path):
    return io.read_table(path, AZIMUTHAL_FIT_TABLE)


def azimuthal_summary(c, res, sigma):
    """what the log says of columns_azimuthal's result: resolution_summary's entries (the trace is the sum of the R_jj), rms_before,
    rms_after over all columns, and over the nodes of the interior columns that are not flagged the median and the largest strength, the
    share whose amplitude exceeds 2 sd_g and the median R_jj per depth (None without such a column)"""
    m = np.asarray(res["measures"], np.float64)
    sm = resolution_summary(c, dict(res, trace=m[0].sum(axis=0)))
    chi2 = np.asarray(res["chi2"], np.float64)
    sm.update(rms_before=rms_of(chi2[0] + chi2[1], 2 * np.asarray(res["nused"], np.int64)), rms_after=azimuthal_sigma(chi2, res["nused"]), strength=None,
              significant=None, rjj=None)
    nx, ny = c["nx"], c["ny"]
    inner = np.zeros((ny, nx), bool); inner[1:-1, 1:-1] = True
    ok = inner.ravel() & (np.asarray(res["flag"]).reshape(ny * nx) == 0)
    if ok.any():
        col = azimuthal_columns(res, sigma)
        st = col["strength"][:, ok]
        sm["strength"] = (float(np.median(st)), float(st.max()))
        sm["significant"] = float((st / 50.0 > 2.0 * col["sd_g"][:, ok]).mean())
        sm["rjj"] = [float(x) for x in np.median(m[0][:, ok], axis=1)]
    return sm


def run_azimuthal(eng, c, plan, vels, obs, a1, a2, wt, smooth, damp, sigma, out_dir, log=print):
    """--azimuthal on an engine whose stage holds the final model vels: the runs of plan once more, columns_azimuthal, the two files, the log.
    sigma: the standard deviation of the weighted A1, A2, or None for the rms of the fit's residual.  Returns dict(azimuthal: the call's
    result, azimuthal_sigma, azimuthal_summary, azimuthal_path, azimuthal_fit_path)."""
    for wave, kind, t, first in plan:
        eng.dispersion_run(wave, kind, t, True, first, first)
    res = eng.columns_azimuthal(obs, a1, a2, wt, smooth, damp)
    own = sigma is None
    sigma = azimuthal_sigma(res["chi2"], res["nused"]) if own else float(sigma)
    apath = os.path.join(out_dir, "DSurfTomo.inDepthAzim.dat")
    fpath = os.path.join(out_dir, "DSurfTomo.inDepthAzimFit.dat")
    write_azimuthal(apath, c, vels, res, sigma)
    write_azimuthal_fit(fpath, c, res)
    sm = azimuthal_summary(c, res, sigma)
    log(" depth azimuthal: %d columns solved, %d flagged (%d not positive definite, %d without data), smooth %g damp %g" %
        (sm["columns"], sm["flagged1"] + sm["flagged2"], sm["flagged1"], sm["flagged2"], smooth, damp))
    log(" depth azimuthal: rms of (A1, A2) %.6f km/s before, %.6f km/s after; sigma %.6f km/s (%s)" %
        (sm["rms_before"], sm["rms_after"], sigma, "the rms of the fit's residual" if own else "--azimuthal-sigma"))
    if sm["strength"] is not None:
        log(" depth azimuthal: strength median %.4f %%, largest %.4f %% of Vs; the amplitude exceeds 2 sd_g at %.1f %% of the nodes" %
            (sm["strength"] + (100.0 * sm["significant"],)))
        log(" depth azimuthal: median R_jj per depth %s; the median R_jj %s" %
            (" ".join("%.4f" % x for x in sm["rjj"]), "stays under 0.1 from %g km down" % sm["depth"] if sm["depth"] is not None else "is 0.1 or more at the deepest unknown"))
    log(" depth azimuthal: written to %s, the fit to %s" % (apath, fpath))
    return dict(azimuthal=res, azimuthal_sigma=sigma, azimuthal_summary=sm, azimuthal_path=apath, azimuthal_fit_path=fpath)


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
    v0 = np.asarray(start, np.float64).reshape(nz, ny * nx)[:M]
    kept = (np.asarray(res["nkept"]).reshape(ny * nx) > 0)[None]
    grid = lambda a: np.asarray(a, np.float64).reshape(M, ny * nx)
    mean = np.where(kept, grid(res["mean"]), v0); best = np.where(kept, grid(res["best"]), v0)
    sd = np.where(kept, grid(sample_sd(res["var"])), 0.0)
    rhat = grid(sample_rhat(res["W"], res["B"], np.asarray(res["nkept"])[None]))
    io.write_table(path, POSTERIOR_TABLE, [dict(row, start=v0[k, q], mean=mean[k, q], sd=sd[k, q], best=best[k, q], rhat=rhat[k, q]) for k, q, row in _node_rows(c, M)])


def read_posterior(path):
    return io.read_table(path, POSTERIOR_TABLE)


def write_posterior_fit(path, c, res):
    """<input>DepthPosteriorFit.dat: per column (j, then i) the data used, phi of the start, the best phi + psi, the mean kept phi,
    the shares of the proposals (chains x sweeps) that were accepted, fell out of the box, lost a root; the chains put back; the flag"""
    total = np.asarray(res["accepted"], np.float64) + np.asarray(res["rejected"], np.float64)
    acc, oob, noroot = (_rate(res[n], total) for n in ("accepted", "out_of_box", "no_root"))
    io.write_table(path, POSTERIOR_FIT_TABLE, [dict(row, nused=int(res["nused"][q]), phi_start=float(res["phi_start"][q]), phi_best=float(res["best_energy"][q]),
                                                    phi_mean=float(res["mean_phi"][q]), accepted=float(acc[q]), out_of_box=float(oob[q]), no_root=float(noroot[q]),
                                                    reseeded=int(res["reseeded"][q]), flag=int(res["flag"][q])) for q, row in _column_rows(c)])


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
    M = c["nz"] - 1
    corr = sample_correlation(cov, M)
    rows = []
    for q, row in _column_rows(c):
        row.update(("r%d_%d" % (a, b), float(corr[a, b, q])) for a in range(M) for b in range(M))
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
    v = np.asarray(vsv, np.float64).reshape(nz, ny * nx); h = np.asarray(vsh, np.float64).reshape(nz, ny * nx)
    voigt, xi = voigt_xi(v, h)
    io.write_table(path, RADIAL_TABLE, [dict(row, vsv=v[k, q], vsh=h[k, q], voigt=voigt[k, q], xi=xi[k, q]) for k, q, row in _node_rows(c, nz)])


def read_radial(path):
    return io.read_table(path, RADIAL_TABLE)


def write_radial_fit(path, c, first, last):
    """<input>DepthRadialFit.dat: first / last = columns_step_radial's results of the first and the last iteration; one line per column, j then i"""
    nx, ny = c["nx"], c["ny"]
    col_rms = lambda s, q: np.sqrt(np.divide(s["chi2"][q], s["nused"][q], out=np.zeros(nx * ny), where=s["nused"][q] > 0))
    r = [[col_rms(first, q), col_rms(last, q)] for q in range(2)]
    io.write_table(path, RADIAL_FIT_TABLE, [dict(row, nused_r=int(last["nused"][0][q]), nused_l=int(last["nused"][1][q]), rms_first_r=float(r[0][0][q]),
                                                 rms_last_r=float(r[0][1][q]), rms_first_l=float(r[1][0][q]), rms_last_l=float(r[1][1][q]), flag=int(last["flag"][q]))
                                            for q, row in _column_rows(c)])


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
    io.write_table(path, RADIAL_RESOLUTION_TABLE, [dict(row, **{name: cols[name][k, q] for name in RADIAL_RESOLUTION_NAMES}) for k, q, row in _node_rows(c, nz - 1)])


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


# ---- the options, the stages and the driver ----

# every option once, in the command line's order: (flag, run()'s keyword, default, argparse's arguments); parser(), run() and main() read this
OPTIONS = (
    ("--maps", "maps_file", None, dict(metavar="FILE", help="the maps file of dsurftomo_amd.maps (default: DSurfTomo.inMaps.dat in --out)")),
    ("--iterations", "iterations", DEFAULT_ITERATIONS, dict(type=int, metavar="N")),
    ("--smooth", "smooth", DEFAULT_SMOOTH, dict(type=float, metavar="L", help="weight of the depth Laplacian (default %g)" % DEFAULT_SMOOTH)),
    ("--damp", "damp", DEFAULT_DAMP, dict(type=float, metavar="D", help="damping of a column's step, > 0 (default %g)" % DEFAULT_DAMP)),
    ("--dvmax", "dvmax", DEFAULT_DVMAX, dict(type=float, metavar="V", help="largest change of a node per iteration in km/s (default %g)" % DEFAULT_DVMAX)),
    ("--min-dws", "min_dws", 0.0, dict(type=float, metavar="X", help="map vertices whose column DWS is below X get weight 0 (default 0: all count)")),
    ("--out", "out_dir", ".", dict()),
    ("--resolution", "resolution", False, dict(action="store_true", help="after the last step write the resolution measures and the leverages of the final model")),
    ("--sigma", "sigma", None, dict(type=float, metavar="S", help="standard deviation of the map values in km/s for the sd column (default: the rms before the last step)")),
    ("--map-sigma", "map_sigma", None, dict(metavar="FILE", help="the MapsResolution.dat of maps --resolution: every map value weighs sigma_ref / sd, sigma_ref the median sd of the kept values (default: weights 0 / 1); without --sigma the stages' standard deviation is sigma_ref")),
    ("--radial", "radial", False, dict(action="store_true", help="radial anisotropy: invert the Rayleigh maps for Vsv(z) and the Love maps for Vsh(z) together")),
    ("--aniso", "aniso", DEFAULT_ANISO, dict(type=float, metavar="G", help="with --radial: weight of the tie between Vsh and Vsv, >= 0 (default %g)" % DEFAULT_ANISO)),
    ("--lateral", "lateral", None, dict(type=float, metavar="W", help="couple neighbouring columns: weight of the penalty on their differences, >= 0 (default: columns alone)")),
    ("--lateral-tol", "lateral_tol", DEFAULT_LATERAL_TOL, dict(type=float, metavar="T", help="with --lateral: relative tolerance of the conjugate gradients, > 0 (default %g)" % DEFAULT_LATERAL_TOL)),
    ("--lateral-maxit", "lateral_maxit", DEFAULT_LATERAL_MAXIT, dict(type=int, metavar="N", help="with --lateral: most conjugate-gradient iterations per step (default %d)" % DEFAULT_LATERAL_MAXIT)),
    ("--radial-lateral", "radial_lateral", None, dict(type=float, metavar="W", help="with --radial: couple neighbouring columns, weight of the penalty on the differences of Vsv and of Vsh, >= 0 (default: columns alone); --lateral-tol and --lateral-maxit apply")),
    ("--radial-lateral-aniso", "radial_lateral_aniso", None, dict(type=float, metavar="A", help="with --radial-lateral: weight of the penalty on the differences of Vsh - Vsv between neighbours, >= 0 (default: W)")),
    ("--radial-resolution", "radial_resolution", False, dict(action="store_true", help="with --radial: after the last step write the resolution measures of Vsv, Vsh and xi and the leverages of the final models (--sigma applies)")),
    ("--lateral-resolution", "lateral_resolution", False, dict(action="store_true", help="with --lateral: after the last step write the point-spread lengths, own shares and standard deviations of the coupled system (--sigma applies)")),
    ("--lateral-resolution-stride", "lateral_resolution_stride", 1, dict(type=int, metavar="N", help="with --lateral-resolution: resolve every N-th unknown (default 1: all)")),
    ("--lateral-checkerboard", "lateral_checkerboard", None, dict(metavar="NX,NY,NZ[,AMP]", help="with --lateral-resolution: recover a checkerboard of NX x NY x NZ blocks of amplitude AMP km/s (default %g)" % DEFAULT_CHECKER_AMP)),
    ("--azimuthal", "azimuthal", False, dict(action="store_true", help="after the last step invert the maps' 2psi terms A1(T), A2(T) (maps --azimuthal) of every column for gc(z), gs(z): strength, fast axis, resolution and standard deviations of the final model")),
    ("--azimuthal-smooth", "azimuthal_smooth", None, dict(type=float, metavar="L", help="with --azimuthal: weight of the depth Laplacian on gc and gs, >= 0 (default: --smooth)")),
    ("--azimuthal-damp", "azimuthal_damp", None, dict(type=float, metavar="D", help="with --azimuthal: damping of gc and gs, > 0 (default: --damp)")),
    ("--azimuthal-sigma", "azimuthal_sigma", None, dict(type=float, metavar="S", help="with --azimuthal: standard deviation of the A1, A2 values in km/s for the sd columns (default: the rms of the fit's residual)")),
    ("--sample", "sample", None, dict(metavar="C,SWEEPS[,BURN]", help="after the last step sample the posterior of every column with C Metropolis chains for SWEEPS sweeps, the first BURN (default SWEEPS / 2) left out (--sigma applies)")),
    ("--sample-step", "sample_step", DEFAULT_SAMPLE_STEP, dict(type=float, metavar="S", help="with --sample: half width of the single-node proposal in km/s (default %g)" % DEFAULT_SAMPLE_STEP)),
    ("--sample-spread", "sample_spread", DEFAULT_SAMPLE_SPREAD, dict(type=float, metavar="P", help="with --sample: half width of the scatter of the chains' starts in km/s (default %g)" % DEFAULT_SAMPLE_SPREAD)),
    ("--sample-width", "sample_width", DEFAULT_SAMPLE_WIDTH, dict(type=float, metavar="W", help="with --sample: half width of the prior box about the step's result in km/s (default %g)" % DEFAULT_SAMPLE_WIDTH)),
    ("--sample-seed", "sample_seed", DEFAULT_SAMPLE_SEED, dict(type=int, metavar="N", help="with --sample: seed of the counter-based generator (default %d)" % DEFAULT_SAMPLE_SEED)),
    ("--sample-temperature", "sample_temperature", DEFAULT_SAMPLE_TEMPERATURE, dict(type=float, metavar="T", help="with --sample: the chains sample exp(-(phi + psi) / 2T) (default %g)" % DEFAULT_SAMPLE_TEMPERATURE)),
    ("--sample-block", "sample_block", 0, dict(type=int, metavar="EVERY", help="with --sample: every EVERY-th sweep proposes all nodes of a column at once, along its linearised posterior (default 0: single nodes only)")),
    ("--sample-block-scale", "sample_block_scale", None, dict(type=float, metavar="S", help="with --sample-block: scale of the block proposal (default 2.38 sqrt(3 T / M) for M unknowns per column at temperature T)")),
    ("--sample-bins", "sample_bins", 0, dict(type=int, metavar="NB", help="with --sample: histogram every node's kept states in NB (2 to 256) equal bins of its box and write mode, quantiles and marginals (default 0: off)")),
    ("--sample-quantiles", "sample_quantiles", DEFAULT_SAMPLE_QUANTILES, dict(metavar="P1,P2,...", help="with --sample-bins: the levels of the quantiles, at most 16 inside (0, 1) (default %s)" % DEFAULT_SAMPLE_QUANTILES)),
    ("--sample-covariance", "sample_covariance", False, dict(action="store_true", help="with --sample-bins: also accumulate the covariance between the depths of a column and write their correlations")),
)
PLACES = ("maps_file", "out_dir")                   # run()'s own parameters among them; the others are its **options


def options_over_defaults(options):
    """run()'s **options over the defaults of OPTIONS, as a namespace; a name the table does not hold is a TypeError, like any unknown keyword"""
    o = {keyword: default for _, keyword, default, _ in OPTIONS if keyword not in PLACES}
    unknown = sorted(set(options) - set(o))
    if unknown:
        raise TypeError("run() got an unexpected keyword argument %r" % unknown[0])
    return types.SimpleNamespace(**dict(o, **options))


def check_options(o):
    """Every precondition on the options o (options_over_defaults'), in the one order run() and main() both refuse in (ValueError), before the
    library is loaded: --sample's, the marginals', then the loop's (aniso only with radial; --lateral-tol and --lateral-maxit only with a
    coupling), --lateral's, --radial's, --radial-lateral's, --radial-resolution's, --lateral-resolution's, --azimuthal's, then --map-sigma's file (its header names the needed columns).  Returns (parse_sample's tuple or
    None, check_marginals' tuple or None, the parsed --lateral-checkerboard or None)."""
    sampling = check_sample(o.sample, o.radial, o.lateral, o.sample_step, o.sample_spread, o.sample_width, o.sample_temperature, o.sample_seed, o.sample_block,
                            o.sample_block_scale)
    marginals = check_marginals(o.sample, o.sample_bins, o.sample_quantiles, o.sample_covariance)
    tol, maxit = (o.lateral_tol, o.lateral_maxit) if o.lateral is not None or o.radial_lateral is not None else (None, None)
    check(o.iterations, o.smooth, o.damp, o.dvmax, o.min_dws, o.sigma, o.aniso if o.radial else None, o.lateral, tol, maxit, o.radial_lateral, o.radial_lateral_aniso)
    if o.lateral is not None:
        check_lateral(o.radial, o.resolution)
    if o.radial:
        check_radial(None, o.resolution)
    check_radial_lateral(o.radial_lateral, o.radial_lateral_aniso, o.radial, o.lateral, o.resolution)
    check_radial_resolution(o.radial_resolution, o.radial, o.radial_lateral)
    checker = check_lateral_resolution(o.lateral_resolution, o.lateral_resolution_stride, o.lateral_checkerboard, o.lateral, o.radial)
    check_azimuthal(o.azimuthal, o.radial, o.azimuthal_smooth, o.azimuthal_damp, o.azimuthal_sigma)
    if o.map_sigma is not None:
        maps.resolution_header(o.map_sigma, o.azimuthal)
    return sampling, marginals, checker


def stage_sigma(label, sigma, history, log, sigma_ref=None):
    """the data's standard deviation of an after-loop stage: --sigma, or with --map-sigma its sigma_ref (the weights are sigma_ref / sd: a
    datum of weight w then has the standard deviation sigma_ref / w = its sd), or the rms before the last step; the log says which"""
    rms = history[-1]["rms"]
    if sigma is None and sigma_ref is not None:
        log(" %s: the data's standard deviation is --map-sigma's reference, the median sd of the kept map values, %.6f km/s (the weighted rms before the last step was %.6f)" %
            (label, sigma_ref, rms))
        return sigma_ref
    log(" %s: the data's standard deviation is %s" % (label, "--sigma %.6f km/s" % sigma if sigma is not None else "the rms before the last step, %.6f km/s" % rms))
    return rms if sigma is None else sigma


# the stages after the loop, in the order they run: (the label of their log lines, the path: radial or not, wanted(o), call(r, o, sigma) -> the
# entries the result gains); r: what run() holds (eng, c, plan, obs, wt, out_dir, log, out: the loop's result, sampling, marginals, checker,
# azi: (a1, a2) or None).  A label of None: the stage has a sigma of its own and stage_sigma is not asked (sigma None).  "depth sample" leaves
# the stage in sample mode, which refuses the column calls: it comes last on its path.
STAGES = (
    ("depth resolution", False, lambda o: o.resolution, lambda r, o, sigma: resolve(r.eng, r.c, r.plan, r.obs, r.wt, o.smooth, o.damp, sigma, r.out_dir, r.log)),
    ("depth lateral resolution", False, lambda o: o.lateral_resolution,
     lambda r, o, sigma: resolve_lateral(r.eng, r.c, r.plan, r.obs, r.wt, o.smooth, o.damp, o.lateral, o.lateral_tol, o.lateral_maxit, sigma, r.out_dir,
                                         o.lateral_resolution_stride, r.checker, r.log)),
    (None, False, lambda o: o.azimuthal,
     lambda r, o, sigma: run_azimuthal(r.eng, r.c, r.plan, r.out["vels"], r.obs, r.azi[0], r.azi[1], r.wt if r.wt_azi is None else r.wt_azi, o.smooth if o.azimuthal_smooth is None else o.azimuthal_smooth,
                                       o.damp if o.azimuthal_damp is None else o.azimuthal_damp, o.azimuthal_sigma, r.out_dir, r.log)),
    ("depth sample", False, lambda o: o.sample is not None,
     lambda r, o, sigma: run_sample(r.eng, r.c, r.plan, r.out["vels"], r.obs, r.wt, o.smooth, sigma, r.sampling, r.out_dir, o.sample_step, o.sample_spread, o.sample_width,
                                    o.sample_seed, o.sample_temperature, r.log, o.sample_block, o.sample_block_scale, o.damp, r.marginals)),
    ("depth radial resolution", True, lambda o: o.radial_resolution,
     lambda r, o, sigma: resolve_radial(r.eng, r.c, r.plan, r.obs, r.wt, o.smooth, o.damp, o.aniso, sigma, r.out_dir, r.log)),
)


def run(directory, maps_file=None, out_dir=".", log=print, **options):
    """the driver behind main(); options: the keywords of OPTIONS over its defaults.  Returns (iterate's result with vels (nz, ny, nx) added,
    the paths of Depth.dat and DepthFit.dat).  With resolution the first item also holds resolve's entries (resolution_path and leverage_path
    among them); sigma None: the rms before the last step.  With radial: run_radial's result (DepthRadial.dat and DepthRadialFit.dat in place
    of the two files).  With lateral (not None): the loop steps with columns_step_lateral; the files are the same two.  With radial and
    radial_lateral (not None): the radial loop steps with columns_step_radial_lateral, radial_lateral_aniso (None: radial_lateral) the
    weight on Vsh - Vsv; the files are --radial's.  With radial and radial_resolution: after the loop resolve_radial's entries are added to
    the first item (DepthRadialResolution.dat and DepthRadialLeverage.dat beside --radial's files); sigma as with resolution.  With lateral
    and lateral_resolution: after the loop resolve_lateral's entries are added to the first item (DepthLateralResolution.dat and, with
    lateral_checkerboard, DepthLateralChecker.dat beside the two files); sigma as with resolution.  With sample ("C,SWEEPS[,BURN]"): after
    the loop (and the resolution) run_sample's entries are added to the first item (DepthPosterior.dat and DepthPosteriorFit.dat beside the
    two files); sigma as with resolution; sample_block (EVERY > 0) makes every EVERY-th sweep a block proposal of scale sample_block_scale
    (None: sample_block_scale(nz - 1, temperature)); sample_bins (2 .. 256) adds the posterior marginals at the levels sample_quantiles
    ("P1,P2,...") and, with sample_covariance, the correlations between a column's depths (run_sample's three files).  With azimuthal: after
    the resolutions and before the sample stage run_azimuthal's entries are added to the first item (DepthAzim.dat and DepthAzimFit.dat beside
    the two files); azimuthal_smooth / azimuthal_damp None: smooth / damp; azimuthal_sigma None: the rms of the fit's residual; a maps file
    without a1 / a2 columns is a ValueError naming it, before the library is loaded.  With map_sigma (the MapsResolution.dat of maps
    --resolution): every stage's wt is map_sigma_weights' sigma_ref / sd under the --min-dws mask, the 2psi stage's its own from the sd of A1
    and A2, and without sigma the stages take sigma_ref, so that the sampler's weights are 1 / sd; a file without the needed columns is a
    ValueError naming it, before the library is loaded.  The radial path writes
    its two files in run_radial, before its stage; the isotropic path writes Depth.dat and DepthFit.dat after its stages, the engine closed."""
    o = options_over_defaults(options)
    sampling, marginals, checker = check_options(o)
    c = io.load(directory)
    if o.radial:
        check_radial(c)
    maps_file = os.path.join(out_dir, "DSurfTomo.inMaps.dat") if maps_file is None else maps_file
    rows = maps.read_maps(maps_file)
    obs, dws = maps_to_obs(rows, c)
    if o.azimuthal and not (rows and "a1" in rows[0] and "a2" in rows[0]):
        raise ValueError("depth: --azimuthal needs the a1 and a2 columns, which %s does not have; write it with maps --azimuthal" % maps_file)
    azi = maps_to_azimuthal(rows, c) if o.azimuthal else None
    plan = slot_plan(c)
    kmax = c["kmax"]
    if not plan or kmax > 60:
        raise ValueError("depth: %d periods; the step takes 1 to 60" % kmax)
    wt = dws_weights(dws, o.min_dws) if o.min_dws > 0 else None
    wt_azi = sigma_ref = None
    if o.map_sigma is not None:
        sd_rows = maps.read_maps_resolution(o.map_sigma, o.azimuthal)
        mask = None if wt is None else wt > 0
        wt, sigma_ref = map_sigma_weights(sd_rows, c, mask)
        log(" depth: weights sigma_ref / sd from %s: sigma_ref %.6f km/s, %d of %d map values kept, weights %.4f to %.4f" %
            (o.map_sigma, sigma_ref, int((wt > 0).sum()), kmax * (c["nx"] - 2) * (c["ny"] - 2), float(wt[wt > 0].min()) if (wt > 0).any() else 0.0, float(wt.max())))
        if wt.max() > 10.0:
            log(" depth: weights above 10 belong to map values the rays hardly resolve -- damping pulls them to the start and their variance with them; --min-dws masks them")
        if o.azimuthal:
            wt_azi, azi_ref = map_sigma_weights(sd_rows, c, mask, azimuthal=True)
            log(" depth: weights of the 2psi stage from sqrt((sd_a1^2 + sd_a2^2) / 2): reference %.6f km/s, %d values kept" % (azi_ref, int((wt_azi > 0).sum())))
    from .engine import Engine
    r = types.SimpleNamespace(eng=Engine(0), c=c, plan=plan, obs=obs, wt=wt, out_dir=out_dir, log=log, sampling=sampling, marginals=marginals, checker=checker, azi=azi,
                              wt_azi=wt_azi)
    try:
        if o.radial:
            r.out, path, fit = run_radial(r.eng, c, plan, obs, wt, o.iterations, o.smooth, o.damp, o.aniso, o.dvmax, out_dir, log, o.radial_lateral, o.radial_lateral_aniso,
                                          o.lateral_tol, o.lateral_maxit)
        else:
            r.eng.dispersion_begin(np.ascontiguousarray(np.asarray(c["vels"], np.float32).transpose(2, 1, 0)), c["depz"], c["minthk"], kmax, kmax)
            r.out = iterate(r.eng, plan, obs, wt, o.iterations, o.smooth, o.damp, o.dvmax, float(c["minvel"]), float(c["maxvel"]), log, o.lateral, o.lateral_tol, o.lateral_maxit)
            r.out["vels"] = r.eng.dispersion_get_model()
        for label, radial, wanted, call in STAGES:
            if radial == o.radial and wanted(o):
                r.out.update(call(r, o, None if label is None else stage_sigma(label, o.sigma, r.out["history"], log, sigma_ref)))
    finally:
        r.eng.close()
    if not o.radial:
        path = os.path.join(out_dir, "DSurfTomo.inDepth.dat")
        fit = os.path.join(out_dir, "DSurfTomo.inDepthFit.dat")
        write_depth(path, c, r.out["vels"])
        write_fit(fit, c, r.out["steps"][0], r.out["steps"][-1])
        log(" depth: %d x %d x %d nodes written to %s, the fit of %d columns to %s" % (c["nx"], c["ny"], c["nz"], path, c["nx"] * c["ny"], fit))
    return r.out, path, fit


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    for flag, _, default, arguments in OPTIONS:
        ap.add_argument(flag, default=default, **arguments)
    return ap


def main(argv=None):
    ap = parser()
    a = vars(ap.parse_args(argv))
    options = {keyword: a[flag[2:].replace("-", "_")] for flag, keyword, _, _ in OPTIONS}
    places = {keyword: options.pop(keyword) for keyword in PLACES}
    try:
        check_options(options_over_defaults(options))
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(places["out_dir"], exist_ok=True)
    run(a["directory"], **places, **options)
    return 0


if __name__ == "__main__":
    sys.exit(main())
