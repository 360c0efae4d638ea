"""Monte-Carlo radial depth inversion: the posterior of Vsv(z), Vsh(z) and xi = (Vsh / Vsv)^2 of every column.

    python -m dsurftomo_amd.radial_posterior <dir> --sample C,SWEEPS[,BURN]
        [--maps FILE] [--model FILE] [--smooth L] [--aniso G] [--sigma S] [--min-dws X] [--map-sigma FILE] [--sample-step S]
        [--sample-spread P] [--sample-width W] [--sample-seed N] [--sample-temperature T] [--no-pairs] [--out DIR]

<dir> holds DSurfTomo.in and its data, as for dsurftomo_amd.depth.  The chains start from the DepthRadial.dat that `depth --radial` wrote
(--model; default: that file in --out); the maps, the slots, the --min-dws mask and the --map-sigma weights are depth's.  C Metropolis chains
of [Vsv ; Vsh] per interior column run SWEEPS sweeps on the device (dsa_columns_sample_radial_*), the first BURN (default SWEEPS / 2) left
out: a Rayleigh map is computed on a chain's Vsv, a Love map on its Vsh; the prior is depth --radial's -- smooth on each model's depth
Laplacian, aniso on Vsh - Vsv -- inside a box of half width --sample-width about each model's start.  A proposal moves one Vsv node, one
Vsh node or (unless --no-pairs) the two of one depth together.

sigma, the data's standard deviation in km/s, is --sigma, or --map-sigma's reference, or the weighted rms of obs - pv of the start, which one
radial dispersion stage computes; the log says which.  The weights are 1 / sigma where the mask keeps a datum (with --map-sigma: 1 / sd) and
smooth and aniso are both divided by sigma, so that phi is the chi-square of the data and the prior keeps the balance it had in the step.

<input>DepthRadialPosterior.dat, per node above the bottom depth: lon, lat, depth; start, mean, sd, best and R-hat of Vsv; the same of Vsh;
xi of the start, mean, sd and R-hat of xi; the correlation of Vsv and Vsh; the sd of Vsh - Vsv; P(Vsh > Vsv).  <input>DepthRadialPosteriorFit.dat,
per column: nused_r, nused_l; phi of the start, the best phi + psi, the mean kept phi; the shares of the proposals accepted, out of the box,
without a root; the acceptance per kind of proposal; reseeded, flag.  Both with 17 significant digits.  column_sample_radial_twin
(depth_twins) is the Python twin of the arithmetic, csrc/column_sample_radial.h."""
import argparse
import math
import os
import sys

import numpy as np

from . import depth, io, maps
from .depth_twins import column_sample_radial_twin, sample_rhat, sample_sd        # noqa: F401 (the twin is reached as radial_posterior.<name>)

_F64 = depth._F64
POSTERIOR_TABLE = (True, _F64("lon", "lat", "depth", "vsv_start", "vsv_mean", "vsv_sd", "vsv_best", "vsv_rhat", "vsh_start", "vsh_mean", "vsh_sd", "vsh_best", "vsh_rhat",
                              "xi_start", "xi_mean", "xi_sd", "xi_rhat", "corr", "sd_diff", "p_pos"))
FIT_TABLE = (True, _F64("lon", "lat") + (("nused_r", "%d", "int"), ("nused_l", "%d", "int")) +
             _F64("phi_start", "phi_best", "phi_mean", "accepted", "out_of_box", "no_root", "accepted_v", "accepted_h", "accepted_pair") +
             (("reseeded", "%d", "int"), ("flag", "%d", "int")))
KINDS = ("v", "h", "pair")


def check(sample=None, smooth=None, aniso=None, sigma=None, min_dws=None, step=None, spread=None, width=None, temperature=None, seed=None, map_sigma=None):
    """every refusal of the command line, before the library is loaded (ValueError).  Returns depth.parse_sample's tuple."""
    if sample is None:
        raise ValueError("--sample C,SWEEPS[,BURN] is required")
    parsed = depth.check_sample(sample, False, None, step, spread, width, temperature, seed)
    for name, v in (("--smooth", smooth), ("--aniso", aniso), ("--min-dws", min_dws)):
        if v is not None and not (np.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and >= 0, not %r" % (name, v))
    if sigma is not None and not (np.isfinite(sigma) and sigma > 0):
        raise ValueError("--sigma must be finite and > 0, not %r" % (sigma,))
    if map_sigma is not None:
        maps.resolution_header(map_sigma, False)
    return parsed


def sample_scaling(wt, smooth, aniso, sigma, shape):
    """depth.sample_scaling with the tie beside the smoothing: (wt / sigma (1 / sigma where wt is None), smooth / sigma, aniso / sigma)"""
    w, lam = depth.sample_scaling(wt, smooth, sigma, shape)
    return w, lam, float(aniso) / float(sigma)


def start_sigma(eng, c, plan, vsv, vsh, obs, wt):
    """the weighted rms of obs - pv of the start over the data the sampler will use: one radial stage, the plan's runs (times only), a fetch"""
    kmax = c["kmax"]
    eng.dispersion_begin_radial(vsv, vsh, c["depz"], c["minthk"], kmax, kmax)
    for wave, kind, t, first in plan:
        eng.dispersion_run(wave, kind, t, False, 0, first)
    pv = eng.dispersion_fetch(0, kmax, False, 0)
    o = np.asarray(obs, np.float64).reshape(kmax, -1)
    w = np.ones(o.shape) if wt is None else np.asarray(wt, np.float64).reshape(o.shape)
    inner = np.zeros((c["ny"], c["nx"]), bool); inner[1:-1, 1:-1] = True
    used = (w > 0) & (o > 0) & (pv > 0) & inner.ravel()[None]
    n = int(used.sum())
    if n == 0:
        raise ValueError("radial_posterior: no datum is used at the start; give --sigma")
    return math.sqrt(float(((w * (o - pv))[used] ** 2).sum()) / n), n


def posterior_columns(start_v, start_h, res):
    """the node columns of DepthRadialPosterior.dat from the starts (M, ncol) and columns_sample_radial_fetch's result: every root is taken here
    (sample_sd, sample_rhat).  Where no sweep was kept mean and best are the start, the sds 0, R-hat 1, corr 0 and p_pos 0."""
    v0 = np.asarray(start_v, np.float64); h0 = np.asarray(start_h, np.float64)
    n = np.asarray(res["nkept"])[None]
    kept = n > 0
    xi0 = depth.voigt_xi(v0, h0)[1]
    out = {}
    for t, name, s0 in (("v", "vsv", v0), ("h", "vsh", h0), ("xi", "xi", xi0)):
        out[name + "_start"] = s0
        out[name + "_mean"] = np.where(kept, res["mean_" + t], s0)
        out[name + "_sd"] = np.where(kept, sample_sd(res["var_" + t]), 0.0)
        out[name + "_rhat"] = sample_rhat(res["W_" + t], res["B_" + t], n)
    out["vsv_best"] = np.where(kept, res["best_v"], v0); out["vsh_best"] = np.where(kept, res["best_h"], h0)
    prod = out["vsv_sd"] * out["vsh_sd"]
    out["corr"] = np.divide(res["cov_vh"], prod, out=np.zeros(prod.shape), where=prod > 0)
    out["sd_diff"] = sample_sd(res["var_v"] + res["var_h"] - 2.0 * res["cov_vh"]) * kept
    out["p_pos"] = np.asarray(res["p_pos"], np.float64)
    return out


def write_posterior(path, c, vsv, vsh, res):
    """<input>DepthRadialPosterior.dat: the starts (nz, ny, nx) and columns_sample_radial_fetch's result; every node above the bottom depth:
    depth slowest, then j, then i"""
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    M = nz - 1
    cols = posterior_columns(np.asarray(vsv).reshape(nz, ny * nx)[:M], np.asarray(vsh).reshape(nz, ny * nx)[:M], res)
    names = [n for n, _, _ in POSTERIOR_TABLE[1][3:]]
    io.write_table(path, POSTERIOR_TABLE, [dict(row, **{n: float(cols[n][k, q]) for n in names}) for k, q, row in depth._node_rows(c, M)])


def read_posterior(path):
    return io.read_table(path, POSTERIOR_TABLE)


def kind_rates(res):
    """the acceptance per kind of proposal of every column: dict(v, h, pair) of accepted / proposed (0 where none was proposed)"""
    return {k: depth._rate(res["accepted_" + k], np.asarray(res["proposed_" + k], np.float64)) for k in KINDS}


def write_posterior_fit(path, c, res):
    """<input>DepthRadialPosteriorFit.dat: per column (j, then i) the Rayleigh and Love data used, phi of the start, the best phi + psi, the
    mean kept phi, the shares of the proposals (chains x sweeps) accepted, out of the box, without a root, the acceptance of the Vsv, Vsh and
    pair proposals, the chains put back, the flag"""
    total = np.asarray(res["accepted"], np.float64) + np.asarray(res["rejected"], np.float64)
    acc, oob, noroot = (depth._rate(res[n], total) for n in ("accepted", "out_of_box", "no_root"))
    kr = kind_rates(res)
    io.write_table(path, FIT_TABLE, [dict(row, nused_r=int(res["nused_r"][q]), nused_l=int(res["nused_l"][q]), phi_start=float(res["phi_start"][q]),
                                          phi_best=float(res["best_energy"][q]), phi_mean=float(res["mean_phi"][q]), accepted=float(acc[q]), out_of_box=float(oob[q]),
                                          no_root=float(noroot[q]), accepted_v=float(kr["v"][q]), accepted_h=float(kr["h"][q]), accepted_pair=float(kr["pair"][q]),
                                          reseeded=int(res["reseeded"][q]), flag=int(res["flag"][q])) for q, row in depth._column_rows(c)])


def read_posterior_fit(path):
    return io.read_table(path, FIT_TABLE)


def summary(res):
    """what the log says: dict(rhat: {v, h, xi: dict(median, worst)}, unknowns, above: the share of the unknowns (Vsv and Vsh nodes) with
    R-hat above 1.1, accepted: {v, h, pair}, sure: the share of nodes with P(Vsh > Vsv) outside [0.025, 0.975]) over the columns with a kept
    sweep, or None without one"""
    kept = np.asarray(res["nkept"]) > 0
    if not kept.any():
        return None
    n = np.asarray(res["nkept"])[None]
    r = {t: sample_rhat(res["W_" + t], res["B_" + t], n)[:, kept] for t in ("v", "h", "xi")}
    unknowns = np.concatenate([r["v"].ravel(), r["h"].ravel()])
    p = np.asarray(res["p_pos"])[:, kept]
    return dict(rhat={t: dict(median=float(np.median(r[t])), worst=float(r[t].max())) for t in r}, unknowns=int(unknowns.size), above=float((unknowns > 1.1).mean()),
                accepted={k: float(depth._rate(float(res["accepted_" + k].sum()), float(res["proposed_" + k].sum()))) for k in KINDS},
                sure=float(((p < 0.025) | (p > 0.975)).mean()))


def read_start(path, c):
    """Vsv, Vsh (nz, ny, nx) fp32 from a DepthRadial.dat of c's grid (ValueError when it holds another number of nodes)"""
    rows = depth.read_radial(path)
    nx, ny, nz = c["nx"], c["ny"], c["nz"]
    if len(rows) != nx * ny * nz:
        raise ValueError("radial_posterior: %s holds %d nodes, the input's grid %d x %d x %d" % (path, len(rows), nx, ny, nz))
    grid = lambda name: np.ascontiguousarray(np.array([r[name] for r in rows], np.float64).reshape(nz, ny, nx), np.float32)
    return grid("vsv"), grid("vsh")


def run(directory, sample, maps_file=None, model_file=None, out_dir=".", smooth=depth.DEFAULT_SMOOTH, aniso=depth.DEFAULT_ANISO, sigma=None, min_dws=0.0,
        map_sigma=None, sample_step=depth.DEFAULT_SAMPLE_STEP, sample_spread=depth.DEFAULT_SAMPLE_SPREAD, sample_width=depth.DEFAULT_SAMPLE_WIDTH,
        sample_seed=depth.DEFAULT_SAMPLE_SEED, sample_temperature=depth.DEFAULT_SAMPLE_TEMPERATURE, pairs=True, log=print):
    """the driver behind main().  Returns dict(posterior: columns_sample_radial_fetch's result, sample_sigma, summary, posterior_path,
    posterior_fit_path)."""
    chains, sweeps, burn = check(sample, smooth, aniso, sigma, min_dws, sample_step, sample_spread, sample_width, sample_temperature, sample_seed, map_sigma)
    c = io.load(directory)
    depth.check_radial(c)
    if not float(c["minvel"]) > 0:
        raise ValueError("radial_posterior: the input's minvel %g must be > 0 (xi divides by Vsv)" % float(c["minvel"]))
    maps_file = os.path.join(out_dir, "DSurfTomo.inMaps.dat") if maps_file is None else maps_file
    model_file = os.path.join(out_dir, "DSurfTomo.inDepthRadial.dat") if model_file is None else model_file
    obs, dws = depth.maps_to_obs(maps.read_maps(maps_file), c)
    plan = depth.slot_plan(c)
    kmax = c["kmax"]
    if not plan or kmax > 60:
        raise ValueError("radial_posterior: %d periods; the sampler takes 1 to 60" % kmax)
    vsv, vsh = read_start(model_file, c)
    wt = depth.dws_weights(dws, min_dws) if min_dws > 0 else None
    sigma_ref = None
    if map_sigma is not None:
        wt, sigma_ref = depth.map_sigma_weights(maps.read_maps_resolution(map_sigma, False), c, None if wt is None else wt > 0)
    from .engine import Engine
    eng = Engine(0)
    try:
        if sigma is not None:
            log(" radial posterior: the data's standard deviation is --sigma %.6f km/s" % sigma)
        elif sigma_ref is not None:
            sigma = sigma_ref
            log(" radial posterior: the data's standard deviation is --map-sigma's reference, the median sd of the kept map values, %.6f km/s" % sigma)
        else:
            sigma, n = start_sigma(eng, c, plan, vsv, vsh, obs, wt)
            log(" radial posterior: the data's standard deviation is the weighted rms of the start over %d data, %.6f km/s" % (n, sigma))
        w, lam, gam = sample_scaling(wt, smooth, aniso, sigma, np.shape(obs))
        eng.columns_sample_radial_begin(vsv, vsh, c["depz"], c["minthk"], plan, obs, w, chains, lam, gam, sample_step, sample_spread, sample_width, sample_temperature,
                                        float(c["minvel"]), float(c["maxvel"]), sample_seed, burn, pairs)
        eng.columns_sample_radial_run(sweeps)
        res = eng.columns_sample_radial_fetch()
    finally:
        eng.close()
    ppath = os.path.join(out_dir, "DSurfTomo.inDepthRadialPosterior.dat")
    fpath = os.path.join(out_dir, "DSurfTomo.inDepthRadialPosteriorFit.dat")
    write_posterior(ppath, c, vsv, vsh, res)
    write_posterior_fit(fpath, c, res)
    moved = res["nkept"] > 0
    tried = float(res["accepted"].sum() + res["rejected"].sum())
    log(" radial posterior: %d chains x %d sweeps (%d kept) on %d columns, %d columns without data, %d chains put back at the set-up, pair proposals %s" %
        (chains, sweeps, sweeps - burn, int(moved.sum()), int((res["flag"] == 2).sum()), int(res["reseeded"].sum()), "on" if pairs else "off"))
    if tried > 0:
        log(" radial posterior: %.1f %% of the proposals accepted, %.1f %% out of the box, %.1f %% without a root" %
            tuple(100.0 * float(res[n].sum()) / tried for n in ("accepted", "out_of_box", "no_root")))
    if moved.any():
        log(" radial posterior: phi per column from %.4g at the start to %.4g on average over the kept sweeps (median over the columns)" %
            (float(np.median(res["phi_start"][moved])), float(np.median(res["mean_phi"][moved]))))
    sm = summary(res)
    if sm is not None:
        log(" radial posterior: R-hat median / worst: Vsv %.4f / %.4f, Vsh %.4f / %.4f, xi %.4f / %.4f; %.1f %% of %d unknowns above 1.1" %
            (sm["rhat"]["v"]["median"], sm["rhat"]["v"]["worst"], sm["rhat"]["h"]["median"], sm["rhat"]["h"]["worst"], sm["rhat"]["xi"]["median"], sm["rhat"]["xi"]["worst"],
             100.0 * sm["above"], sm["unknowns"]))
        log(" radial posterior: accepted %.1f %% of the Vsv, %.1f %% of the Vsh and %.1f %% of the pair proposals" % tuple(100.0 * sm["accepted"][k] for k in KINDS))
        log(" radial posterior: P(Vsh > Vsv) is outside [0.025, 0.975] at %.1f %% of the nodes" % (100.0 * sm["sure"]))
    log(" radial posterior: the posterior written to %s, the fit of the columns to %s" % (ppath, fpath))
    return dict(posterior=res, sample_sigma=float(sigma), summary=sm, posterior_path=ppath, posterior_fit_path=fpath)


def parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("directory")
    ap.add_argument("--sample", default=None, metavar="C,SWEEPS[,BURN]", help="C Metropolis chains for SWEEPS sweeps, the first BURN (default SWEEPS / 2) left out")
    ap.add_argument("--maps", default=None, metavar="FILE", help="the maps file of dsurftomo_amd.maps (default: DSurfTomo.inMaps.dat in --out)")
    ap.add_argument("--model", default=None, metavar="FILE", help="the DepthRadial.dat of depth --radial the chains start from (default: DSurfTomo.inDepthRadial.dat in --out)")
    ap.add_argument("--smooth", type=float, default=depth.DEFAULT_SMOOTH, metavar="L", help="weight of the depth Laplacian of each model (default %g)" % depth.DEFAULT_SMOOTH)
    ap.add_argument("--aniso", type=float, default=depth.DEFAULT_ANISO, metavar="G", help="weight of the tie between Vsh and Vsv, >= 0 (default %g)" % depth.DEFAULT_ANISO)
    ap.add_argument("--sigma", type=float, default=None, metavar="S", help="standard deviation of the map values in km/s (default: --map-sigma's reference, else the rms of the start)")
    ap.add_argument("--min-dws", type=float, default=0.0, metavar="X", help="map vertices whose column DWS is below X get weight 0 (default 0: all count)")
    ap.add_argument("--map-sigma", default=None, metavar="FILE", help="the MapsResolution.dat of maps --resolution: every map value weighs sigma_ref / sd")
    ap.add_argument("--sample-step", type=float, default=depth.DEFAULT_SAMPLE_STEP, metavar="S", help="half width of a proposal in km/s (default %g)" % depth.DEFAULT_SAMPLE_STEP)
    ap.add_argument("--sample-spread", type=float, default=depth.DEFAULT_SAMPLE_SPREAD, metavar="P", help="half width of the scatter of the chains' starts in km/s (default %g)" % depth.DEFAULT_SAMPLE_SPREAD)
    ap.add_argument("--sample-width", type=float, default=depth.DEFAULT_SAMPLE_WIDTH, metavar="W", help="half width of the prior box about each model's start in km/s (default %g)" % depth.DEFAULT_SAMPLE_WIDTH)
    ap.add_argument("--sample-seed", type=int, default=depth.DEFAULT_SAMPLE_SEED, metavar="N", help="seed of the counter-based generator (default %d)" % depth.DEFAULT_SAMPLE_SEED)
    ap.add_argument("--sample-temperature", type=float, default=depth.DEFAULT_SAMPLE_TEMPERATURE, metavar="T", help="the chains sample exp(-(phi + psi) / 2T) (default %g)" % depth.DEFAULT_SAMPLE_TEMPERATURE)
    ap.add_argument("--no-pairs", action="store_true", help="propose single Vsv and Vsh nodes only (default: a third of the proposals move the two of one depth together)")
    ap.add_argument("--out", default=".", metavar="DIR")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    try:
        check(a.sample, a.smooth, a.aniso, a.sigma, a.min_dws, a.sample_step, a.sample_spread, a.sample_width, a.sample_temperature, a.sample_seed, a.map_sigma)
    except ValueError as exc:
        ap.error(str(exc))
    os.makedirs(a.out, exist_ok=True)
    run(a.directory, a.sample, a.maps, a.model, a.out, a.smooth, a.aniso, a.sigma, a.min_dws, a.map_sigma, a.sample_step, a.sample_spread, a.sample_width, a.sample_seed,
        a.sample_temperature, not a.no_pairs)
    return 0


if __name__ == "__main__":
    sys.exit(main())
