"""The posterior marginals of the Monte-Carlo depth inversion (dsurftomo_amd/csrc/column_sample.h) on the CPU through
tests/hostcheck_column_sample_marginals.cpp: the bin rule against its NumPy twin at every edge, the header's counts, products and finish
against depth.SampleMarginalTwin beside depth.column_sample_twin bit for bit, with and without block sweeps, the bits of the sampler's own
state with the marginals on, the laws the figures obey, and the stand-alone program."""
import subprocess

import numpy as np
import pytest

import column_sample_marginals_ref as G
import column_sample_ref as R
import test_hostcheck_column_sample as T29
import test_hostcheck_column_sample_block as T32
from dsurftomo_amd import depth

F = np.float32
same_bits = T29.same_bits
linear_case = T29.linear_case
NARROW = T32.NARROW
LEVELS = G.LEVELS


@pytest.fixture(scope="module")
def h():
    return G.load()


def marginal_stage(h, start, obs, wt, C, nx=3, ny=3, smooth=10.0, step=0.05, spread=0.05, temperature=1.0, seed=77, burn=0, width=5.0, minvel=0.0, maxvel=10.0,
                   shape=None, block_every=0, block_scale=None, nbins=0, with_cov=False):
    M = start.shape[0] - 1
    scale = depth.sample_block_scale(M, float(F(temperature))) if block_scale is None else block_scale
    return G.MarginalStage(h, nx, ny, start, obs, wt, C, smooth, step, spread, width, temperature, minvel, maxvel, seed, burn, shape, block_every, scale, nbins=nbins,
                           with_cov=with_cov)


# ---- 1. the bin rule ----

@pytest.mark.parametrize("nbins", [2, 7, 256])
def test_bin_rule_equals_the_twin_at_every_edge(h, nbins):
    M, K = 3, 2
    start, obs, wt, pv0, A = linear_case(M, K)
    start[0, 4], start[1, 4], start[2, 4] = F(3.25), F(3.0), F(3.45)
    a = dict(width=0.15, minvel=3.0, maxvel=3.5)
    st = marginal_stage(h, start, obs, wt, 2, nbins=nbins, **a)
    lo, hi = depth.sample_box(start[:M], a["width"], a["minvel"], a["maxvel"])
    c = 4
    assert lo[1, c] == F(3.0) and hi[2, c] == F(3.5) and lo[0, c] == F(3.25) - F(0.15) and hi[0, c] == F(3.25) + F(0.15)         # a box cut by minvel, one by maxvel, one by neither
    for l in range(M):
        dlo, w = float(lo[l, c]), float(hi[l, c]) - float(lo[l, c])
        edges = (dlo + (np.arange(1, nbins) / nbins) * w).astype(F)                 # every interior edge, to fp32
        below, above = np.nextafter(edges, F(-np.inf)), np.nextafter(edges, F(np.inf))
        v = np.concatenate([[lo[l, c], hi[l, c]], edges, below, above, np.nextafter(below, F(-np.inf)), np.nextafter(above, F(np.inf)),
                            [np.nextafter(lo[l, c], F(-np.inf)), np.nextafter(hi[l, c], F(np.inf)), lo[l, c] - F(1.0), hi[l, c] + F(1.0), F(0.0), F(-3.0), F(1e30)]]).astype(F)
        got = st.bins(c, l, v)
        want = depth.sample_marginal_bin(v, lo[l, c], hi[l, c], nbins)
        assert same_bits(got, want), "depth %d: %d of %d bins differ" % (l, int((got != want).sum()), v.size)
        assert got[0] == 0 and got[1] == nbins - 1                                   # v = lo, v = hi (the last bin)
        assert (got[-7:] == [0, nbins - 1, 0, nbins - 1, 0, 0, nbins - 1]).all()      # outside the box: an end bin
        assert got.min() == 0 and got.max() == nbins - 1 and len(set(got.tolist())) == nbins
        inner = got[2 + 2 * (nbins - 1):2 + 3 * (nbins - 1)]                          # just above edge k: bin k or k - 1 (the edge is a rounded fp32)
        assert (np.abs(inner - np.arange(1, nbins)) <= 1).all()
        exact = np.floor(((v.astype(np.float64) - dlo) / w) * nbins).clip(0, nbins - 1)
        assert (got == exact).all()


def test_bin_of_a_box_without_width_and_of_chain_zero_outside(h):
    M, K = 2, 2
    start, obs, wt, pv0, A = linear_case(M, K)
    start[0, 4], start[1, 4] = F(2.5), F(3.9)                                        # depth 0: below minvel - width; depth 1: above maxvel
    a = dict(width=0.25, minvel=3.0, maxvel=3.5)
    st = marginal_stage(h, start, obs, wt, 2, nbins=7, **a)
    lo, hi = depth.sample_box(start[:M], a["width"], a["minvel"], a["maxvel"])
    assert lo[0, 4] == F(3.0) and hi[0, 4] == F(2.75) and lo[1, 4] == F(3.65) and hi[1, 4] == F(3.5)      # hi < lo: no width
    v = np.array([2.0, 2.75, 3.0, 3.2, 3.5, 3.65, 9.0], F)
    for l in (0, 1):
        assert not st.bins(4, l, v).any() and not depth.sample_marginal_bin(v, lo[l, 4], hi[l, 4], 7).any()
    start[0, 4] = F(3.25)
    st = marginal_stage(h, start, obs, wt, 2, nbins=7, width=0.0, minvel=3.0, maxvel=3.5)      # width 0: lo = hi
    assert not st.bins(4, 0, v).any() and not depth.sample_marginal_bin(v, F(3.25), F(3.25), 7).any()
    # chain 0 starts at the unclipped start: below lo at depth 0 of column 4, above hi at depth 1; the counts fall into the end bins
    start[0, 4], start[1, 4] = F(2.9), F(3.6)
    st = marginal_stage(h, start, obs, wt, 3, nbins=7, burn=0, step=1e-6, spread=0.0, width=0.2, minvel=3.0, maxvel=3.5)
    T32.begin(st, pv0, A)
    assert st.a["models"][0, 0, 4] == F(2.9) and st.a["models"][1, 0, 4] == F(3.6)
    st.linear(pv0, A, 4)
    hist = st.marginal_state()["hist"]
    assert hist[0, 0, 0, 4] == 4 and hist[6, 1, 0, 4] == 4 and hist[:, :, 0, 4].sum() == 8      # every proposal of chain 0 leaves the box
    tw = depth.sample_marginal_bin(st.a["models"][:M, :, 4], F([[3.0], [3.4]]), F([[3.1], [3.5]]), 7)
    assert tw[0, 0] == 0 and tw[1, 0] == 6


# ---- 2. the header's stage against the twin, bit for bit; the sampler's own bits ----

@pytest.mark.parametrize("every", [0, 2])
@pytest.mark.parametrize("M,K,C", [(1, 2, 2), (3, 6, 3), (7, 12, 2)])
def test_header_equals_the_twin_and_only_observes(h, M, K, C, every):
    nx, ny, sweeps, nbins = 4, 3, 25, 7
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] *= F(0.5)
    wt[1, 6] = 0.0
    a = NARROW
    assert a["burn"] == 5
    sh = T32.header_shape(h, nx, ny, obs, wt, pv0, A, a["smooth"], 0.1)
    st = marginal_stage(h, start, obs, wt, C, nx, ny, shape=sh, block_every=every, nbins=nbins, with_cov=True, **a)
    T32.begin(st, pv0, A)
    st.linear(pv0, A, sweeps)
    off = marginal_stage(h, start, obs, wt, C, nx, ny, shape=sh, block_every=every, **a)
    T32.begin(off, pv0, A)
    off.linear(pv0, A, sweeps)
    got, want = st.state(), off.state()
    for name in want:
        assert same_bits(got[name], want[name]), name                              # the marginals only observe
    for x, y in zip(st.finish(), off.finish()):
        assert same_bits(x, y)
    fw = T29.stage(R.load(), start, obs, wt, C, nx, ny, **a)

    def forward(models):
        fw.a["models"][...] = models
        fw.forward(pv0, A)
        return fw.pv.copy()

    mt = depth.SampleMarginalTwin(start, C, a["width"], a["minvel"], a["maxvel"], a["burn"], nbins, True)
    tw = depth.column_sample_twin(nx, ny, start, obs, wt, forward, C, sweeps, a["burn"], a["smooth"], a["step"], a["spread"], a["width"], a["temperature"], a["minvel"],
                                  a["maxvel"], a["seed"], after=mt.after, shape=sh, block_every=every)
    ms = st.marginal_state()
    assert same_bits(ms["hist"], mt.hist) and same_bits(ms["P"], mt.P)
    fin, tfin = st.marginal_finish(LEVELS), mt.finish(tw, LEVELS)
    for name in ("hist", "mode", "quantiles", "cov"):
        assert same_bits(np.ascontiguousarray(fin[name]), np.ascontiguousarray(tfin[name])), name
    assert ms["hist"][:, :, :, [5, 6]].sum() == 2 * M * C * (sweeps - a["burn"]) and (fin["hist"] > 0).sum() > 2 * M      # counts in several bins
    # a second finish with other levels leaves the state alone and keeps the mode
    again = st.marginal_finish((0.5,))
    assert same_bits(again["mode"], fin["mode"]) and same_bits(again["quantiles"][0], fin["quantiles"][2]) and same_bits(st.marginal_state()["hist"], ms["hist"])


# ---- 3. the laws ----

def test_laws_of_the_counts_and_the_finish(h):
    M, K, C, nx, ny, sweeps, burn, nbins = 7, 12, 5, 4, 3, 60, 20, 16
    start, obs, wt, pv0, A = linear_case(M, K, nx, ny)
    wt[:, 5] = 0.0                                                                  # interior column 5: no datum (flag 2); column 6 moves
    st = marginal_stage(h, start, obs, wt, C, nx, ny, burn=burn, nbins=nbins, with_cov=True, width=0.12, minvel=2.9, maxvel=3.6, step=0.08)
    T32.begin(st, pv0, A)
    st.linear(pv0, A, sweeps)
    s, ms, fin = st.state(), st.marginal_state(), st.marginal_finish(LEVELS)
    nodes, cols, counts = st.finish()
    idle = [c for c in range(nx * ny) if c != 6]
    assert counts[7, 6] == sweeps - burn and counts[1, 5] == 2 and not counts[7, idle].any()
    assert (ms["hist"].sum(axis=0)[:, :, 6] == sweeps - burn).all() and not ms["hist"][:, :, :, idle].any() and not ms["P"][:, :, idle].any()
    for i in range(M):
        assert same_bits(ms["P"][depth.column_tri(i, i)], s["S2"][i])              # the diagonal of P is S2
        assert same_bits(fin["cov"][depth.column_tri(i, i)], nodes[1][i])           # and the diagonal of cov the fetched variance
    lo, hi = depth.sample_box(start[:M], 0.12, 2.9, 3.6)
    q = fin["quantiles"]
    assert (np.diff(q, axis=0) >= 0).all() and (q[:, :, 6] >= lo[:, 6]).all() and (q[:, :, 6] <= hi[:, 6]).all()
    assert (fin["mode"][:, 6] > lo[:, 6]).all() and (fin["mode"][:, 6] < hi[:, 6]).all()
    assert not q[:, :, idle].any() and not fin["mode"][:, idle].any() and not fin["cov"][:, idle].any() and not fin["hist"][:, :, idle].any()
    assert all(np.isfinite(x).all() for x in (q, fin["mode"], fin["cov"]))
    full = np.zeros((M, M))
    for i in range(M):
        for j in range(i + 1):
            full[i, j] = full[j, i] = fin["cov"][depth.column_tri(i, j), 6]
    assert np.linalg.eigvalsh(full).min() > -1e-12 * np.trace(full)                 # a covariance
    corr = depth.sample_correlation(fin["cov"], M)
    assert np.abs(corr).max() <= 1.0 + 1e-12 and np.allclose(np.diagonal(corr[:, :, 6]), 1.0) and not corr[:, :, idle].any()


@pytest.mark.parametrize("nbins,b", [(2, 0), (2, 1), (7, 3), (256, 255)])
def test_all_mass_in_one_bin(h, nbins, b):
    M, K, C = 2, 2, 3
    start, obs, wt, pv0, A = linear_case(M, K)
    st = marginal_stage(h, start, obs, wt, C, nbins=nbins, width=0.25, minvel=0.0, maxvel=10.0)
    T32.begin(st, pv0, A)
    st.m["hist"][b, :, :, 4] = [[5, 0, 9], [1, 1, 1]]                                # a hand-made histogram: all counts in bin b
    fin = st.marginal_finish(LEVELS)
    lo, hi = depth.sample_box(start[:M], 0.25, 0.0, 10.0)
    for l in range(M):
        dlo, w = float(lo[l, 4]), float(hi[l, 4]) - float(lo[l, 4])
        assert fin["hist"][b, l, 4] == (14, 3)[l] and fin["hist"][:, l, 4].sum() == (14, 3)[l]
        assert fin["mode"][l, 4] == dlo + ((b + 0.5) / nbins) * w
        for k, p in enumerate(LEVELS):
            N = float((14, 3)[l])
            assert fin["quantiles"][k, l, 4] == dlo + ((b + (p * N) / N) / nbins) * w          # the rule's own operations
            assert abs(fin["quantiles"][k, l, 4] - (dlo + (b + p) * w / nbins)) <= 4e-16 * (dlo + w)      # lo + (b + p) w / nbins
            assert fin["quantiles"][k, l, 4] == depth.sample_marginal_quantile(fin["hist"][:, l, 4], lo[l, 4], hi[l, 4], p)
    # the first fullest bin wins a tie; an empty bin never holds a quantile
    st.m["hist"][...] = 0
    if nbins >= 7:
        st.m["hist"][[1, 4], 0, 0, 4] = 6
        fin = st.marginal_finish((0.5, 0.500001))
        dlo, w = float(lo[0, 4]), float(hi[0, 4]) - float(lo[0, 4])
        assert fin["mode"][0, 4] == dlo + (1.5 / nbins) * w
        assert fin["quantiles"][0, 0, 4] == dlo + (2.0 / nbins) * w and dlo + (4.0 / nbins) * w < fin["quantiles"][1, 0, 4] < dlo + (4.001 / nbins) * w


def test_burn_equal_to_the_sweeps_gives_zeros_and_one_chain_works(h):
    M, K = 3, 6
    start, obs, wt, pv0, A = linear_case(M, K)
    st = marginal_stage(h, start, obs, wt, 4, burn=12, nbins=7, with_cov=True)
    T32.begin(st, pv0, A)
    st.linear(pv0, A, 12)
    fin, ms = st.marginal_finish(LEVELS), st.marginal_state()
    assert not ms["hist"].any() and not ms["P"].any()
    for name in ("hist", "mode", "quantiles", "cov"):
        assert np.isfinite(fin[name]).all() and not fin[name].any(), name            # zeros, not NaN
    st = marginal_stage(h, start, obs, wt, 1, burn=10, nbins=64, with_cov=True)
    T32.begin(st, pv0, A)
    st.linear(pv0, A, 60)
    fin, nodes = st.marginal_finish(LEVELS), st.finish()[0]
    assert (fin["hist"].sum(axis=0)[:, 4] == 50).all() and same_bits(fin["hist"], st.marginal_state()["hist"][:, :, 0])
    assert (np.diff(fin["quantiles"][:, :, 4], axis=0) >= 0).all() and fin["quantiles"][:, :, 4].min() > 0
    for i in range(M):
        assert same_bits(fin["cov"][depth.column_tri(i, i)], nodes[1][i])
    # the median of the histogram is the posterior mean of this Gaussian problem to within a bin and a few standard errors
    w = 10.0 / 64
    assert (np.abs(fin["quantiles"][2, :, 4] - nodes[0][:, 4]) <= w).all()


# ---- 4. the stand-alone program ----

def test_standalone_program_runs(h, tmp_path):
    """the same file with its own main (every size and both bin counts: what the sanitizer build of DESIGN.md section 33 ran), here plain"""
    exe = G.build_main(str(tmp_path / "hostcheck_column_sample_marginals"))
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok") and out.stdout.count("0 laws broken") == 24, out.stdout + out.stderr
