"""Deterministic COO matrices shaped like the inversion system of main.f90:361-466, at sizes that cut the input vector of
both products into several blocks of csrc/spmv.hip (kSpmvBlock = 32768 elements).

Everything is index arithmetic on numpy arrays: `mix` hashes an index array into uniform draws, so a matrix of a few
million entries costs milliseconds (synth.LCG is a Python loop and only draws the few seeds here).

What a matrix holds (`system`):
  - data rows: ray-like runs of ascending columns (steps 0, 1, 1, 1, nvx: a run along x with jumps to the next row of
    the model, and repeated columns, which are non-decreasing and so stay in the blocked part), lengths 1 .. ~300, plus
    a few very long rows that run the two-batch UNROLL = 16 pipeline of k_spmv_block; many short ones run its tail loop;
  - regularisation rows appended behind them like main.f90:420-457: `here, here-1, here+1, here-nvx, here+nvx,
    here-plane, here+plane` (not ascending: these segments go to blocks[nblocks]) inside the model, one entry `here` on
    its faces;
  - entries at the block edges 0, 32767, 32768, 65535, 65536 and n-1 of the columns, and of the rows;
  - optionally an index range that no entry touches (a block of the input vector with no entries: padded == 0).
The data entries come first in storage, so the split of the DWS column sums at nar_data matters.
"""
import numpy as np

import synth

BLOCK = 32768                                   # csrc/spmv.hip kSpmvBlock
EDGES = (0, BLOCK - 1, BLOCK, 2 * BLOCK - 1, 2 * BLOCK)


def mix(i, seed):
    """uniform [0, 1) draws from an index array (splitmix64 finaliser of i + seed)"""
    with np.errstate(over="ignore"):
        z = np.asarray(i, np.uint64) + np.uint64((int(seed) * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def edges(n):
    return sorted({e for e in EDGES if e < n} | {n - 1})


def segment_ascending(key, other, nkeys):
    """per segment (1-based keys), whether its entries are stored in non-decreasing `other` order -- the rule of
    k_not_monotone that sends a segment to the blocked part (True) or to blocks[nblocks] (False)"""
    order = np.argsort(key, kind="stable")
    k, o = key[order], other[order]
    bad = (k[1:] == k[:-1]) & (o[1:] < o[:-1])
    flag = np.zeros(nkeys + 1, bool)
    flag[k[1:][bad]] = True
    return ~flag[1:]


def data_rows(m, n, nvx, seed, skip=None, long_rows=4, long_len=2500, mean_len=40):
    """m ray-like rows over n columns (0-based row, col; row-major storage order).  skip = (lo, hi): no column in
    [lo, hi) and no row in [lo, hi) gets an entry (an empty input block for one of the two products)."""
    r = np.arange(m, dtype=np.int64)
    u = mix(r, seed)
    # mostly short rows (many of length 1 .. 8), a tail to ~300, and `long_rows` rows of `long_len` entries
    ln = np.where(u < 0.3, 1 + (u * 26.0).astype(np.int64), 1 + (mean_len * -np.log1p(-u)).astype(np.int64).clip(0, 300))
    ln[(np.arange(long_rows) * 7919 + 11) % m] = long_len
    if skip is not None:
        ln[skip[0]:min(skip[1], m)] = 0
    ln[edges(m)] = np.maximum(ln[edges(m)], 3)           # the edge rows hold entries
    ptr = np.concatenate([[0], np.cumsum(ln)])
    nar = int(ptr[-1])
    row = np.repeat(r, ln)
    pos = np.arange(nar, dtype=np.int64) - ptr[:-1][row]
    # steps: 0 (the same column again), 1, 1, 1, nvx
    w = (mix(np.arange(nar), seed + 1) * 5).astype(np.int64)
    step = np.where(w == 0, 0, np.where(w == 4, nvx, 1))
    step[pos == 0] = 0
    cs = np.cumsum(step)
    start = (mix(r, seed + 2) * n).astype(np.int64)
    col = start[row] + cs - cs[ptr[:-1]][row]
    col = np.minimum(col, n - 1)                          # (clipping keeps a row non-decreasing)
    if skip is not None:
        inside = (col >= skip[0]) & (col < skip[1])
        col[inside] = skip[0] - 1                         # ... and so does moving into the gap's lower edge
    # every edge column is the first entry of some row (its column order stays ascending: the entry is first)
    e = edges(n)
    if skip is not None:
        e = [c for c in e if not skip[0] <= c < skip[1]]
    firsts = ptr[:-1][ln >= 2][(np.arange(len(e)) * 13 + 5)]
    for f, c in zip(firsts, e):
        row_end = ptr[row[f] + 1]
        col[f] = c
        col[f + 1:row_end] = np.maximum(col[f + 1:row_end], c)
    val = (mix(np.arange(nar), seed + 3) - 0.5).astype(np.float32) * np.float32(0.2)
    return row.astype(np.int64), col.astype(np.int64), val


def regularisation_rows(nvx, nvy, nl, weight, first_row, descending=False):
    """main.f90:420-457 (0-based rows from first_row, 0-based columns): one row per model parameter in (k, j, i) order;
    descending: the rows stored last to first (every column's entries then run downwards: nothing is ascending)"""
    i = np.arange(nvx)[None, None, :]; j = np.arange(nvy)[None, :, None]; k = np.arange(nl)[:, None, None]
    here = (k * nvy * nvx + j * nvx + i).reshape(-1)
    face = ((i == 0) | (i == nvx - 1) | (j == 0) | (j == nvy - 1) | (k == 0) | (k == nl - 1)).reshape(-1)
    plane = nvx * nvy
    offs = np.array([0, -1, 1, -nvx, nvx, -plane, plane])
    cnt = np.where(face, 1, 7)
    idx = np.arange(here.size)
    if descending:
        idx = idx[::-1]
    rowp = np.repeat(idx, cnt[idx])
    ptr = np.concatenate([[0], np.cumsum(cnt[idx])])
    pos = np.arange(rowp.size) - np.repeat(ptr[:-1], cnt[idx])
    col = here[rowp] + offs[pos]
    w = np.float32(weight)
    val = np.where(pos == 0, np.where(face[rowp], np.float32(2.0) * w, np.float32(6.0) * w), np.float32(-1.0) * w).astype(np.float32)
    return (first_row + rowp).astype(np.int64), col.astype(np.int64), val


def system(m_data, nvx, nvy, nl, seed=1, skip=None, regularise=True, long_rows=4, mean_len=40):
    """m_data data rows over n = nvx nvy nl columns, then (regularise) the n regularisation rows.
    Returns dict(m, n, rw, row, col (1-based int32), nar_data)."""
    n = nvx * nvy * nl
    s = int(synth.LCG(seed).uniform(1)[0] * (1 << 40))
    row, col, val = data_rows(m_data, n, nvx, s, skip=skip, long_rows=long_rows, mean_len=mean_len)
    m = m_data
    if regularise:
        rr, rc, rv = regularisation_rows(nvx, nvy, nl, 2.0, m_data)
        row, col, val = np.concatenate([row, rr]), np.concatenate([col, rc]), np.concatenate([val, rv])
        m += n
    return dict(m=m, n=n, rw=np.ascontiguousarray(val, np.float32), row=(row + 1).astype(np.int32), col=(col + 1).astype(np.int32),
                nar_data=m_data and int((row < m_data).sum()))
