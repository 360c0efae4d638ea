"""Device matrix-vector products against the reference's aprod (aprod.f90:7-60): bit-exact, because every
output element adds its entries in storage order in fp32."""
import ctypes as C

import numpy as np
import pytest

import _libs as L
import synth
from dsurftomo_amd import io as taipei
from dsurftomo_amd.engine import Engine, load_library

pytestmark = pytest.mark.gpu


def aprod(fn, mode, m, n, x, y, rw, row, col):
    """the reference's calling convention: iw = [nar, rows, cols]"""
    nar = rw.size
    iw = np.concatenate([[nar], row, col]).astype(np.int32)
    x = np.array(x, np.float32, copy=True)
    y = np.array(y, np.float32, copy=True)
    ib = lambda v: C.byref(C.c_int(int(v)))
    fn(ib(mode), ib(m), ib(n), L.ptr(x), L.ptr(y), ib(iw.size), ib(nar), L.ptr(iw), L.ptr(np.ascontiguousarray(rw, np.float32)))
    return y if mode == 1 else x


def check(e, m, n, rw, row, col, seed):
    r = synth.LCG(seed)
    x = (2.0 * r.uniform(n) - 1.0).astype(np.float32)
    y = (2.0 * r.uniform(m) - 1.0).astype(np.float32)
    e.spmv_load(m, n, rw, row, col)
    fns = [L.oracle().dso_aprod] + ([L.ref().aprod_] if L.ref() is not None else [])
    for mode in (1, 2):
        got = e.spmv(mode, x, y)
        for fn in fns:
            want = aprod(fn, mode, m, n, x, y, rw, row, col)
            assert (got.view(np.uint32) != want.view(np.uint32)).sum() == 0


def test_taipei_matrix_with_weights_and_appended_rows():
    """the matrix of the Taipei forward call, data weights applied and smoothing-like rows appended the way
    main.f90:361-457 does, then both products"""
    c = taipei.load()
    d = L.call_boundary(load_library().dsa_calsurfg, c)
    m0, n = c["ndata"], c["nparpi"]
    r = synth.LCG(3)
    w = (r.uniform(m0) > 0.1).astype(np.float32)
    rw = d["rw"] * w[d["iw"] - 1]
    extra_rows = np.repeat(np.arange(m0 + 1, m0 + 1 + 400, dtype=np.int32), 7)
    extra_cols = (1 + (r.uniform(extra_rows.size) * n).astype(np.int32)).clip(1, n)
    extra_val = np.tile(np.array([6, -1, -1, -1, -1, -1, -1], np.float32) * np.float32(4.0), 400)
    e = Engine(0)
    try:
        check(e, m0 + 400, n, np.concatenate([rw, extra_val]), np.concatenate([d["iw"], extra_rows]), np.concatenate([d["col"], extra_cols]), 11)
    finally:
        e.close()


def test_unsorted_storage_order_and_empty_rows():
    r = synth.LCG(8)
    m, n, nar = 300, 170, 20000
    row = (1 + (r.uniform(nar) * (m - 40)).astype(np.int32)).astype(np.int32)        # the last 40 rows stay empty
    col = (1 + (r.uniform(nar) * n).astype(np.int32)).clip(1, n).astype(np.int32)
    rw = (r.uniform(nar) - 0.5).astype(np.float32)
    e = Engine(0)
    try:
        check(e, m, n, rw, row, col, 5)
        with pytest.raises(Exception):
            e.spmv_load(m, n, rw, row + m, col)
    finally:
        e.close()


def test_dropin_aprod_caches_the_matrix():
    """dsa_aprod with the reference's argument list: same bits as aprod_, also after the matrix changes in place"""
    lib = load_library()
    r = synth.LCG(21)
    m, n, nar = 120, 90, 5000
    row = (1 + (r.uniform(nar) * m).astype(np.int32)).clip(1, m).astype(np.int32)
    col = (1 + (r.uniform(nar) * n).astype(np.int32)).clip(1, n).astype(np.int32)
    rw = (r.uniform(nar) - 0.5).astype(np.float32)
    iw = np.concatenate([[nar], row, col]).astype(np.int32)
    ib = lambda v: C.byref(C.c_int(int(v)))
    for trial in range(3):
        if trial == 2:
            rw *= np.float32(1.5)                         # modified in place: must be noticed
        for mode in (1, 2, 1):
            out = []
            for fn in (lib.dsa_aprod, L.oracle().dso_aprod):
                x = np.linspace(-1, 1, n).astype(np.float32)
                y = np.linspace(2, -2, m).astype(np.float32)
                rc = fn(ib(mode), ib(m), ib(n), L.ptr(x), L.ptr(y), ib(iw.size), ib(nar), L.ptr(iw), L.ptr(rw))
                assert fn is not lib.dsa_aprod or rc == 0, lib.dsa_dropin_error()
                out.append(np.concatenate([x, y]))
            assert (out[0].view(np.uint32) != out[1].view(np.uint32)).sum() == 0


# ---- past one block: the inputs of the products cut into several blocks of kSpmvBlock elements ---------------------------------
# (csrc/spmv.hip: build_order, run_ordering.  The tests above stay below 32 768 rows and columns: one block, index base 0.)

import synth_matrix as SM


def dispatch(S):
    """what run_ordering runs for the matrix S, per product: blocks of the input vector, the threads of k_spmv_block (1024 when
    a block has nslices = ceil(segments / 64) >= 16 * 200, else 512), blocked segments (entries in ascending input order) and
    segments of blocks[nblocks] (k_spmv_sliced), and the blocks without an entry (padded == 0: not launched)"""
    out = {}
    for mode, key, other, nkeys, ninput in ((1, S["row"], S["col"], S["m"], S["n"]), (2, S["col"], S["row"], S["n"], S["m"])):
        asc = SM.segment_ascending(key, other, nkeys)
        used = np.bincount(key, minlength=nkeys + 1)[1:] > 0
        seg_ok = asc[key - 1]
        nblocks = (ninput + SM.BLOCK - 1) // SM.BLOCK
        per_block = np.bincount((other[seg_ok] - 1) // SM.BLOCK, minlength=nblocks)
        out[mode] = dict(nblocks=nblocks, threads=1024 if (nkeys + 63) // 64 >= 16 * 200 else 512, blocked=int((asc & used).sum()),
                         unblocked=int((~asc & used).sum()), empty_blocks=[b for b in range(nblocks) if per_block[b] == 0],
                         tail=ninput - (nblocks - 1) * SM.BLOCK)
    return out


def check_big(S, seed):
    """both products through Engine.spmv and through the drop-in dsa_aprod, each against dso_aprod, bit for bit"""
    m, n, rw, row, col = S["m"], S["n"], S["rw"], S["row"], S["col"]
    x = (2.0 * SM.mix(np.arange(n), seed) - 1.0).astype(np.float32)
    y = (2.0 * SM.mix(np.arange(m), seed + 1) - 1.0).astype(np.float32)
    lib = load_library()
    lib.dsa_aprod_invalidate()
    e = Engine(0)
    try:
        e.spmv_load(m, n, rw, row, col)
        for mode in (1, 2):
            want = aprod(L.oracle().dso_aprod, mode, m, n, x, y, rw, row, col)
            got = e.spmv(mode, x, y)
            assert (got.view(np.uint32) != want.view(np.uint32)).sum() == 0, "Engine.spmv mode %d" % mode
            got = aprod(lib.dsa_aprod, mode, m, n, x, y, rw, row, col)
            assert (got.view(np.uint32) != want.view(np.uint32)).sum() == 0, "dsa_aprod mode %d" % mode
            assert np.abs(want - (x if mode == 2 else y)).max() > 0       # (the product did something)
    finally:
        e.close()


def test_several_blocks_with_regularisation_rows_512_threads():
    """(a) 100 001 x 68 479, data rows then regularisation rows: y += A x over 3 blocks of x (the last 2 943 long: LDS tail copy)
    and x += A^T y over 4 blocks of y (the last 1 697 long), both with k_spmv_block<512>; the regularisation rows are the unblocked
    part of y += A x (k_spmv_sliced), A^T y is all blocked"""
    S = SM.system(31522, 47, 47, 31, seed=1)
    d = dispatch(S)
    assert (S["m"], S["n"]) == (100001, 68479)
    assert d[1]["nblocks"] == 3 and d[1]["threads"] == 512 and d[1]["unblocked"] > 50000 and d[1]["blocked"] > 40000 and d[1]["tail"] % 4 == 3
    assert d[2]["nblocks"] == 4 and d[2]["threads"] == 512 and d[2]["unblocked"] == 0 and d[2]["tail"] % 4 == 1
    assert not d[1]["empty_blocks"] and not d[2]["empty_blocks"]
    check_big(S, 3)


def test_several_blocks_1024_threads_and_an_empty_block():
    """(b) 238 479 rows (>= 204 737: nslices >= 3 200): y += A x runs k_spmv_block<1024> on each of the 3 blocks of x, plus the
    unblocked regularisation rows; rows 131 072 .. 163 839 hold no entry, so x += A^T y skips block 4 of its 8 blocks of y (padded 0)
    and runs <512> on the others, the last one 9 103 long"""
    S = SM.system(170000, 47, 47, 31, seed=2, skip=(4 * SM.BLOCK, 5 * SM.BLOCK), mean_len=25)
    d = dispatch(S)
    assert S["m"] >= 204801 and d[1]["threads"] == 1024 and d[1]["nblocks"] == 3 and d[1]["unblocked"] > 50000
    assert d[2]["threads"] == 512 and d[2]["nblocks"] == 8 and d[2]["empty_blocks"] == [4] and d[2]["tail"] % 4 == 3
    assert S["rw"].size < 6_000_000
    check_big(S, 4)


def test_several_blocks_all_unblocked_and_all_blocked():
    """(c) regularisation rows only, the interior ones (7 entries, `here` first: none ascending), stored last row first so that
    the columns run downwards too: y += A x has nothing blocked (every segment in k_spmv_sliced, blocks 0..2 of x skipped), and
    A^T y keeps only the single-entry columns blocked.  Then data rows only: blocks[nblocks] empty in both products."""
    nvx, nvy, nl = 47, 47, 31
    r, c, v = SM.regularisation_rows(nvx, nvy, nl, 2.0, 0, descending=True)
    keep = np.repeat(np.bincount(r) == 7, np.bincount(r))
    r, c, v = r[keep], c[keep], v[keep]
    rows = np.unique(r)
    r = np.searchsorted(rows, r)                              # interior rows numbered 0 .. 58 724, storage still last-row first
    S = dict(m=int(rows.size), n=nvx * nvy * nl, rw=v, row=(r + 1).astype(np.int32), col=(c + 1).astype(np.int32))
    d = dispatch(S)
    assert d[1]["nblocks"] == 3 and d[1]["blocked"] == 0 and d[1]["empty_blocks"] == [0, 1, 2]
    assert d[2]["nblocks"] == 2 and d[2]["unblocked"] > 50000
    check_big(S, 5)
    S = SM.system(120001, 47, 47, 31, seed=6, regularise=False, mean_len=25)
    d = dispatch(S)
    assert d[1]["unblocked"] == 0 and d[2]["unblocked"] == 0 and d[1]["nblocks"] == 3 and d[2]["nblocks"] == 4
    check_big(S, 7)
