// Device copy of a COO matrix in row order and in column order (spmv.hip builds it, lsmr.hip uses it).
#pragma once

#include <vector>

#include "engine.h"

namespace dsa {

struct SpmvState {
    int m = 0, n = 0;
    long long nar = 0;
    // One ordering of the matrix (by row for A x, by column for A^T y) in slices of 64 segments, longest segments first:
    // entry k of the segment held by lane l of slice j sits at off[j] + 64 k + l, so the 64 lanes of a wavefront read 64
    // consecutive values / indices per step (coalesced) while every lane adds the entries of ITS segment in storage order.
    struct Sliced {
        DevBuf<long long> off;       // nslices + 1 slice offsets (entries)
        DevBuf<int> seg, len;        // per (slice, lane): segment (row / column) and its entry count; nslices * 64
        DevBuf<float> val;
        DevBuf<int> idx;             // 0-based index into the input vector (the unblocked part), or
        DevBuf<unsigned short> idx16; // block-local index (blocks of 32768 input elements)
        int nslices = 0;
        long long padded = 0;        // entries of storage (>= nar)
    };
    // One orientation of the matrix: the input vector is cut into blocks of `block` elements that fit the LDS; block b holds,
    // slice-transposed, the entries whose input index falls into it, for the segments whose entries are stored in ascending
    // input order (every data row and every column are; the reference's regularisation rows are not), and a product runs the
    // blocks one after the other -- so every output element still adds its entries in storage order, but the gathers of the
    // input vector are LDS reads instead of one 128-B L2 line per 4-byte operand.  blocks[nblocks] holds the other segments with
    // global indices (gathers from L2).  data_len: per block, how many entries of each (slice, lane) are data entries (DWS).
    struct Ordering {
        int block = 0, nblocks = 0, ninput = 0;
        std::vector<Sliced> blocks;
        std::vector<DevBuf<int>> data_len;
    };
    Ordering by_row, by_col;
    // the matrix is dsa_iteration_system_radial_device's: below the data rows it holds tie rows as well as Laplacian rows, which the entry
    // points that rebuild every row below the data with another weight refuse (dsa_lsmr_tradeoff, dsa_lsmr_crossval); cleared by every load
    bool radial = false;
    DevBuf<float> x, y;
    // LSMR work vectors (lsmr.hip)
    DevBuf<float> u, v, h, hbar, xs, localV, scal;
    // pinned host copies of u and v for the host-vector placement (they cross PCIe twice per LSMR iteration)
    float* hu = nullptr; float* hv = nullptr;
    size_t hu_cap = 0, hv_cap = 0;
    // dsa_lsmr_batch (lsmr_batch.hip): each ordering once more as plain CSR / CSC -- a segment's entries contiguous, in storage
    // order, global input indices -- built from the orderings above on the first batch after a load (valid = false: rebuild)
    struct Contiguous {
        DevBuf<long long> ptr;       // nseg + 1
        DevBuf<float> val;
        DevBuf<int> idx;
    };
    Contiguous row_csr, col_csr;
    bool contiguous_valid = false;
    // dsa_lsmr_tradeoff: copies of row_csr.val / col_csr.val whose entries of the rows from coef_ndata up hold their integer
    // coefficient c (the resident entry is fl(c * coef_weight0)); built on the first trade-off call after a load, or when the key changes
    DevBuf<float> row_coef, col_coef;
    bool coef_valid = false;
    int coef_ndata = 0;
    float coef_weight0 = 0.0f;
    DevBuf<int> bflag;               // ... the flag its validation reports
    // batch vectors, realisations in groups of 64, one per lane: element i of realisation 64 g + l at (g * len + i) * 64 + l.  btmp is not
    // one of them: every entry point of lsmr_batch.hip carves it into its own pieces (the solutions on their way out, b, weights, folds,
    // row scales or host models, realisation-major), which live for that call alone
    DevBuf<float> bu, bv, bh, bhbar, bx, blocalV, bscale, bparam, bred, btmp, bterm, bpmax;
    // the solutions a batch solve left in bx, for dsa_forward_steps / dsa_step_models with steps == NULL: set by a successful batch solve in the
    // space of the unknowns (bx_n = the matrix's columns then), cleared when a batch begins, when the resident matrix is loaded or edited, and
    // by dsa_lsmr_voronoi, whose bx is in cell space
    bool bx_valid = false;
    int bx_nreal = 0, bx_n = 0;
    // bcoord: dsa_lsmr_resolution's coordinates of the unknowns and their cosines.  bpsf: the fp64 measures of a call, carved per call into
    // block partials, results and (dsa_lsmr_crossval) residuals -- dsa_lsmr_resolution's PSFs, dsa_lsmr_tradeoff's and dsa_lsmr_crossval's measures
    DevBuf<double> bcoord, bpsf;
    // dsa_lsmr_voronoi: per call, the tessellations (vxyz: points of the unknowns; vseeds: seed unknowns, member-major; vcell_mm: cell of every
    // unknown, member-major; vcell: the same as [group][unknown][64]), the data rows' CSR positions sorted by cell per member (vlist, with
    // vcptr: ncells + 1 pointers per member; vrowof: row of every position), the operands of the projected products (vfull: v expanded to the
    // unknowns, [group][unknown][64]; vut: u member-major), the sort's buffers and the ensemble statistics
    DevBuf<double> vxyz, vstats;
    DevBuf<int> vseeds, vcell_mm, vcell, vlist, vcptr, vrowof, vkeys, vkeys_out, vpos;
    DevBuf<float> vfull, vut;
    DevBuf<unsigned char> vsort;
    float* hbatch = nullptr;         // pinned: per-realisation coefficients and flags (bparam) on their way to the device, norms on their way back
    size_t hbatch_cap = 0;
};

// y += A x (mode 1; x: n, y: m) or x += A^T y (mode 2) on device vectors, on the engine's stream; every output
// element adds its entries in storage order (reference aprod.f90:7-60)
void spmv_device(Engine* e, int mode, float* d_x, float* d_y);
// row_csr / col_csr of the resident matrix (e->spmv is not null), built on the first call after a load (lsmr_batch.hip); the engine's device is current
int spmv_ensure_contiguous(Engine* e);
// the resident matrix was replaced or edited: the contiguous copies of dsa_lsmr_batch (and dsa_lsmr_tradeoff's coefficient copy of them) are stale,
// and the batch solutions in bx no longer belong to it
inline void spmv_invalidate_contiguous(SpmvState* s) { if (s) s->contiguous_valid = s->coef_valid = s->bx_valid = false; }

}  // namespace dsa
