// rm_itemweights_csr.hpp -- the scores of an item-item model whose weight matrix is SPARSE (SLIM, item-kNN; rm_*_item_weights_csr_*):
// S = X_hist * W with W a CSR of n_in rows over n columns, formed from the stored entries only.  k_scores_item_weights_csr writes the
// chunk S[users of a batch][lds] that k_scores_item_weights (rm_itemweights.hpp) writes from a dense W; everything behind the chunk is
// the from-scores stages, unchanged.
//
// Contract.  W_p[n_in + 1], column ids W_i in [0, n), values W_v in T; every row strictly ascending (validated in front of the kernel:
// rm_lib.hip check_csr_rows -- the k_check_csr_* kernels of rm_prep.hpp and k_check_csr_repeats below; unsorted rows never get here, they
// are sorted in a copy first).  For user u with stored history entries (j_1, v_1) .. (j_h, v_h) in ascending j
//     s_i = fma_chain_step(v, W[j][i], acc)   over the j whose row STORES column i, in ascending j, from acc = +0.
// A stored zero is a step; an entry that W does not store is skipped, never multiplied; an item no row of the history stores is +0.
//   * Finite W, finite history values: every output equals, bit for bit, what the dense entries return for W densified -- as long as no
//     partial sum is a negative zero (a skipped fma(v, +0, acc) leaves every other acc as it is, and the ranking reads -0 as +0 anyway).
//   * A non-finite stored W[j][i] reaches exactly the users who have j, and only item i -- sharper than the dense route, which reads the
//     whole row j.
//
// The kernel is a SCATTER WITH AN ORDER: the contributions to one column must be applied in ascending j.  LDS atomics cannot carry that
// order, so the design keeps one writer stream per accumulator tile:
//
// Work split.  A WAVEFRONT owns one user times one column tile; the tile's accumulators live in LDS (zero-filled with 16-byte writes).
// A block is four wavefronts (four users, one tile) that share nothing: no block barrier.  The column tile is the slow grid index, users
// the fast one, as in the dense kernel: the blocks resident at one time touch the same slice of W's rows.
//
// Tile width.  16 KiB of LDS per wavefront: 4,096 columns in fp32, 2,048 in fp64 -- 64 KiB per block, two blocks per compute unit of
// 160 KiB.  (8 KiB tiles double the searches and the passes over the history per user, 32 KiB tiles leave one block per compute unit;
// no A/B of the three has been run on the device yet: DESIGN.md section 8.)
//
// History through registers.  64 (id, value) pairs per load, one per lane, as in the dense kernel.  With more than one tile every lane
// finds the sub-range of ITS row W_i[W_p[j] .. W_p[j + 1]) that falls into the tile with two lower-bound searches -- 64 rows searched at
// once; with one tile the sub-range is the whole row.
//
// Walk.  The entries are taken in order: v_readlane gives a row's sub-range and the history value; the lanes stride over the piece's
// (column, weight) pairs and do acc[col - c0] = fma_chain_step(v, w, acc[col - c0]) in LDS.  The columns inside one row are distinct
// (validated), so a step has no conflict; the LDS instructions of ONE wavefront are executed in program order, so a later row's step
// sees the earlier row's -- the chain order holds without a barrier.  (The accumulators are accessed through a volatile LDS pointer and the
// steps are separated by a wavefront-scope fence: the compiler must not reorder what the hardware keeps in order.)
// Unrolled by IW_UNROLL rows: the global loads of the next rows' first pieces are issued first, then the LDS read-modify-writes in row
// order.  Pieces longer than 64 entries loop; the tail is predicated, never padded.
//
// Write-out.  The tile is copied to the chunk with whole 16-byte stores (the chunk's stride is a multiple of the vector); a partial last
// vector is stored by element, columns at or beyond n are not stored.  A user without history stores a tile of +0.
//
// No matrix instruction, for the reason rm_itemweights.hpp gives.  No faster variant whose order is not proven is kept: several short
// pieces packed into one 64-lane step (ordered conflict resolution) and accumulators in global memory are follow-ups, DESIGN.md section 8.
#pragma once
#include "rm_itemweights.hpp"

namespace rm {

constexpr int CSR_BAD_REPEAT = 16;                                   // (beside rm_device.hpp's CSR_BAD_*: a column id twice in one row)
constexpr int IW_CSR_TILE_BYTES = 16384;
template <class T> struct ItemWeightCsrTile {
    static constexpr int VE = 16 / (int)sizeof(T), COLS = IW_CSR_TILE_BYTES / (int)sizeof(T);
};

template <class T> struct ItemWeightCsrArgs {
    const int *W_p, *W_i; const T *W_v; int n, m;                    // m: the users of the batch
    const int *hist_p, *hist_i; const T *hist_v;                     // hist_p: at the batch's first user (its entries index the whole arrays)
    const Plan *plan;                                                // the verdict of the validation (rm_lib.hip check_csr_rows)
    T *S; size_t lds;                                                // the chunk [m][lds], lds a multiple of VE
    unsigned ublocks, tiles;                                         // blocks of four users per column tile; column tiles
};

// Equal neighbours inside a row: k_check_csr_flat counts descents and allows idx[e] == idx[e + 1] (SciPy's has_sorted_indices), which a
// scatter cannot take.  Flat, one thread per entry; the rare hit names its row.  Meaningful once the rows are known to ascend.
__global__ __launch_bounds__(CHECK_FLAT_THREADS) void k_check_csr_repeats(int rows, const int *indptr, const int *idx, Plan *plan)
#ifdef RM_ITEMWEIGHTS_CSR_PLAIN_KERNELS
{
    if (plan->csr_bad & (CSR_BAD_INDPTR | CSR_BAD_INDEX)) return;
    const long long e0 = indptr[0], e1 = indptr[rows];
    for (long long e = e0 + (long long)blockIdx.x * blockDim.x + threadIdx.x; e + 1 < e1; e += (long long)gridDim.x * blockDim.x) {
        if (idx[e] != idx[e + 1]) continue;
        int lo = 0, hi = rows;                                       // the last row that starts at or before e + 1
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((long long)indptr[mid] <= e + 1) lo = mid; else hi = mid - 1; }
        if ((long long)indptr[lo] <= e) { atomicOr(&plan->csr_bad, CSR_BAD_REPEAT); plan->csr_where = lo; }      // (e in the same row)
    }
}
#else
;
#endif

template <class T>
__global__ __launch_bounds__(IW_THREADS) void k_scores_item_weights_csr(ItemWeightCsrArgs<T> a)
{
    typedef ItemWeightCsrTile<T> G;
    typedef T VT __attribute__((ext_vector_type(G::VE)));
    constexpr int VE = G::VE, U = IW_UNROLL, COLS = G::COLS;
    __shared__ __attribute__((aligned(16))) T tiles[IW_THREADS / WAVE][COLS];
    if (a.plan->csr_bad) return;                                     // (the history indexes the rows of W, W_i the accumulators)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned tile = blockIdx.x / a.ublocks, ub = blockIdx.x % a.ublocks;
    const int u = (int)ub * (IW_THREADS / WAVE) + wv;
    if (u >= a.m) return;
    const int n = a.n, c0 = (int)tile * COLS, c1 = min(c0 + COLS, n);
    const bool one_tile = a.tiles == 1;
    // (an LDS pointer by its address space: through a generic volatile pointer every step would be a flat access that waits for the
    // global loads in flight)
    typedef __attribute__((address_space(3))) volatile T LdsT;
    LdsT *acc = (LdsT *)&tiles[wv][0];
    #pragma unroll
    for (int i = 0; i < COLS / VE / WAVE; i++) *(VT *)&tiles[wv][(i * WAVE + lane) * VE] = VT{};
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const int h0 = __builtin_amdgcn_readfirstlane(a.hist_p[u]), h1 = __builtin_amdgcn_readfirstlane(a.hist_p[u + 1]);
    // one (column, weight) pair of a piece, by this lane: the chain step on the column's accumulator
    const auto step = [&](T vj, int col, T w) { const int c = col - c0; acc[c] = fma_chain_step(vj, w, acc[c]); };
    for (int base = h0; base < h1; base += WAVE) {
        const int e = base + lane;
        int s0 = 0, s1 = 0; T v = (T)0;                              // the lane's row piece W_i[s0 .. s1) inside the tile
        if (e < h1) {
            const int j = a.hist_i[e];
            v = a.hist_v ? a.hist_v[e] : (T)1;
            s0 = a.W_p[j]; s1 = a.W_p[j + 1];
            if (!one_tile) {
                int lo = s0, hi = s1;                                // first entry with column >= c0
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.W_i[mid] < c0) lo = mid + 1; else hi = mid; }
                s0 = lo; hi = s1;                                    // ... with column >= c1
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (a.W_i[mid] < c1) lo = mid + 1; else hi = mid; }
                s1 = lo;
            }
        }
        const int cnt = min(WAVE, h1 - base);
        for (int j0 = 0; j0 < cnt; j0 += U) {
            int lo[U], hi[U], col[U]; T w[U];
            #pragma unroll
            for (int j = 0; j < U; j++) {                            // the loads of the rows' first pieces (rows beyond cnt: empty)
                lo[j] = hi[j] = 0;
                if (j0 + j < cnt) { lo[j] = lane_bcast<int>(s0, j0 + j); hi[j] = lane_bcast<int>(s1, j0 + j); }
                col[j] = c0; w[j] = (T)0;
                if (lo[j] + lane < hi[j]) { col[j] = a.W_i[lo[j] + lane]; w[j] = a.W_v[lo[j] + lane]; }
            }
            #pragma unroll
            for (int j = 0; j < U; j++) {                            // the chain steps, in row order
                if (j0 + j < cnt) {
                    const T vj = lane_bcast<T>(v, j0 + j);
                    if (lo[j] + lane < hi[j]) step(vj, col[j], w[j]);
                    for (int p = lo[j] + WAVE; p < hi[j]; p += WAVE)                 // a piece of more than 64 entries
                        if (p + lane < hi[j]) step(vj, a.W_i[p + lane], a.W_v[p + lane]);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
            }
        }
    }
    T *out = a.S + (size_t)u * a.lds + c0;
    #pragma unroll 4
    for (int i = 0; i < COLS / VE / WAVE; i++) {
        const int c = (i * WAVE + lane) * VE;
        if (c0 + c + VE <= n) *(VT *)(out + c) = *(const VT *)&tiles[wv][c];
        else {
            #pragma unroll
            for (int k = 0; k < VE; k++) if (c0 + c + k < n) out[c + k] = tiles[wv][c + k];
        }
    }
}

// ---- every instantiation of this header's kernel template (rm_kernel_units.hpp) -----------------------------------------
#define RM_ITEMWEIGHTS_CSR_KERNELS_F32(X) X(k_scores_item_weights_csr<float>)
#define RM_ITEMWEIGHTS_CSR_KERNELS_F64(X) X(k_scores_item_weights_csr<double>)
RM_ITEMWEIGHTS_CSR_KERNELS_F32(RM_EXTERN_KERNEL)
RM_ITEMWEIGHTS_CSR_KERNELS_F64(RM_EXTERN_KERNEL)

} // namespace rm
