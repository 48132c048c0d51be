// rm_itemweights.hpp -- the scores of an ITEM-ITEM model (EASE, SLIM, item-kNN; rm_*_item_weights_*): S = X_hist * W, formed from the
// rows of W that a user's history names -- a gather-accumulate, never a dense product.  k_scores_item_weights writes a chunk
// S[users of a batch][n] into the workspace; the from-scores stages (k_score_rows / k_topk_rows and everything behind them) run on
// that chunk unchanged.
//
// Contract.  W is row-major [n_in][n] with row stride ldw (elements).  For user u with stored history entries (j_1, v_1) .. (j_h, v_h)
// in ascending j (validated and sorted in front of the kernel: an id outside [0, n_in) never gets here, and the kernel returns when
// the plan says so)
//     s_i = fma(v_h, W[j_h][i], .. fma(v_2, W[j_2][i], fma(v_1, W[j_1][i], +0)) ..)
// in T: the library's k-ordered fma chain (fma_chain_step) for A = dense(X_hist), B = W^T with its zero terms left out.  Every STORED
// entry is a step, an explicit zero and a repeated id included; an entry that is not stored is never multiplied by zero (a non-finite
// W[j][i] must not reach a user who does not have j), so the tail of a row is predicated, not padded.  No history: +0 everywhere.
// hist_v == NULL: every value is 1.
//
// Work split.  A WAVEFRONT owns one user times one column tile of 2 x 64 x VE columns (VE = 16 / sizeof(T): 512 columns in fp32, 256
// in fp64).  Each lane holds two 16-byte accumulators a tile-half apart, so each of the two loads of a row piece by the wavefront is
// 1 KiB contiguous.  A block is four wavefronts (four users, one tile), with no LDS and no barrier.
//
// Grid order.  The column tile is the slow index, users the fast one: the blocks resident at one time read one slab W[:, tile]
// (n_in x 2 KiB), and the popular items' pieces are asked for again and again while they are still cached.  The other order -- a
// user's tiles next to each other, all of W in flight at once -- was measured 13 % slower and is gone.
//
// History through registers.  The wavefront loads 64 (id, value) pairs at a time, one per lane, and walks them with v_readlane: a
// row's base address is wavefront-uniform (a scalar base plus the lane's column offset), the value a scalar operand of the fma.  The
// walk is unrolled by IW_UNROLL = 8: the 16 loads are issued first, then the 16 fma in chain order -- the columns are independent, so
// the ordered chain stalls on nothing but the loads.
//
// Alignment.  VEC: W and ldw * sizeof(T) are multiples of 16 bytes -- 16-byte loads.  Otherwise the same kernel loads by element.  A
// partial last vector of a row (n % VE) takes guarded element loads in both; columns beyond n are neither loaded nor stored.  The
// chunk's row stride is a multiple of VE, so whole vectors are stored whole.
//
// No matrix instruction: the operand X_hist is 0.5 % dense.  An MFMA formulation multiplies the dense [users][n_in] matrix -- 2 m n_in n
// flop for 2 nnz n useful ones, the route this kernel replaces; the gather is bound by the bytes of W it moves, not by its fma.
#pragma once
#include "rm_prep.hpp"
#include "rm_kernel_units.hpp"

namespace rm {

constexpr int IW_THREADS = 256, IW_UNROLL = 8;
template <class T> struct ItemWeightTile {
    static constexpr int VE = 16 / (int)sizeof(T), HALF = WAVE * VE, COLS = 2 * HALF;
};

template <class T> struct ItemWeightArgs {
    const T *W; size_t ldw; int n, m;                                // m: the users of the batch
    const int *hist_p, *hist_i; const T *hist_v;                     // hist_p: at the batch's first user (its entries index the whole arrays)
    const Plan *plan;                                                // the history's validation (rm_lib.hip check_history)
    T *S; size_t lds;                                                // the chunk [m][lds], lds a multiple of VE
    unsigned ublocks;                                                // blocks of four users per column tile
};

template <class T, bool VEC>
__global__ __launch_bounds__(IW_THREADS) void k_scores_item_weights(ItemWeightArgs<T> a)
{
    typedef ItemWeightTile<T> G;
    typedef T VT __attribute__((ext_vector_type(G::VE)));
    constexpr int VE = G::VE, U = IW_UNROLL;
    if (a.plan->csr_bad & (CSR_BAD_INDPTR | CSR_BAD_INDEX)) return;   // (the history indexes the rows of W)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const unsigned tile = blockIdx.x / a.ublocks, ub = blockIdx.x % a.ublocks;
    const int u = (int)ub * (IW_THREADS / WAVE) + wv;
    if (u >= a.m) return;
    const int n = a.n;
    const int c0 = (int)tile * G::COLS + lane * VE, c1 = c0 + G::HALF;
    const bool whole0 = c0 + VE <= n, whole1 = c1 + VE <= n;
    const auto piece = [&](const T *row, int c, bool whole) {
        VT x = {};
        if (VEC && whole) x = *(const VT *)(row + c);
        else {
            #pragma unroll
            for (int i = 0; i < VE; i++) if (c + i < n) x[i] = row[c + i];
        }
        return x;
    };
    const int h0 = __builtin_amdgcn_readfirstlane(a.hist_p[u]), h1 = __builtin_amdgcn_readfirstlane(a.hist_p[u + 1]);
    VT acc0 = {}, acc1 = {};
    for (int base = h0; base < h1; base += WAVE) {
        const int e = base + lane;
        int id = 0; T v = (T)0;
        if (e < h1) { id = a.hist_i[e]; v = a.hist_v ? a.hist_v[e] : (T)1; }
        const int cnt = min(WAVE, h1 - base);
        int j0 = 0;
        for (; j0 + U <= cnt; j0 += U) {                             // eight whole steps: the loads, then the chain
            VT w0[U], w1[U];
            #pragma unroll
            for (int j = 0; j < U; j++) {
                const T *row = a.W + (size_t)lane_bcast<int>(id, j0 + j) * a.ldw;
                w0[j] = piece(row, c0, whole0); w1[j] = piece(row, c1, whole1);
            }
            #pragma unroll
            for (int j = 0; j < U; j++) {
                const T vj = lane_bcast<T>(v, j0 + j);
                #pragma unroll
                for (int i = 0; i < VE; i++) { acc0[i] = fma_chain_step(vj, w0[j][i], acc0[i]); acc1[i] = fma_chain_step(vj, w1[j][i], acc1[i]); }
            }
        }
        if (j0 < cnt) {                                              // the row's tail: predicated, never padded with zero values
            VT w0[U], w1[U];
            #pragma unroll
            for (int j = 0; j < U; j++) {
                if (j0 + j < cnt) {
                    const T *row = a.W + (size_t)lane_bcast<int>(id, j0 + j) * a.ldw;
                    w0[j] = piece(row, c0, whole0); w1[j] = piece(row, c1, whole1);
                }
            }
            #pragma unroll
            for (int j = 0; j < U; j++) {
                if (j0 + j < cnt) {
                    const T vj = lane_bcast<T>(v, j0 + j);
                    #pragma unroll
                    for (int i = 0; i < VE; i++) { acc0[i] = fma_chain_step(vj, w0[j][i], acc0[i]); acc1[i] = fma_chain_step(vj, w1[j][i], acc1[i]); }
                }
            }
        }
    }
    T *out = a.S + (size_t)u * a.lds;
    const auto store = [&](int c, bool whole, VT x) {
        if (whole) *(VT *)(out + c) = x;
        else {
            #pragma unroll
            for (int i = 0; i < VE; i++) if (c + i < n) out[c + i] = x[i];
        }
    };
    store(c0, whole0, acc0); store(c1, whole1, acc1);
}

// ---- every instantiation of this header's kernel template (rm_kernel_units.hpp) -----------------------------------------
#define RM_ITEMWEIGHTS_KERNELS_F32(X) X(k_scores_item_weights<float, true>) X(k_scores_item_weights<float, false>)
#define RM_ITEMWEIGHTS_KERNELS_F64(X) X(k_scores_item_weights<double, true>) X(k_scores_item_weights<double, false>)
RM_ITEMWEIGHTS_KERNELS_F32(RM_EXTERN_KERNEL)
RM_ITEMWEIGHTS_KERNELS_F64(RM_EXTERN_KERNEL)

} // namespace rm
