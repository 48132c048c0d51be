// rm_scores.hpp -- the front of a call whose scores are the CALLER'S matrix S[users x items] (rm_calc_metrics_scores_*; Call::scores).
//
// The factor call's sweep does three things for a streamed user: it writes the masked score row k_select_topk / k_rank_streamed
// read (train items carry the NaN sentinel, as does the padding up to the row stride), it leaves the validity statistics of the
// user's CANDIDATES (max, min, has-NaN: PartialStat), and -- through k_pos_scores_flat -- it scores the test entries.  Here the scores
// exist already: k_score_rows copies a user's row of S into that layout and reduces the statistics on the way (2 n s bytes per user:
// bound by HBM), k_pos_scores_given gathers S[user][test item].  Everything behind them is the factor call's finalisation, unchanged.
// S may hold 16-bit scores (IEEE binary16 / bfloat16: ScoreSrc below) under an fp32 call: both kernels widen them in registers.
//
// One difference between a caller's scores and the fma chain's: the chain starts at +0 and never yields -0, and the ordered integer
// keys of k_select_topk / k_pos_place tell the two zeros apart.  Both kernels store +0 for -0 (the contract: +0 == -0, ties by item id).
#pragma once
#include "rm_device.hpp"
#include "rm_kernel_units.hpp"
#include "rm_prep.hpp"

namespace rm {

template <class T> __device__ __forceinline__ T score_sentinel();
template <> __device__ __forceinline__ float score_sentinel<float>() { return nan_sentinel_f(); }
template <> __device__ __forceinline__ double score_sentinel<double>() { return __longlong_as_double(-1ll); }
template <class T> __device__ __forceinline__ T score_canonical(T x) { return x == (T)0 ? (T)0 : x; }      // -0 -> +0; NaN stays

// ---- the element type of the caller's matrix (Src) apart from the type everything is computed in (T) ----------------------------
// rm_*_scores_{f16,bf16} (include/recometrics_hip_half.h): S holds 16-bit patterns, read where they lie and widened EXACTLY to fp32 in
// registers -- bf16 is the upper half of an fp32 (a shift / a mask per score, two scores per dword), IEEE binary16 goes through the
// hardware conversion (v_cvt_f32_f16: subnormals become fp32 normals; the build sets no flush flag and fp16 denormals are on by
// default).  Behind the widening a score is the fp32 call's score: the callbacks of walk_score_row never see Src.
// A 16-byte load of Src holds PIECES pieces of PE = 16 / sizeof(T) scores each -- a piece is what one call of `piece` gets, and what
// k_score_rows stores with one 16-byte store; Src == T: one piece, the load itself.
// (F16Bits / BF16Bits and the widening itself, half_lo / half_hi: rm_half.hpp, shared with the 16-bit factors of rm_prep.hpp)
template <class T> struct ScoreVec {
    typedef T Aligned __attribute__((ext_vector_type(16 / sizeof(T))));
    typedef T Unaligned __attribute__((ext_vector_type(16 / sizeof(T)), aligned(sizeof(T))));
};
template <class T, class Src> struct ScoreSrc;
template <class T> struct ScoreSrc<T, T> {
    static constexpr int PIECES = 1;
    typedef typename ScoreVec<T>::Aligned Raw;
    static __device__ __forceinline__ T widen(T x) { return x; }
    static __device__ __forceinline__ const Raw &part(const Raw &r, int) { return r; }
};
template <class Half> struct ScoreSrcHalf {
    static constexpr int PIECES = 2;
    typedef unsigned Raw __attribute__((ext_vector_type(4)));
    static __device__ __forceinline__ float widen(Half x) { return half_lo(Half{}, (unsigned)x.b); }
    // scores 4 p .. 4 p + 3 of the eight in `r`
    static __device__ __forceinline__ ScoreVec<float>::Aligned part(const Raw &r, int p)
    {
        const unsigned w0 = r[2 * p], w1 = r[2 * p + 1];
        ScoreVec<float>::Aligned y;
        y[0] = half_lo(Half{}, w0); y[1] = half_hi(Half{}, w0); y[2] = half_lo(Half{}, w1); y[3] = half_hi(Half{}, w1);
        return y;
    }
};
template <> struct ScoreSrc<float, F16Bits> : ScoreSrcHalf<F16Bits> {};
template <> struct ScoreSrc<float, BF16Bits> : ScoreSrcHalf<BF16Bits> {};

// NaN-ignoring max / min (a NaN candidate is reported through has_nan, the sentinel never gets here)
__device__ __forceinline__ float stat_max(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ float stat_min(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double stat_max(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ double stat_min(double a, double b) { return __builtin_fmin(a, b); }

// scores of the test entries, by entry (the place of k_pos_scores_flat + k_pos_apply_masked): a test item that is a train item of
// its user scores +inf -- S is not read there -- everything else S[user][item] as given
template <class T, class Src = T>
__global__ __launch_bounds__(256) void k_pos_scores_given(PosArgs<T> a, const Src *S, size_t lds, const int *ent_user, const unsigned char *ent_masked)
{
    if (a.plan->csr_bad & (CSR_BAD_INDPTR | CSR_BAD_INDEX)) return;       // (the test items index the rows of S)
    const long long e = (long long)a.test_p[0] + (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)a.test_p[a.m]) return;
    const int u = ent_user[e];
    const int f = a.flags[u];
    if (!(f & UF_ACTIVE) || (f & UF_ONLY_NDCG)) return;
    const int item = a.test_i[e];
    const T s = ent_masked[e] ? (T)__int_as_float(0x7f800000) : score_canonical<T>(ScoreSrc<T, Src>::widen(S[(size_t)u * lds + (size_t)item]));
    a.pos_tmp[e] = s;
    if (sizeof(T) == 4 && a.pos_key) a.pos_key[e] = ((unsigned long long)ord_key((float)s) << 32) | (unsigned)~item;
}

// ---- the masked score rows and the candidates' statistics ----------------------------------------------------------------------
// A block per streamed user (row).  The row of S is read in aligned 16-byte pieces, with element loads in front of the first aligned
// address and behind the last whole piece (`lds` and the caller's pointer are arbitrary: a row starts wherever it starts); the
// stored row starts 16-byte aligned, so a piece lands at the alignment the head leaves it -- element-aligned vector stores.
// Train items: the row's sorted train items are merged in by a CURSOR over pieces of SCORE_CHUNK items -- per piece the block marks
// the train items that fall into it in an LDS bitmap (each thread takes entries cursor + tid, + 256, ... until one lies beyond the
// piece) and the cursor moves by how many were marked; a score then costs a bit test, not a search.  BASELINE C2's 26,744 items are
// one piece.
constexpr int SCORE_ROW_THREADS = 256;
constexpr int SCORE_CHUNK = 32768;                 // items per piece: a 4 KiB bitmap
constexpr int SCORE_UNROLL = 4;                    // 16-byte loads in flight per thread

// One pass over a row of S, shared by k_score_rows and k_topk_rows (rm_rowtopk.hpp): the pieces of SCORE_CHUNK items with their bitmap
// of train items, and per piece the element loads around the aligned 16-byte middle.  The caller says what happens to a score:
//   elem(i, x, masked)      item i, loaded alone (in front of the first 16-byte boundary, behind the last whole load);
//   piece(i, x, mb)         items i .. i + PE - 1, PE = 16 / sizeof(T): an aligned 16-byte load, or with 16-bit scores one half of it,
//                           widened (ScoreSrc); bit j of `mb` = item i + j is a train item;
//   pass()                  called by EVERY thread of the block in front of each step in which a thread handles at most one element or
//                           one piece (so it may hold a barrier): SCORE_ROW_THREADS * PE scores per step at the most -- a 16-byte
//                           load of 16-bit scores is two steps, so a step is as many scores as in the fp32 call.
// `bitmap` (SCORE_CHUNK / 32 + 2 words) and `sh_taken` are the block's LDS; `cursor` / `tr_end` the user's entries of `train_i`.
template <class T, class Src, class Elem, class Piece, class Pass>
__device__ __forceinline__ void walk_score_row(const Src *src, const int n, const int *train_i, int cursor, const int tr_end,
                                               unsigned *bitmap, int *sh_taken, Elem elem, Piece piece, Pass pass)
{
    typedef ScoreSrc<T, Src> SS;
    constexpr int VE = 16 / (int)sizeof(Src);                                  // scores per 16-byte load
    constexpr int PE = VE / SS::PIECES;                                        // ... and per piece
    typedef typename SS::Raw VT;
    const int tid = threadIdx.x;
    // scores in front of the first 16-byte boundary of the source row
    const int mis = (int)(((size_t)src) & 15);
    // (a pointer that is not even a multiple of the score's size never reaches a 16-byte boundary: element loads throughout)
    const int head = (mis % (int)sizeof(Src)) ? n : min(n, mis ? (16 - mis) / (int)sizeof(Src) : 0);
    for (int c0 = 0; c0 < n; c0 += SCORE_CHUNK) {
        const int c1 = min(n, c0 + SCORE_CHUNK);
        // ---- the train items of [c0, c1) into the bitmap; the cursor moves behind them ----
        for (int i = tid; i < SCORE_CHUNK / 32 + 2; i += SCORE_ROW_THREADS) bitmap[i] = 0u;
        if (tid == 0) *sh_taken = 0;
        __syncthreads();
        int mine = 0;
        for (int e = cursor + tid; e < tr_end; e += SCORE_ROW_THREADS) {
            const int it = train_i[e];
            if (it >= c1) break;
            const unsigned rel = (unsigned)(it - c0);
            if (rel < (unsigned)SCORE_CHUNK) atomicOr(&bitmap[rel >> 5], 1u << (rel & 31));
            mine++;
        }
        if (mine) atomicAdd(sh_taken, mine);
        __syncthreads();
        cursor += *sh_taken;
        auto masked_bits = [&](int i) -> unsigned {                           // bits of items i, i + 1, ... (i in [c0, c1))
            const unsigned rel = (unsigned)(i - c0);
            const unsigned long long w = (unsigned long long)bitmap[rel >> 5] | ((unsigned long long)bitmap[(rel >> 5) + 1] << 32);
            return (unsigned)(w >> (rel & 31));
        };
        // ---- this piece of the row: [lo, hi) element by element around the aligned middle [v0, v1) ----
        const int lo = c0, hi = c1;
        int v0 = lo <= head ? head : head + (lo - head + VE - 1) / VE * VE;   // first aligned piece at or behind lo
        v0 = min(v0, hi);
        const int v1 = v0 + (hi - v0) / VE * VE;
        for (int i0 = lo; i0 < v0; i0 += SCORE_ROW_THREADS) { pass(); const int i = i0 + tid; if (i < v0) elem(i, SS::widen(src[i]), (masked_bits(i) & 1u) != 0u); }
        for (int i0 = v1; i0 < hi; i0 += SCORE_ROW_THREADS) { pass(); const int i = i0 + tid; if (i < hi) elem(i, SS::widen(src[i]), (masked_bits(i) & 1u) != 0u); }
        const int nvec = (v1 - v0) / VE;
        for (int vb = 0; vb < nvec; vb += SCORE_ROW_THREADS * SCORE_UNROLL) {
            VT x[SCORE_UNROLL];
            #pragma unroll
            for (int q = 0; q < SCORE_UNROLL; q++) {
                const int v = vb + q * SCORE_ROW_THREADS + tid;
                if (v < nvec) x[q] = *(const VT *)(src + v0 + v * VE);
            }
            #pragma unroll
            for (int q = 0; q < SCORE_UNROLL; q++) {
                if constexpr (SS::PIECES == 1) {
                    pass();
                    const int v = vb + q * SCORE_ROW_THREADS + tid;
                    if (v < nvec) { const int i = v0 + v * VE; piece(i, x[q], masked_bits(i)); }
                } else {
                    #pragma unroll
                    for (int p = 0; p < SS::PIECES; p++) {
                        pass();
                        const int v = vb + q * SCORE_ROW_THREADS + tid;
                        if (v < nvec) { const int i = v0 + v * VE + p * PE; piece(i, SS::part(x[q], p), masked_bits(i)); }
                    }
                }
            }
        }
        __syncthreads();                                                      // (the bitmap is cleared for the next piece)
    }
}

// max / min / has-NaN of a thread's candidates (-0 counted and handed back as +0), and their reduction over the block
template <class T> struct CandStats {
    T vmax = -(T)INFINITY, vmin = (T)INFINITY; int has_nan = 0;
    __device__ __forceinline__ T take(T x)
    {
        x = score_canonical<T>(x);
        has_nan |= x != x;
        vmax = stat_max(vmax, x); vmin = stat_min(vmin, x);
        return x;
    }
    // thread 0 holds the block's statistics afterwards (`sh_*`: SCORE_ROW_THREADS / WAVE entries each; holds a barrier)
    __device__ __forceinline__ void reduce_block(T *sh_max, T *sh_min, int *sh_nan)
    {
        #pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            vmax = stat_max(vmax, __shfl_xor(vmax, s)); vmin = stat_min(vmin, __shfl_xor(vmin, s)); has_nan |= __shfl_xor(has_nan, s);
        }
        const int tid = threadIdx.x, wv = tid >> 6;
        if ((tid & 63) == 0) { sh_max[wv] = vmax; sh_min[wv] = vmin; sh_nan[wv] = has_nan; }
        __syncthreads();
        if (tid == 0)
            for (int w = 1; w < SCORE_ROW_THREADS / WAVE; w++) { vmax = stat_max(vmax, sh_max[w]); vmin = stat_min(vmin, sh_min[w]); has_nan |= sh_nan[w]; }
    }
};

template <class T, class Src = T> struct ScoreRowArgs {
    int n, n_rows, stream_slot0, n_part;
    const int *slot_user, *train_p, *train_i;
    const Src *S; size_t lds;
    T *rows; long long row_ld;                     // [n_rows][row_ld], row_ld >= n, rows 16-byte aligned
    PartialStat<T> *pst;                           // [n_slots][n_part]: part 0 is written
};

template <class T, class Src = T>
__global__ __launch_bounds__(SCORE_ROW_THREADS) void k_score_rows(ScoreRowArgs<T, Src> a)
{
    constexpr int VE = 16 / (int)sizeof(T);
    typedef typename ScoreVec<T>::Aligned VT;
    typedef typename ScoreVec<T>::Unaligned VTU;
    __shared__ unsigned bitmap[SCORE_CHUNK / 32 + 2];
    __shared__ int sh_taken;
    __shared__ T sh_max[SCORE_ROW_THREADS / WAVE], sh_min[SCORE_ROW_THREADS / WAVE];
    __shared__ int sh_nan[SCORE_ROW_THREADS / WAVE];
    const int d = blockIdx.x, tid = threadIdx.x;
    if (d >= a.n_rows) return;
    const int slot = a.stream_slot0 + d;
    const int u = a.slot_user[slot];
    const int n = a.n;
    T *dst = a.rows + (size_t)d * (size_t)a.row_ld;
    CandStats<T> st;
    const T sentinel = score_sentinel<T>();
    walk_score_row<T, Src>(a.S + (size_t)u * a.lds, n, a.train_i, a.train_p[u], a.train_p[u + 1], bitmap, &sh_taken,
        [&](int i, T x, bool masked) { dst[i] = masked ? sentinel : st.take(x); },
        [&](int i, const VT &x, unsigned mb) {
            VT y;
            #pragma unroll
            for (int j = 0; j < VE; j++) y[j] = ((mb >> j) & 1u) ? sentinel : st.take(x[j]);
            *(VTU *)(dst + i) = y;
        },
        [] {});
    // the padding up to the row stride: masked, like the items beyond n of the sweep's last tile
    for (long long i = (long long)n + tid; i < a.row_ld; i += SCORE_ROW_THREADS) dst[i] = sentinel;
    // ---- the block's statistics -> part 0 of the slot ----
    st.reduce_block(sh_max, sh_min, sh_nan);
    if (tid == 0) {
        PartialStat<T> ps;
        ps.vmax = st.vmax; ps.vmin = st.vmin; ps.rocsum = 0; ps.has_nan = st.has_nan; ps.pad = 0;
        a.pst[(size_t)slot * a.n_part] = ps;
    }
}

// ---- every instantiation of this header's kernel templates (rm_kernel_units.hpp) ----------------------------------------
#define RM_SCORES_KERNELS(X, T) X(k_pos_scores_given<T>) X(k_score_rows<T>)
#define RM_SCORES_KERNELS_F32(X) RM_SCORES_KERNELS(X, float)
#define RM_SCORES_KERNELS_F64(X) RM_SCORES_KERNELS(X, double)
#define RM_SCORES_KERNELS_HALF(X) X(k_pos_scores_given<float, F16Bits>) X(k_score_rows<float, F16Bits>) \
                                  X(k_pos_scores_given<float, BF16Bits>) X(k_score_rows<float, BF16Bits>)
RM_SCORES_KERNELS_F32(RM_EXTERN_KERNEL)
RM_SCORES_KERNELS_F64(RM_EXTERN_KERNEL)
RM_SCORES_KERNELS_HALF(RM_EXTERN_KERNEL)

} // namespace rm
