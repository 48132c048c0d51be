// rm_rowtopk.hpp -- the ordered top-K of a user's row of the caller's score matrix, selected while the row is read
// (rm_recommend_scores_*; Call::reco && Call::scores, k_top <= ROW_TOPK_MAX_K).
//
// k_score_rows + k_select_topk + k_finalize_reco store a masked copy of every row and read it back several times.  k_topk_rows reads
// the row of S once (walk_score_row: rm_scores.hpp), masks it in flight and keeps nothing per user but the answer:
//   * every candidate is one totally ordered PAIR (ord_key(score), ~item): larger = better score, then smaller item id -- ties need no
//     special case;
//   * the block keeps a BOUND pair (at first below everything) and an append buffer of ROW_TOPK_CAP pairs in LDS; a candidate strictly
//     above the bound is appended, one LDS atomic per wavefront and step (the lanes that append are counted by their lane mask);
//   * in front of a step of the walk that could overflow the buffer (count + ROW_TOPK_PASS > ROW_TOPK_CAP) the block COMPACTS: a bitonic
//     network sorts the pairs in LDS, descending, the first K stay and the K-th becomes the bound.  A step appends ROW_TOPK_PASS pairs
//     at the most and K + ROW_TOPK_PASS <= ROW_TOPK_CAP, so no append can land outside the buffer (and its index is checked anyway).
//     It also compacts as soon as the buffer holds max(4 K, 256) pairs: a small network early is cheaper than a full one later;
//   * behind the row the same network sorts what is left; min(K, C) entries, -1 / NaN behind them and the status go straight to the
//     caller's arrays, consecutive threads on consecutive addresses.
// 16-bit scores (Src = F16Bits / BF16Bits, T = float: rm_scores.hpp): a 16-byte load is 8 scores, which walk_score_row hands over in two
// pieces of four with a step in front of each -- ROW_TOPK_PASS, ROW_TOPK_CAP and `early` are the fp32 kernel's.
// The validity statistics (max / min / has-NaN of the CANDIDATES, -0 as +0) are reduced on the way as k_score_rows does: status 2
// overrides the list.  A score at an excluded item takes part in nothing.
#pragma once
#include "rm_scores.hpp"
#include "rm_finalize.hpp"
#include "rm_kernel_units.hpp"

namespace rm {

constexpr int ROW_TOPK_MAX_K = 1024;
constexpr int ROW_TOPK_CAP = 2048;                                   // pairs of the append buffer: a power of two (the network's size)
template <class T> constexpr int row_topk_pass() { return SCORE_ROW_THREADS * (16 / (int)sizeof(T)); }      // appends of one step at the most
static_assert(ROW_TOPK_MAX_K + row_topk_pass<float>() <= ROW_TOPK_CAP && ROW_TOPK_MAX_K + row_topk_pass<double>() <= ROW_TOPK_CAP,
              "the K survivors of a compaction and one step's appends must fit the buffer");
static_assert((ROW_TOPK_CAP & (ROW_TOPK_CAP - 1)) == 0, "the bitonic network sorts a power of two");

// the append buffer: fp32 one 64-bit word per pair (as k_pos_scores_given packs it), fp64 a 64-bit key plus a 32-bit word
template <class T> struct TopkPairs;
template <> struct TopkPairs<float> {
    struct Pair { unsigned long long v; };
    unsigned long long p[ROW_TOPK_CAP];
    static __device__ __forceinline__ Pair make(float s, int item) { return Pair{((unsigned long long)ord_key(s) << 32) | (unsigned)~item}; }
    static __device__ __forceinline__ Pair lowest() { return Pair{0ull}; }
    static __device__ __forceinline__ bool above(Pair a, Pair b) { return a.v > b.v; }
    static __device__ __forceinline__ int item(Pair x) { return (int)~(unsigned)x.v; }
    static __device__ __forceinline__ float score(Pair x) { return ord_unkey((unsigned)(x.v >> 32)); }
    __device__ __forceinline__ Pair get(int i) const { return Pair{p[i]}; }
    __device__ __forceinline__ void set(int i, Pair x) { p[i] = x.v; }
};
template <> struct TopkPairs<double> {
    struct Pair { unsigned long long k; unsigned lo; };
    unsigned long long key[ROW_TOPK_CAP]; unsigned low[ROW_TOPK_CAP];
    static __device__ __forceinline__ Pair make(double s, int item) { return Pair{ord_key(s), (unsigned)~item}; }
    static __device__ __forceinline__ Pair lowest() { return Pair{0ull, 0u}; }
    static __device__ __forceinline__ bool above(Pair a, Pair b) { return a.k > b.k || (a.k == b.k && a.lo > b.lo); }
    static __device__ __forceinline__ int item(Pair x) { return (int)~x.lo; }
    static __device__ __forceinline__ double score(Pair x) { return ord_unkey(x.k); }
    __device__ __forceinline__ Pair get(int i) const { return Pair{key[i], low[i]}; }
    __device__ __forceinline__ void set(int i, Pair x) { key[i] = x.k; low[i] = x.lo; }
};

// The first `cnt` pairs of the buffer, sorted descending (the selection a later pull request can hand to the metric path).  Called by
// every thread of a block of SCORE_ROW_THREADS with the same cnt <= ROW_TOPK_CAP, behind a barrier that has made the pairs visible;
// ends with a barrier.  The network runs over the next power of two, the places up to it filled with the lowest pair.
template <class T>
__device__ __forceinline__ void topk_sort_desc(TopkPairs<T> &buf, const int cnt)
{
    typedef TopkPairs<T> B;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = cnt + tid; i < P; i += SCORE_ROW_THREADS) buf.set(i, B::lowest());
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += SCORE_ROW_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const typename B::Pair x = buf.get(i), y = buf.get(l);
                const bool desc = (i & k) == 0;                            // (k == P: every pair -- the whole buffer descends)
                if (desc ? B::above(y, x) : B::above(x, y)) { buf.set(i, y); buf.set(l, x); }
            }
            __syncthreads();
        }
}

template <class T, class Src = T> struct RowTopkArgs {
    int n, K;
    const int *train_p, *train_i;                  // the exclusion rows, validated and sorted (run(): the plan stage)
    const Src *S; size_t lds;
    int *idx; T *score; int *status;               // the caller's arrays [m][K], [m][K] (may be null), [m]
};

// A block per user of the call.
template <class T, class Src = T>
__global__ __launch_bounds__(SCORE_ROW_THREADS) void k_topk_rows(RowTopkArgs<T, Src> a)
{
    typedef TopkPairs<T> B;
    typedef typename B::Pair Pair;
    typedef typename ScoreVec<T>::Aligned VT;
    constexpr int VE = 16 / (int)sizeof(T), CAP = ROW_TOPK_CAP, PASS = row_topk_pass<T>();
    // (16-bit scores: walk_score_row hands a 16-byte load over in two pieces with a step in front of each, so a step is VE scores per
    // thread as in the fp32 call and the buffer and `early` stay what they are)
    static_assert(16 / (int)sizeof(Src) == VE * ScoreSrc<T, Src>::PIECES && ROW_TOPK_MAX_K + PASS <= CAP,
                  "the K survivors of a compaction and one step's appends must fit the buffer");
    __shared__ B buf;
    __shared__ unsigned bitmap[SCORE_CHUNK / 32 + 2];
    __shared__ int sh_taken, sh_count, sh_status;
    __shared__ T sh_max[SCORE_ROW_THREADS / WAVE], sh_min[SCORE_ROW_THREADS / WAVE];
    __shared__ int sh_nan[SCORE_ROW_THREADS / WAVE];
    const int u = blockIdx.x, tid = threadIdx.x, K = a.K, n = a.n;
    const int tr0 = a.train_p[u], tr1 = a.train_p[u + 1];
    int *out_i = a.idx + (size_t)u * K;
    T *out_s = a.score ? a.score + (size_t)u * K : nullptr;
    int status = (n - (tr1 - tr0) < 1) ? 1 : 0, W = 0;              // 1: the row excludes the whole catalogue -- S is not read
    if (status == 0) {
        if (tid == 0) sh_count = 0;                                  // (walk_score_row's first barrier is in front of every append)
        Pair bound = B::lowest();
        // (... and EARLY, as soon as the buffer holds 4 K pairs, 256 at least: the first bound comes from a network over the first
        // step's 1,024 pairs instead of a full buffer's 2,048, and with a bound in place few candidates are appended at all)
        const int early = max(4 * K, 256);
        CandStats<T> st;
        auto offer = [&](int i, T x, bool masked) {
            if (masked) return;
            const Pair p = B::make(st.take(x), i);
            if (!B::above(p, bound)) return;
            // the lanes that got here, counted by their mask: the first one takes the places for all of them
            const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, 0u));
            int base = 0;
            if (rank == 0) base = atomicAdd(&sh_count, __popcll(act));
            const int at = __builtin_amdgcn_readfirstlane(base) + rank;
            if (at < CAP) buf.set(at, p);                            // (never false: see `pass`)
        };
        walk_score_row<T, Src>(a.S + (size_t)u * a.lds, n, a.train_i, tr0, tr1, bitmap, &sh_taken,
            offer,
            [&](int i, const VT &x, unsigned mb) {
                #pragma unroll
                for (int j = 0; j < VE; j++) offer(i + j, x[j], ((mb >> j) & 1u) != 0u);
            },
            [&] {
                // the count as the step before left it, the same for every thread: nobody appends between the two barriers
                __syncthreads();
                const int cnt = sh_count;
                __syncthreads();
                if (cnt + PASS <= CAP && cnt < early) return;
                topk_sort_desc<T>(buf, cnt);                         // (cnt > CAP - PASS >= K, or cnt >= early > K)
                bound = buf.get(K - 1);
                if (tid == 0) sh_count = K;
                __syncthreads();
            });
        __syncthreads();
        const int cnt = min(sh_count, CAP);
        topk_sort_desc<T>(buf, cnt);
        st.reduce_block(sh_max, sh_min, sh_nan);
        if (tid == 0) sh_status = (st.has_nan || st.vmax == (T)INFINITY || st.vmin == -(T)INFINITY) ? 2 : 0;
        __syncthreads();
        status = sh_status;
        W = status ? 0 : min(K, cnt);
    }
    for (int t = tid; t < K; t += SCORE_ROW_THREADS) {
        int it = -1; T s = (T)qnan<float>();
        if (t < W) { const Pair p = buf.get(t); it = B::item(p); s = B::score(p); }
        out_i[t] = it;
        if (out_s) out_s[t] = s;
    }
    if (tid == 0) a.status[u] = status;
}

// ---- every instantiation of this header's kernel template (rm_kernel_units.hpp) -----------------------------------------
#define RM_ROWTOPK_KERNELS_F32(X) X(k_topk_rows<float>)
#define RM_ROWTOPK_KERNELS_F64(X) X(k_topk_rows<double>)
#define RM_ROWTOPK_KERNELS_HALF(X) X(k_topk_rows<float, F16Bits>) X(k_topk_rows<float, BF16Bits>)
RM_ROWTOPK_KERNELS_F32(RM_EXTERN_KERNEL)
RM_ROWTOPK_KERNELS_F64(RM_EXTERN_KERNEL)
RM_ROWTOPK_KERNELS_HALF(RM_EXTERN_KERNEL)

} // namespace rm
