// rm_candidates.hpp -- the ordered top-K of a user's CANDIDATE SET (rm_recommend_candidates_*; Call::cand, k_top <= ROW_TOPK_MAX_K):
// gather the candidates' item rows, score them against the user's factors, select -- one kernel, one pass, no score stored in between.
//
// The candidates of user u are the distinct ids of row u of the candidate CSR (validated and sorted by the plan stage: an id outside
// [0, n) never gets here, and the kernel returns when the plan says so).  The score of (u, item) is the library's: the k-ordered fma
// chain from +0 (fma_chain_step), the bits rm_recommend_* writes.  Order: score descending, then item ascending; -0 is +0.
//
// Geometry.  One block of SCORE_ROW_THREADS (256) per user, so TopkPairs / topk_sort_desc / CandStats of rm_rowtopk.hpp serve as they
// are.  A STEP is 256 consecutive entries of the row, 64 per wavefront, one per lane.  An entry equal to its predecessor in the row
// is a duplicate and takes part in nothing; a wavefront none of whose 64 entries is live skips the step's gather.
//
// Gather.  FlatDot's (rm_prep.hpp), a piece of 64 bytes of every row at a time: four lanes cover a row's piece with 16 bytes each, a
// load instruction covers 16 rows, four instructions the wavefront's 64 -- 4 KiB of item factors per wavefront and piece.  The pieces
// are written to a padded LDS image (80-byte rows: the sixteen lanes of a 16-byte read group sit on sixteen different slots of the
// bank row) and every lane reads its own candidate's piece back: the exchange is fenced as FlatDot's is.  Element loads where B or
// ldb * sizeof(T) is not 16-byte aligned and at a partial last piece; bits beyond k are zero.
//
// The user's factors are the same for all 256 lanes.  A wavefront holds the piece in ONE register: lane f < CH has A[u][k0 + f] -- a
// single coalesced load of 64 bytes per wavefront and piece, where FlatDot's lanes load 64 bytes EACH for a row that never changes
// -- and the chain reads it with v_readlane (a scalar operand of the fma).  No LDS, no barrier.
//
// Loads in flight.  The gather is bound by latency, not by arithmetic: the loop over (step, piece) is software-pipelined by one piece,
// across the step's end.  The loads of the NEXT piece -- the next step's first piece behind a step's last, its item ids having been
// read a whole step ahead -- are issued before the fences and the fma chain of the current one: 4 KiB + 64 B per wavefront, 16 KiB
// per block in flight while the chain runs.  LDS per block: the pair buffer 16 KiB (fp64 24 KiB) + the image 4 x 64 x 80 B = 20 KiB
// + the statistics' few words = 36 KiB (44 KiB): four (three) blocks, i.e. sixteen (twelve) wavefronts and 64 (48) KiB of loads in
// flight per compute unit of 160 KiB.
//
// No matrix instruction: with one user per block a 32 x 32 MFMA tile would carry ONE live column in 32 -- 3 % of the unit's work
// useful, against a chain of k fma per lane that hides behind the gather anyway.
//
// Selection.  Every live candidate is a pair TopkPairs<T>::make(st.take(s), item) (CandStats: -0 -> +0, max / min / has-NaN for the
// status).  Rows of at most ROW_TOPK_CAP entries -- the usual case -- append every pair (one LDS atomic per wavefront and step) and
// sort once at the end: no bound, no compaction, no barrier inside the row.  Longer rows follow k_topk_rows: in front of a step that
// could overflow the buffer (count + 256 > CAP) the block sorts, keeps K, and the K-th becomes the bound a pair has to beat.  The
// tail is k_topk_rows': final network, min(K, count) entries, -1 / NaN behind them, the status; consecutive threads on consecutive
// addresses.  Status 1: the row is empty.  Status 2: a CANDIDATE's score is NaN / +-Inf.
#pragma once
#include "rm_prep.hpp"
#include "rm_rowtopk.hpp"
#include "rm_kernel_units.hpp"

namespace rm {

constexpr int CAND_STEP = SCORE_ROW_THREADS;                         // entries of the row per step of the block
static_assert(ROW_TOPK_MAX_K + CAND_STEP <= ROW_TOPK_CAP, "the K survivors of a compaction and one step's appends must fit the buffer");

template <class T> struct CandArgs {
    int k, K;
    const T *A; size_t lda; const T *B; size_t ldb;
    const int *cand_p, *cand_i;                    // the candidate rows, validated and sorted (run(): the plan stage)
    const Plan *plan;
    int *idx; T *score; int *status;               // the caller's arrays [m][K], [m][K] (may be null), [m]
};

// A block per user of the call.
template <class T>
__global__ __launch_bounds__(SCORE_ROW_THREADS) void k_topk_candidates(CandArgs<T> a)
{
    typedef TopkPairs<T> B;
    typedef typename B::Pair Pair;
    typedef FlatDot<T> G;                                            // (the gather's geometry; A is not read FlatDot's way)
    typedef typename G::VT VT;
    constexpr int CH = G::CH, VE = G::VE, LD = G::LD, LPR = G::LPR, RPI = G::RPI, Q = WAVE / RPI;
    constexpr int WAVES = SCORE_ROW_THREADS / WAVE, CAP = ROW_TOPK_CAP;
    __shared__ B buf;
    __shared__ __attribute__((aligned(16))) T rows[WAVES][WAVE][LD];
    __shared__ int sh_count, sh_status;
    __shared__ T sh_max[WAVES], sh_min[WAVES];
    __shared__ int sh_nan[WAVES];
    if (a.plan->csr_bad & (CSR_BAD_INDPTR | CSR_BAD_INDEX)) return;   // (the candidates index the item factors)
    const int u = blockIdx.x, tid = threadIdx.x, K = a.K, k = a.k;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r0 = a.cand_p[u], r1 = a.cand_p[u + 1];
    int *out_i = a.idx + (size_t)u * K;
    T *out_s = a.score ? a.score + (size_t)u * K : nullptr;
    int status = r1 - r0 < 1 ? 1 : 0, W = 0;
    if (status == 0) {
        if (tid == 0) sh_count = 0;
        __syncthreads();                                             // (in front of every append)
        const bool longrow = r1 - r0 > CAP;                          // (entries, duplicates included: C <= CAP whenever this is false)
        const T *Au = a.A + (size_t)u * a.lda;
        const int rsub = lane / LPR, piece = lane % LPR;
        const bool vec_ok = ((((size_t)a.B) | (a.ldb * sizeof(T))) & 15) == 0;
        // the entries of a step as this wavefront sees them: the lane's item, whether it is a live candidate, the rows the lane helps to fetch
        struct Ids { int item; bool mine; unsigned long long live; const T *brow[Q]; };
        const auto ids_of = [&](int base) {
            const int e = base + wv * WAVE + lane;
            Ids s;
            const bool in = e < r1;
            s.item = in ? a.cand_i[e] : 0;
            s.mine = in && !(e > r0 && a.cand_i[e - 1] == s.item);
            s.live = __ballot(s.mine);
            #pragma unroll
            for (int q = 0; q < Q; q++) s.brow[q] = a.B + (size_t)__shfl(s.item, q * RPI + rsub) * a.ldb;
            return s;
        };
        // the loads of one piece: 16 bytes of four rows per lane, and the lane's factor of the user's piece
        const auto fetch = [&](const Ids &s, int k0, VT (&bv)[Q], T &av) {
            const int e0 = k0 + piece * VE;                          // first factor of this lane's 16 bytes
            #pragma unroll
            for (int q = 0; q < Q; q++) {
                const int p = q * RPI + rsub;
                const T *brow = s.brow[q];
                VT x = {};                                           // (zero bits: +0 beyond k)
                if (((s.live >> p) & 1) && e0 < k) {
                    if (vec_ok && e0 + VE <= k) x = *(const VT *)(brow + e0);
                    else {
                        #pragma unroll
                        for (int i = 0; i < VE; i++) if (e0 + i < k) x[i] = brow[e0 + i];
                    }
                }
                bv[q] = x;
            }
            av = (lane < CH && k0 + lane < k) ? Au[k0 + lane] : (T)0;
        };
        Pair bound = B::lowest();
        CandStats<T> st;
        Ids cur = ids_of(r0);
        VT bv[Q]; T av = 0;
        if (cur.live) fetch(cur, 0, bv, av);
        for (int base = r0; base < r1; base += CAND_STEP) {
            const bool more = base + CAND_STEP < r1;
            Ids nxt{};
            if (more) nxt = ids_of(base + CAND_STEP);                // (a step ahead: the next step's first loads need them)
            if (longrow) {
                // the count as the step before left it, the same for every thread: nobody appends between the two barriers
                __syncthreads();
                const int cnt = sh_count;
                __syncthreads();
                if (cnt + CAND_STEP > CAP) {
                    topk_sort_desc<T>(buf, cnt);                     // (cnt > CAP - CAND_STEP >= K)
                    bound = buf.get(K - 1);
                    if (tid == 0) sh_count = K;
                    __syncthreads();
                }
            }
            T s = 0;
            if (cur.live) {
                for (int k0 = 0; k0 < k; k0 += CH) {
                    #pragma unroll
                    for (int q = 0; q < Q; q++) *(VT *)&rows[wv][q * RPI + rsub][piece * VE] = bv[q];
                    const T a_cur = av;
                    // the next piece's loads, in flight while this piece's chain runs
                    if (k0 + CH < k) fetch(cur, k0 + CH, bv, av);
                    else if (nxt.live) fetch(nxt, 0, bv, av);
                    // (the pieces change lanes through LDS: fenced like FlatDot's, not left to the compiler's alias analysis)
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
                    const T *r = rows[wv][lane];
                    if (k0 + CH <= k) {
                        #pragma unroll
                        for (int j = 0; j < CH / VE; j++) {
                            const VT b = *(const VT *)(r + j * VE);
                            #pragma unroll
                            for (int i = 0; i < VE; i++) s = fma_chain_step(lane_bcast<T>(a_cur, j * VE + i), b[i], s);
                        }
                    } else {
                        #pragma unroll
                        for (int j = 0; j < CH / VE; j++) {
                            const VT b = *(const VT *)(r + j * VE);
                            #pragma unroll
                            for (int i = 0; i < VE; i++) if (k0 + j * VE + i < k) s = fma_chain_step(lane_bcast<T>(a_cur, j * VE + i), b[i], s);
                        }
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();      // the image is rewritten by the next piece
                }
            } else if (nxt.live) fetch(nxt, 0, bv, av);              // (an idle step of this wavefront in front of a live one: duplicates only)
            if (cur.mine) {
                const Pair p = B::make(st.take(s), cur.item);
                if (!longrow || B::above(p, bound)) {
                    // the lanes that got here, counted by their mask: the first one takes the places for all of them
                    const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, 0u));
                    int at0 = 0;
                    if (rank == 0) at0 = atomicAdd(&sh_count, __popcll(act));
                    const int at = __builtin_amdgcn_readfirstlane(at0) + rank;
                    if (at < CAP) buf.set(at, p);                    // (never false: a short row has at most CAP entries, a long one compacts)
                }
            }
            cur = nxt;
        }
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
#define RM_CANDIDATES_KERNELS_F32(X) X(k_topk_candidates<float>)
#define RM_CANDIDATES_KERNELS_F64(X) X(k_topk_candidates<double>)
RM_CANDIDATES_KERNELS_F32(RM_EXTERN_KERNEL)
RM_CANDIDATES_KERNELS_F64(RM_EXTERN_KERNEL)

} // namespace rm
