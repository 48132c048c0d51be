// rm_candmetrics.hpp -- the ten metrics of a user over its CANDIDATE SET (rm_calc_metrics_candidates_*; Call::cand without Call::reco):
// gather the candidates' item rows, score them, rank the WHOLE row, find the test items in the ranking, write the outputs -- one
// kernel, one pass per user, nothing in device memory between the gather and the outputs.
//
// Contract.  The pool of user u is the set of distinct ids of row u of the candidate CSR (C of them; validated and sorted by the plan
// stage), scores and order are k_topk_candidates' (rm_candidates.hpp: the k-ordered fma chain from +0, score descending then item
// ascending, -0 is +0, no tie noise).  Every output is what k_classify + the sweep + k_finalize write for the train matrix that is
// the complement of the candidate row, without noise and with cold start considered: eligibility from (npos, C, K, the request),
// validity from the ranking's first, W-th and last score and the NaN statistics, the top-K walk, the NaN overrides, ROC / PR-AUC
// from the positives' ranks, the NDCG normalisation with its quirks (rm_finalize.hpp k_finalize is the text followed here, line by
// line).  A test item that is not among the user's candidates makes every requested output of that user NaN.
//
// Teams.  TEAM = 64: a WAVEFRONT per user, rows of at most 256 entries (the protocols' "1 positive + 99 negatives"), four users per
// block of 256 threads and no block barrier anywhere: every exchange is fenced per wavefront, the append counter is a register.
// TEAM = 256: a BLOCK per user, rows of 257 .. ROW_TOPK_CAP entries, k_topk_candidates' short-row path (append everything, one
// topk_sort_desc at the end).  Both kernels are launched over all users of the call and return at once for a user of the other class.
//
// Gather.  k_topk_candidates': FlatDot's geometry (64-byte pieces, four lanes a row, 80-byte rows of the LDS image), the user's
// piece in one register read with v_readlane, the loads of the next piece in flight while the chain of this one runs.
//
// Ranking.  All C pairs (ord_key(score), ~item) are sorted descending, so a positive's exact rank is its place in the buffer.  The
// wavefront team sorts its own 256-pair segment with a bitonic network fenced per wavefront.
//
// Behind the sort, both teams alike:
//   hits     the test row's ids are staged in LDS; every lane takes places of the ranking and looks its item up (binary search); a
//            ballot / prefix count packs the hits, in rank order, into a list of (place, index in the test row).  Fewer hits than
//            test items: one is no candidate -- NaN.
//   sums     P / TP / R / Hit / RR and ROC-AUC are exact integers up to their last division (the sum of the positives' ranks is
//            reduced in parallel; the AUC is formed as finalize_auc forms it).  AP / TAP / DCG / PR-AUC are fp64 sums in the
//            reference's order: their TERMS (hits / (place + 1), value / log2(place + 2)) are made in parallel, ONE lane adds them
//            up left to right and leaves the running sums per hit in LDS -- the oracle's bits, no parallel reduction.
//   outputs  not cumulative: a lane per metric.  Cumulative: a lane per place ix < K -- hits(ix) is the number of listed hits at
//            or in front of ix (binary search in the list), the running sums are read at that hit; consecutive lanes write
//            consecutive addresses; the tail beyond C and the NaN overrides are k_finalize's.
//   ideal    the test values, descending, by the team's network (they are at most as many as the candidates); one lane adds the
//   DCG      discounts up in order and leaves the running sum per place; NaN / Inf / <= 0 rules and quirks Q5 / Q6 as k_finalize.
//
// LDS.  Per team: the pair buffer (8 or 12 bytes a pair) and one region that is first the gather's image and then the test ids /
// the running AP sums, the hit list and the running DCG sums.  Wavefront team: 2 + 5 KiB (fp64 3 + 5) per user, 28.1 (32.1) KiB per
// block: five (four) blocks, twenty (sixteen) users in flight per compute unit of 160 KiB.  Block team: 16 + 24 KiB (fp64 24 + 24):
// three blocks per compute unit.
//
// No matrix instruction, for rm_candidates.hpp's reason: one user per team.
#pragma once
#include "rm_candidates.hpp"

namespace rm {

constexpr int CANDM_WAVE_ROW = 256;                                  // entries of the longest row a wavefront team takes

template <class T> struct CandMetricArgs {
    int k, K, req, cumulative, min_items_pool, min_pos_test;         // (the two clamped as reference recometrics.hpp:390-393)
    const T *A; size_t lda; const T *B; size_t ldb;
    const int *cand_p, *cand_i;                                      // the candidate rows, validated and sorted (run(): the plan stage)
    const int *test_p, *test_i; const T *test_v;                     // the test rows, validated and sorted
    const Plan *plan; const double *log2tab;
    T *out[10];                                                      // p, tp, r, ap, tap, ndcg, hit, rr [m][K or 1]; roc, pr [m]
};

// the wavefront team's pair buffer: TopkPairs' pairs, CANDM_WAVE_ROW of them
template <class T> struct WavePairs;
template <> struct WavePairs<float> {
    typedef TopkPairs<float>::Pair Pair;
    unsigned long long p[CANDM_WAVE_ROW];
    __device__ __forceinline__ Pair get(int i) const { return Pair{p[i]}; }
    __device__ __forceinline__ void set(int i, Pair x) { p[i] = x.v; }
};
template <> struct WavePairs<double> {
    typedef TopkPairs<double>::Pair Pair;
    unsigned long long key[CANDM_WAVE_ROW]; unsigned low[CANDM_WAVE_ROW];
    __device__ __forceinline__ Pair get(int i) const { return Pair{key[i], low[i]}; }
    __device__ __forceinline__ void set(int i, Pair x) { key[i] = x.k; low[i] = x.lo; }
};

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// topk_sort_desc for one wavefront and its own segment: the first `cnt` pairs, descending; ends fenced
template <class T>
__device__ __forceinline__ void wave_sort_desc(WavePairs<T> &buf, const int cnt, const int lane)
{
    typedef TopkPairs<T> B;
    int P = 2;
    while (P < cnt) P <<= 1;
    for (int i = cnt + lane; i < P; i += WAVE) buf.set(i, B::lowest());
    wave_sync();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < (P >> 1); t += WAVE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const typename B::Pair x = buf.get(i), y = buf.get(l);
                const bool desc = (i & k) == 0;
                if (desc ? B::above(y, x) : B::above(x, y)) { buf.set(i, y); buf.set(l, x); }
            }
            wave_sync();
        }
}

// what a team shares beside its buffers
struct CandTeamWords {
    int count, nh_top, bad; unsigned sum_ranks;
    int wcnt[SCORE_ROW_THREADS / WAVE], wnan[SCORE_ROW_THREADS / WAVE];
    double ap_full, avg_p, dcg, idcg;
};

template <class T, int TEAM>
__global__ __launch_bounds__(SCORE_ROW_THREADS) void k_metrics_candidates(CandMetricArgs<T> a, int m)
{
    static_assert(TEAM == WAVE || TEAM == SCORE_ROW_THREADS, "a wavefront or a block per user");
    typedef TopkPairs<T> B;
    typedef typename B::Pair Pair;
    typedef FlatDot<T> G;
    typedef typename G::VT VT;
    typedef typename std::conditional<TEAM == WAVE, WavePairs<T>, TopkPairs<T>>::type Buf;
    constexpr int CH = G::CH, VE = G::VE, LD = G::LD, LPR = G::LPR, RPI = G::RPI, Q = WAVE / RPI;
    constexpr int TW = TEAM / WAVE, UPB = SCORE_ROW_THREADS / TEAM;             // wavefronts per team, users per block
    constexpr int CAPT = TEAM == WAVE ? CANDM_WAVE_ROW : ROW_TOPK_CAP;           // entries of the longest row of the team's class
    constexpr int STEPS = CAPT / TEAM;                                           // places of the ranking per thread
    constexpr int RUN = CAPT < ROW_TOPK_MAX_K ? CAPT : ROW_TOPK_MAX_K;           // hits in front of W = min(K, C) at the most
    // the region behind the gather: [test ids, then running AP sums][hit list][running DCG sums]
    constexpr int OFF_HIT = CAPT * 4 > RUN * 8 ? CAPT * 4 : RUN * 8, OFF_DCG = OFF_HIT + CAPT * 4, IMAGE = TW * WAVE * LD * (int)sizeof(T);
    constexpr int REGION = OFF_DCG + RUN * 8 > IMAGE ? OFF_DCG + RUN * 8 : IMAGE;
    __shared__ Buf bufs[UPB];
    __shared__ __attribute__((aligned(16))) char regions[UPB][REGION];
    __shared__ CandTeamWords words[UPB];
    if (a.plan->csr_bad & (CSR_BAD_INDPTR | CSR_BAD_INDEX)) return;   // (the candidates index the item factors)
    const int tid = threadIdx.x, lane = tid & 63;
    const int team = TEAM == WAVE ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;
    const int wv = TEAM == WAVE ? 0 : __builtin_amdgcn_readfirstlane(tid >> 6);  // the wavefront inside its team
    const int tt = TEAM == WAVE ? lane : tid;                                   // the thread inside its team
    const int u = blockIdx.x * UPB + team;
    if (u >= m) return;
    const int r0 = a.cand_p[u], r1 = a.cand_p[u + 1], len = r1 - r0;
    if (TEAM == WAVE ? len > CANDM_WAVE_ROW : (len <= CANDM_WAVE_ROW || len > ROW_TOPK_CAP)) return;   // the other team's user (longer rows: the host has refused the call)
    const auto team_sync = [] { if (TEAM == WAVE) wave_sync(); else __syncthreads(); };
    Buf &buf = bufs[team];
    char *region = regions[team];
    CandTeamWords &w = words[team];
    T (*rows)[WAVE][LD] = (T (*)[WAVE][LD])region;
    int *tids = (int *)region; double *run_ap = (double *)region;
    unsigned *hitl = (unsigned *)(region + OFF_HIT); double *run_dcg = (double *)(region + OFF_DCG);
    double *terms = (double *)&buf;                                  // CAPT doubles over the pairs, once the ranking has been read
    const int K = a.K, k = a.k, req = a.req;
    if (K > ROW_TOPK_MAX_K) return;                                  // (the host has refused such a call: RUN running sums per team)
    const bool cum = a.cumulative != 0;
    const int te0 = a.test_p[u], npos = a.test_p[u + 1] - te0;
    const auto all_nan = [&] {
        for (int q = 0; q < 10; q++) {
            T *arr = a.out[q];
            if (!arr) continue;
            const int per = (q < 8 && cum) ? K : 1;
            for (int i = tt; i < per; i += TEAM) arr[(size_t)u * per + i] = qnan<T>();
        }
    };
    if (npos <= 0 || len < 1) { all_nan(); return; }

    // ---- gather, score, append (k_topk_candidates' short-row path) ----
    if (tt == 0) { w.count = 0; w.nh_top = 0; w.bad = 0; w.sum_ranks = 0u; }
    team_sync();
    const T *Au = a.A + (size_t)u * a.lda;
    const int rsub = lane / LPR, piece = lane % LPR;
    const bool vec_ok = ((((size_t)a.B) | (a.ldb * sizeof(T))) & 15) == 0;
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
    const auto fetch = [&](const Ids &s, int k0, VT (&bv)[Q], T &av) {
        const int e0 = k0 + piece * VE;
        #pragma unroll
        for (int q = 0; q < Q; q++) {
            const int p = q * RPI + rsub;
            const T *brow = s.brow[q];
            VT x = {};
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
    CandStats<T> st;
    int wcount = 0;                                                  // (wavefront team: the append counter)
    Ids cur = ids_of(r0);
    VT bv[Q]; T av = 0;
    if (cur.live) fetch(cur, 0, bv, av);
    for (int base = r0; base < r1; base += TEAM) {
        const bool more = base + TEAM < r1;
        Ids nxt{};
        if (more) nxt = ids_of(base + TEAM);
        T s = 0;
        if (cur.live) {
            for (int k0 = 0; k0 < k; k0 += CH) {
                #pragma unroll
                for (int q = 0; q < Q; q++) *(VT *)&rows[wv][q * RPI + rsub][piece * VE] = bv[q];
                const T a_cur = av;
                if (k0 + CH < k) fetch(cur, k0 + CH, bv, av);
                else if (nxt.live) fetch(nxt, 0, bv, av);
                wave_sync();
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
                wave_sync();                                         // the image is rewritten by the next piece
            }
        } else if (nxt.live) fetch(nxt, 0, bv, av);
        if (TEAM == WAVE) {
            const unsigned long long act = __ballot(cur.mine);
            if (cur.mine) buf.set(wcount + __popcll(act & ((1ull << lane) - 1ull)), B::make(st.take(s), cur.item));
            wcount += __popcll(act);
        } else if (cur.mine) {
            const unsigned long long act = __builtin_amdgcn_ballot_w64(true);
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(act >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)act, 0u));
            int at0 = 0;
            if (rank == 0) at0 = atomicAdd(&w.count, __popcll(act));
            const int at = __builtin_amdgcn_readfirstlane(at0) + rank;
            if (at < CAPT) buf.set(at, B::make(st.take(s), cur.item));    // (never false: the row has at most CAPT entries)
        }
        cur = nxt;
    }
    team_sync();                                                     // (the image is dead from here on)
    const int C = TEAM == WAVE ? wcount : min(w.count, CAPT);
    if constexpr (TEAM == WAVE) wave_sort_desc<T>(buf, C, lane); else topk_sort_desc<T>(buf, C);
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) st.has_nan |= __shfl_xor(st.has_nan, d);
    if (lane == 0) w.wnan[wv] = st.has_nan;

    // ---- who is evaluated (k_classify with ntr = n - C, cold start considered) and whether the ranking is valid (k_finalize) ----
    const bool only_ndcg = npos >= C, kleqn = C <= K;
    bool skip = (only_ndcg && !(req & RQ_NDCG)) || C < a.min_items_pool || npos < a.min_pos_test;
    if (!skip && kleqn && !(req & (RQ_ROC | RQ_PR | RQ_AP | RQ_TAP | RQ_RR))) skip = true;
    const int W = K < C ? K : C;
    // the test row's ids (the region's first words), then every place's item looked up among them
    for (int i = tt; i < npos && i < CAPT; i += TEAM) tids[i] = a.test_i[te0 + i];
    team_sync();
    bool any_nan = false;
    for (int q = 0; q < TW; q++) any_nan |= w.wnan[q] != 0;
    {
        const bool ref_full = ((req & RQ_ROC) && !only_ndcg) || K >= C;
        const T hi = B::score(buf.get(0)), lo = B::score(buf.get(ref_full ? C - 1 : W - 1));
        skip |= any_nan || isinf(hi) || isinf(lo) || hi == lo || npos > C;
    }
    if (skip) { all_nan(); return; }                                 // (the same for every thread of the team)
    int hit_ix[STEPS], mine_hits = 0;
    #pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int p = (wv * STEPS + s) * WAVE + lane;
        int found = -1;
        if (p < C) {
            const int item = B::item(buf.get(p));
            int lo = 0, hi = npos;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (tids[mid] < item) lo = mid + 1; else hi = mid; }
            if (lo < npos && tids[lo] == item) found = lo;
        }
        hit_ix[s] = found;
        mine_hits += __popcll(__ballot(found >= 0));
    }
    if (lane == 0) w.wcnt[wv] = mine_hits;
    team_sync();
    int at = 0, nh = 0;
    for (int q = 0; q < TW; q++) { const int c = w.wcnt[q]; if (q < wv) at += c; nh += c; }
    if (nh != npos) { all_nan(); return; }                           // a test item that is no candidate of the user
    unsigned ranks = 0u; int top = 0;
    #pragma unroll
    for (int s = 0; s < STEPS; s++) {
        const int p = (wv * STEPS + s) * WAVE + lane;
        const bool h = hit_ix[s] >= 0;
        const unsigned long long hm = __ballot(h);
        if (h) { hitl[at + __popcll(hm & ((1ull << lane) - 1ull))] = (unsigned)p | ((unsigned)hit_ix[s] << 16); ranks += (unsigned)p + 1u; top += p < W; }
        at += __popcll(hm);
    }
    #pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { ranks += __shfl_xor(ranks, d); top += __shfl_xor(top, d); }
    if (lane == 0) { atomicAdd(&w.sum_ranks, ranks); atomicAdd(&w.nh_top, top); }
    team_sync();                                                     // (the ranking and the test ids have been read: `terms` and `run_ap` may be written)
    const int nh_top = w.nh_top;
    const bool want_dcg = (req & RQ_NDCG) != 0;

    // ---- AP / TAP / DCG / PR-AUC: the terms in parallel, the sums by one lane in the reference's order ----
    for (int j = tt; j < nh; j += TEAM) {
        const unsigned e = hitl[j];
        const int p = (int)(e & 0xffffu);
        terms[j] = (double)(j + 1) / (double)(p + 1);
        if (j < nh_top) run_dcg[j] = want_dcg ? (double)a.test_v[te0 + (int)(e >> 16)] / a.log2tab[p] : 0.;
    }
    team_sync();
    if (tt == 0) {
        double s = 0, d = 0;
        for (int j = 0; j < nh; j++) { s += terms[j]; if (j < nh_top) { run_ap[j] = s; d += run_dcg[j]; run_dcg[j] = d; } }
        w.ap_full = s; w.avg_p = nh_top ? run_ap[nh_top - 1] : 0.; w.dcg = d;
    }
    team_sync();

    // ---- the ideal DCG: the test values in descending order (the pairs' place again), the discounts added up by one lane ----
    const int L = K < npos ? K : npos;
    bool ndcg_nan = false, neg_tail = false;
    if (want_dcg) {
        bool vnan = false;
        for (int i = tt; i < npos; i += TEAM) { const T x = a.test_v[te0 + i]; vnan |= x != x; buf.set(i, B::make(x, i)); }
        if (lane == 0) w.wnan[wv] = 0;
        team_sync();
        if (__ballot(vnan) && lane == 0) w.wnan[wv] = 1;
        team_sync();
        for (int q = 0; q < TW; q++) ndcg_nan |= w.wnan[q] != 0;
        if (!ndcg_nan) {
            if constexpr (TEAM == WAVE) wave_sort_desc<T>(buf, npos, lane); else topk_sort_desc<T>(buf, npos);
            const T vmaxv = B::score(buf.get(0)), vlast = B::score(buf.get(L - 1));
            ndcg_nan = isinf(vmaxv) || isinf(vlast) || vmaxv <= 0;
            neg_tail = !(vlast >= 0);
            team_sync();                                             // (every thread has read the two before the sums take their place)
            if (!ndcg_nan && tt == 0) {
                double s = 0; bool stopped = false;
                for (int ix = 0; ix < L; ix++) {
                    const T x = B::score(buf.get(ix));
                    stopped |= neg_tail && x < 0;
                    if (!stopped) s += (double)x / a.log2tab[ix];
                    terms[ix] = s;
                }
                w.idcg = s;
            }
            team_sync();
        }
    }

    // ---- outputs ----
    const double avg_p = w.avg_p, dcg = w.dcg;
    const int first = nh_top ? (int)(hitl[0] & 0xffffu) : 0x7fffffff;
    const bool walked = (req & 0xff) && (!kleqn || (req & (RQ_AP | RQ_TAP | RQ_RR | RQ_NDCG)));
    T *const *o = a.out;
    if (!cum) {
        if (tt < 8 && o[tt]) {
            const int mn = K < npos ? K : npos;
            double v = 0;
            switch (tt) {
                case 0: v = (double)nh_top / (double)K; break;
                case 1: v = (double)nh_top / (double)mn; break;
                case 2: v = (double)nh_top / (double)npos; break;
                case 3: v = avg_p / (double)npos; break;
                case 4: v = avg_p / (double)mn; break;
                case 5: v = dcg / w.idcg; break;
                case 6: v = nh_top > 0; break;
                default: v = nh_top ? (1. / (double)(first + 1)) : 0.;
            }
            T x = (T)v;
            const bool count_metric = tt <= 2 || tt == 6;
            if (tt == 5) { if (ndcg_nan) x = qnan<T>(); }
            else if (kleqn ? count_metric : only_ndcg) x = qnan<T>();
            o[tt][u] = x;
        }
    } else {
        // the values of place ix < W as the walk leaves them
        const auto at_place = [&](int ix, double (&v)[8]) {
            int lo = 0, hi = nh_top;                                 // hits at or in front of ix
            while (lo < hi) { const int mid = (lo + hi) >> 1; if ((int)(hitl[mid] & 0xffffu) <= ix) lo = mid + 1; else hi = mid; }
            const int h = lo, mn = (ix + 1) < npos ? (ix + 1) : npos;
            const double ap = h ? run_ap[h - 1] : 0.;
            v[0] = h / (double)(ix + 1); v[1] = h / (double)mn; v[2] = h / (double)npos; v[3] = ap / (double)npos; v[4] = ap / (double)mn;
            v[5] = h ? run_dcg[h - 1] : 0.; v[6] = h > 0; v[7] = h ? ((double)1 / (double)(first + 1)) : 0.;
        };
        for (int ix = tt; ix < K; ix += TEAM) {
            double v[8];
            at_place(ix < C ? ix : C - 1, v);
            T x[8];
            #pragma unroll
            for (int q = 0; q < 8; q++) {
                const bool count_metric = q <= 2 || q == 6;
                x[q] = (T)v[q];
                if (ix >= C && count_metric) x[q] = qnan<T>();
                if (q != 5 && (kleqn ? (count_metric && !walked) : only_ndcg)) x[q] = qnan<T>();
            }
            if (o[5]) {
                if (ndcg_nan) x[5] = qnan<T>();
                else if (ix < L) x[5] = (T)((double)x[5] / terms[ix]);                              // quirk Q5: divides the rounded DCG
                else if (ix < C) { double t[8]; at_place(npos - 1, t); x[5] = (T)((double)(T)t[5] / terms[npos - 1]); }      // quirk Q6
            }
            #pragma unroll
            for (int q = 0; q < 8; q++) if (o[q]) o[q][(size_t)u * K + ix] = x[q];
        }
    }
    if (tt == 8 && o[8]) {
        const unsigned long long P = (unsigned long long)npos, Nneg = (unsigned long long)C - P, sum_ranks = w.sum_ranks;
        o[8][u] = only_ndcg ? qnan<T>() : (T)(1. - (double)(sum_ranks - (P * (P + 1)) / 2) / (double)(P * Nneg));
    }
    if (tt == 9 && o[9]) o[9][u] = only_ndcg ? qnan<T>() : (T)(w.ap_full / (double)npos);
}

// ---- every instantiation of this header's kernel template (rm_kernel_units.hpp) -----------------------------------------
#define RM_CANDMETRICS_KERNELS_F32(X) X(k_metrics_candidates<float, WAVE>) X(k_metrics_candidates<float, SCORE_ROW_THREADS>)
#define RM_CANDMETRICS_KERNELS_F64(X) X(k_metrics_candidates<double, WAVE>) X(k_metrics_candidates<double, SCORE_ROW_THREADS>)
RM_CANDMETRICS_KERNELS_F32(RM_EXTERN_KERNEL)
RM_CANDMETRICS_KERNELS_F64(RM_EXTERN_KERNEL)

} // namespace rm
