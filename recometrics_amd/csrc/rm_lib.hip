// rm_lib.hip -- host orchestration + the C-ABI of include/recometrics_hip.h and recometrics_hip_half.h  (gfx950 only).
//
// Host counterpart of reference src/recometrics.hpp:359-436 (prologue: clamps, scratch) and of the instantiation
// shims src/recometrics_instantiated.cpp:30-143.  The reference's OpenMP loop over users (:428-437) becomes:
//   plan (classify users, slots, groups)  ->  pack operands  ->  positives  ->  k_sweep  ->  k_finalize
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <type_traits>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <csignal>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/recometrics_hip.h"
#include "../../include/recometrics_hip_half.h"
#include "../../include/recometrics_hip_half_factors.h"
#include "rm_device.hpp"
#include "rm_prep.hpp"
#include "rm_launch.hpp"
#include "rm_finalize.hpp"
#include "rm_noise.hpp"
#include "rm_scores.hpp"
#include "rm_rowtopk.hpp"

namespace {

using namespace rm;

thread_local std::string g_err;
struct RmError { int code; std::string msg; };

#define HIP_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            throw RmError{e_ == hipErrorOutOfMemory ? RM_ERR_NOMEM : RM_ERR_HIP,                          \
                          std::string(#expr) + ": " + hipGetErrorString(e_)};                             \
    } while (0)

// ---- switches of tests and A/B timing ----------------------------------------------------------------------------------
// The environment is read ONCE, when the library is loaded (and again only when a test asks: rm_debug_reload_switches), never on
// the path of a call.  Every switch chooses among code paths that produce the same results (DESIGN.md section 7 lists them;
// tests/test_switches_cpu.py compares this table with that list); nothing here turns a feature of the call off.
struct Switches {
    bool no_train_bits, no_spec, no_side, ext_topk, no_test_mask, hbm_lists, nsub2, no_pending, no_pos_beside, no_seed, rank_generic,
         no_fused_auc, no_defer_auc, noise_sequential, one_context, noise_per_batch, host_trace, no_pos_flat, no_row_topk, no_split_cache, no_warm_bounds, ws_guard;
    long long free_mb, stream_budget_mb, noise_budget_mb, lane_cap_min, lane_min_k, lane_cap_set, sample_seed, split_cache_mb;      // -1 = not set
    unsigned long long epoch = 0;                                              // counts load(): what a context keeps of a split was decided under one set of switches
    double batch_users;                                                        // 0 = not set
    std::string splits;
    static bool on(const char *name) { return getenv(name) != nullptr; }
    static long long num(const char *name) { const char *e = getenv(name); return e ? atoll(e) : -1; }
    void load()
    {
        no_train_bits = on("RM_DEBUG_NO_TRAIN_BITS"); no_spec = on("RM_DEBUG_NO_SPEC"); no_side = on("RM_DEBUG_NO_SIDE");
        ext_topk = on("RM_DEBUG_EXT_TOPK"); no_test_mask = on("RM_DEBUG_NO_TEST_MASK");
        hbm_lists = on("RM_DEBUG_HBM_LISTS"); nsub2 = on("RM_DEBUG_NSUB2"); no_pending = on("RM_DEBUG_NO_PENDING");
        no_pos_beside = on("RM_DEBUG_NO_POS_BESIDE"); no_seed = on("RM_DEBUG_NO_SEED");
        rank_generic = on("RM_DEBUG_RANK_GENERIC"); no_fused_auc = on("RM_DEBUG_NO_FUSED_AUC");
        no_defer_auc = on("RM_DEBUG_NO_DEFER_AUC"); noise_sequential = on("RM_DEBUG_NOISE_SEQUENTIAL");
        one_context = on("RM_DEBUG_ONE_CONTEXT"); noise_per_batch = on("RM_DEBUG_NOISE_PER_BATCH"); host_trace = on("RM_HOST_TRACE");
        no_pos_flat = on("RM_DEBUG_NO_POS_FLAT");
        no_row_topk = on("RM_DEBUG_NO_ROW_TOPK");            // lists from a score matrix: stored rows + k_select_topk at every k_top (A/B timing, tests)
        free_mb = num("RM_DEBUG_FREE_MB"); stream_budget_mb = num("RM_STREAM_BUDGET_MB");
        noise_budget_mb = num("RM_NOISE_BUDGET_MB");
        lane_min_k = num("RM_DEBUG_LANE_MIN_K");                // the smallest k_metrics that takes the lane buffers instead of LDS / HBM lists (A/B timing)
        lane_cap_set = num("RM_DEBUG_LANE_CAP");                // entries per lane buffer (A/B timing; rounded to 16, never below what a selection needs)
        sample_seed = num("RM_DEBUG_SAMPLE_SEED");            // items of the sample that seeds the lane buffers' bounds: 0 = none, else forced to 64 / 256 / 1024 / 2048 / 4096 (A/B timing, tests)
        lane_cap_min = num("RM_DEBUG_LANE_CAP_MIN");          // the smallest lane buffers that work: a selection every few tiles (tests)
        no_split_cache = on("RM_DEBUG_NO_SPLIT_CACHE");        // every call plans, validates and builds its split's tables itself (A/B timing, the tests' reference path)
        split_cache_mb = num("RM_SPLIT_CACHE_MB");              // the largest split (bytes of its five arrays) a context keeps copies of; 0 = none
        no_warm_bounds = on("RM_DEBUG_NO_WARM_BOUNDS");        // a call on the kept split seeds its top-K bounds as a first call does: no k_hint_bounds (A/B timing, the tests' reference path)
        ws_guard = on("RM_DEBUG_WS_GUARD");                    // buffers allocated from now on lie between red zones, their payload poisoned (Workspace; tests)
        epoch++;
        const char *b = getenv("RM_BATCH_USERS"); batch_users = b ? atof(b) : 0.0;
        const char *s = getenv("RM_DEBUG_SPLITS"); splits = s ? s : "";
    }
    Switches() { load(); }
};
Switches g_sw;

// bytes the cached workspaces of ALL contexts hold (RM_DEBUG_FREE_MB: tests simulate a device with that much memory, so that
// the memory-bound regimes -- user batches sized by the score rows of k_metrics > 256 -- are reached with small inputs)
std::atomic<long long> g_ws_bytes{0};
inline long long debug_free_cap()
{
    return g_sw.free_mb >= 0 ? (g_sw.free_mb << 20) : -1;
}

// RM_HOST_TRACE: host-side time stamps from inside run() (the phases of one batch), picked up by the host entry's trace line
struct RunTrace {
    std::mutex mu; std::vector<std::pair<const char *, double>> pts; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void point(const char *what) { std::lock_guard<std::mutex> lk(mu); if (pts.size() > 4096) pts.clear(); pts.emplace_back(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count()); }
};
RunTrace g_run_trace;
#define RM_TRACE_POINT(what) do { if (g_sw.host_trace) g_run_trace.point(what); } while (0)

// ---- cached device workspace (per device), so that repeated calls do not pay hipMalloc ----
// Every ALLOCATION of a buffer carries a stamp from a process-wide counter: what is remembered about a buffer's contents (PackedItems,
// DenseRows, DiscountTable) is void once the buffer is allocated anew -- grown, or released and asked for again -- at whatever address.
std::atomic<unsigned long long> g_ws_stamp{1};
// EVERY buffer of a workspace: X(id, the name error messages print) -- what it holds, its shape, who writes it.  (T: the call's
// precision; GU: users per group; DESIGN.md section 1 "Data layout in HBM" describes the large ones.)
#define RM_WS_BUFFERS(X) \
    /* ---- the plan stage (Pipeline::plan_stage); a kept split (SplitCache) vouches for most of these ---- */ \
    X(WS_FLAGS, "flags")                        /* int[m]: the users' flags (k_classify) */ \
    X(WS_USER_NSLOTS, "user_nslots")            /* int[m]: sweep slots of each user (k_classify) */ \
    X(WS_USLOT_BASE, "uslot_base")              /* int[m]: exclusive scan of user_nslots, a user's place in slot_index (k_scan_exclusive) */ \
    X(WS_PLAN, "plan")                          /* Plan: the device Plan -- counts, class offsets, the CSR checks' verdicts, the maxima (zeroed by the plan stage; its kernels) */ \
    X(WS_HEAVY_USERS, "heavy_users")            /* int[m]: the users with more than `heavy_npos` test items, listed (k_classify) */ \
    X(WS_SLOT_USER, "slot_user")                /* int[m + nnz_test / POS_CHUNK + 1]: the user of each slot (k_assign_slots; debug_scores: k_iota) */ \
    X(WS_SLOT_CHUNK, "slot_chunk")              /* int[same]: the chunk of its user's test row each slot takes (k_assign_slots) */ \
    X(WS_SLOT_INDEX, "slot_index")              /* int[same]: at uslot_base[u] + c, the slot of user u's chunk c (k_assign_slots) */ \
    X(WS_SLOT_J, "slot_j")                      /* unsigned char[same]: table depth j of each slot (k_assign_slots, for k_block_tables) */ \
    X(WS_GJ, "gj")                              /* int[slots / GU + 2]: table depth of each group (k_block_tables) */ \
    X(WS_GROW, "grow")                          /* long long[slots / GU + 2]: group g owns the table rows from grow[g] + g (k_block_tables; debug_scores: zeros) */ \
    X(WS_SC_USER, "sc_user")                    /* int[slots]: the streamed users' chunk list, the user ... (k_assign_slots) */ \
    X(WS_SC_CHUNK, "sc_chunk")                  /* int[slots]: ... and the chunk (k_assign_slots) */ \
    X(WS_SCAN_TILE_TOTAL, "scan_tile_total")    /* int[ceil(m / 1024)]: m > 8,192: slots per tile of 1,024 users (k_scan_tiles) */ \
    X(WS_SCAN_TILE_OFFSET, "scan_tile_offset")  /* int[ceil(m / 1024)]: their exclusive scan (k_scan_exclusive) */ \
    X(WS_LOG2TAB, "log2tab")                    /* double[K]: log2(i + 2), the DCG discounts (uploaded by the plan stage; DiscountTable) */ \
    X(WS_ENT_USER, "ent_user")                  /* int[nnz_test]: the user of every test entry (k_entry_users) */ \
    X(WS_ENT_MASKED, "ent_masked")              /* unsigned char[nnz_test]: the entry's item is a train item (the dense train rows' kernel, or k_test_masked) */ \
    X(WS_POS_TMP, "pos_tmp")                    /* T[nnz_test]: score of each test entry, +inf when masked by the train row (k_pos_scores_flat / _given / k_pos_scores) */ \
    X(WS_POS_KEY, "pos_key")                    /* fp32: unsigned long long[nnz_test + 8]: the entry's packed key, score bits << 32 | ~item (the same kernels; PosArgs) */ \
    X(WS_HINT_COUNTS, "hint_counts")            /* int[2]: users k_hint_bounds gave a bound, users whose bound raised the positives' (zeroed by plan_reused; k_hint_bounds) */ \
    X(WS_TRAIN_BITS, "train_bits")              /* unsigned[m][dense_row_words(n)]: the dense train rows, a bit per item and user (launch_train_bits; DenseRows) */ \
    X(WS_HEAVY_TOPV, "heavy_topv")              /* T[m][heavy_ld]: largest test values, descending, of the users in heavy_users (k_top_values) */ \
    X(WS_HEAVY_NAN, "heavy_nan")                /* unsigned char[m]: ... and whether any of their values is NaN (k_top_values) */ \
    /* the context's copies of the kept split's five arrays, in SPLIT_ARRAYS order: 32-bit words as SplitKey::words counts them (keep_split) */ \
    X(WS_SPLIT_TRAIN_P, "split_train_p")        /* int[m + 1] */ \
    X(WS_SPLIT_TRAIN_I, "split_train_i")        /* int[nnz_train] */ \
    X(WS_SPLIT_TEST_P, "split_test_p")          /* int[m + 1] */ \
    X(WS_SPLIT_TEST_I, "split_test_i")          /* int[nnz_test] */ \
    X(WS_SPLIT_TEST_V, "split_test_v")          /* T[nnz_test], when the call has test values */ \
    /* ---- preparation, sweep, finalisation (Pipeline::prep, positives, select_lists) ---- */ \
    X(WS_MERGED, "merged")                      /* Entry<T>[m][K]: every user's final ordered top-K (the finalisation); the next pass's advice on a kept split (SplitCache::lists) */ \
    X(WS_RANK_SORTED, "rank_sorted")            /* long long[nnz_test]: 1-based full-ranking position per sorted positive, 0 = masked (zeroed by prep; the finalisation's rank kernels) */ \
    X(WS_AUC_PART, "auc_part")                  /* AucPart[n_slots]: a slot's sums for the two AUC values (k_auc_slots, the streamed users' rank kernels) */ \
    X(WS_STREAM_SCORES, "stream_scores")        /* T[n_stream][stream_ld]: masked candidate scores of the streamed users (the sweep; k_score_rows) */ \
    X(WS_PST, "pst")                            /* PartialStat<T>[n_slots][n_part]: the candidates' statistics in parts (the sweep; k_score_rows) */ \
    X(WS_BP, "Bp")                              /* 16 B x items_units: the packed item image (pack_operands; PackedItems) */ \
    X(WS_AP, "Ap")                              /* 16 B x users_units: the packed user image, per user group (pack_operands) */ \
    X(WS_PL, "pl")                              /* Entry<T>[n_slots][n_part][K]: the top-K lists in parts (the sweep) */ \
    X(WS_GLISTS, "glists")                      /* per sweep block and wave: [lane_cap][64 lanes] lane buffers of (sizeof(T) + 4)-byte entries, or ListT[GU][2K + 32] replace-the-minimum lists in HBM (the sweep) */ \
    X(WS_LANE_CNT, "lane_cnt")                  /* int[block][wave][64]: entries each lane left in its buffer (the sweep) */ \
    X(WS_THR_SHARED, "thr_shared")              /* ThrT[n_slots]: order-preserving key of the user's bound (k_seed_thresholds or zeroed; raised by k_seed_from_sample, k_hint_bounds, the sweep) */ \
    X(WS_SAMPLE_SCORES, "sample_scores")        /* T[n_slots][S]: every slot's scores of the first S items (the sweep's DUMP variant, seed_from_sample) */ \
    X(WS_SAMPLE_ITEMS, "sample_items")          /* 16 B x items_units: an image of the sample in 64-item tiles, for a sweep with three sub-tiles (pack_operands) */ \
    X(WS_SAMPLE_LISTS, "sample_lists")          /* ListT[n_ublocks][8][GU][2 + 32]: the lists of that DUMP sweep, K = 1 (seed_from_sample hands them to it) */ \
    X(WS_POS_SCORE, "pos_score")                /* T[total_rows + n_groups + 1][GU]: the positives' tables, 2^j rows per group, last row +inf (k_init_tables, k_pos_place) */ \
    X(WS_POS_ITEM, "pos_item")                  /* int[same]: item id of each sorted positive (k_pos_place) */ \
    X(WS_HIST, "hist")                          /* unsigned[same]: candidates ranking between two positives (k_init_tables; the sweep) */ \
    X(WS_POS_ORDER, "pos_order")                /* int[nnz_test]: ascending rank of the entry inside its row (k_pos_place) */ \
    X(WS_SPOS_SCORE, "spos_score")              /* T[nnz_test]: streamed users, at test_p[u] + rank: scores ascending (k_init_tables, k_pos_place) */ \
    X(WS_SPOS_ITEM, "spos_item")                /* int[nnz_test]: ... their item ids (k_pos_place) */ \
    X(WS_SHIST, "shist")                        /* unsigned[nnz_test]: ... candidates above positive j but not above j + 1 (k_init_tables; k_rank_streamed) */ \
    X(WS_SEL_HI, "sel_hi")                      /* unsigned long long[n_slots][sel_ld]: k_select_topk's scratch, sel_ld = K rounded up to a power of two */ \
    X(WS_SEL_LO, "sel_lo")                      /* unsigned[n_slots][sel_ld]: ... the same */ \
    /* ---- the tie noise (ExactPass, run_call) ---- */ \
    X(WS_NOISE_ROW, "noise_row")                /* int[m]: the noise row of each flagged user (k_noise_assign_rows) */ \
    X(WS_NOISE_ROW_USER, "noise_row_user")      /* int[flagged users, or m]: the user of each row (k_noise_assign_rows) */ \
    X(WS_NOISE_COUNTER, "noise_counter")        /* int: rows given out (zeroed by assign; k_noise_assign_rows) */ \
    X(WS_NOISE_ONLY, "noise_only")              /* unsigned char[m]: the users of the rows of one step (k_noise_select) */ \
    X(WS_O_EXACT, "o_exact")                    /* T[block_size(m)]: metric block of an exact pass, [metric][users x width] (that pass's finalisation) */ \
    X(WS_NOISE_DRAWS, "noise_draws")            /* unsigned[rows][d_ld]: mt19937(seed + user) draws (k_mt_draws) */ \
    X(WS_NOISE_ROWS, "noise_rows")              /* T[rows][e_ld]: the per-item noise rows (k_noise_rows / k_noise_rows_bits) */ \
    X(WS_NOISE_FLAG, "noise_flag")              /* int[m]: users the first pass flags (zeroed by run_call; the positives' scores, k_finalize) */ \
    X(WS_NOISE_FLAG_SNAP, "noise_flag_snap")    /* int[m]: the flags when that pass launches its sweep (Pipeline::sweep, a copy) */ \
    /* ---- the host-pointer entry (HostRange): uploads, outputs on the device ---- */ \
    X(WS_IN_B, "in_B")                          /* T (or 16-bit: Request::f_type) [n][k]: the item factors, dense rows (HostRange's uploads; debug_scores) */ \
    X(WS_IN_A, "in_A")                          /* T (or 16-bit) [m][k]: the range's user factors (HostRange's uploads; debug_scores) */ \
    X(WS_IN_TRP, "in_trp")                      /* int[m + 1]: train index pointers, rebased to the range (stage_inputs) */ \
    X(WS_IN_TEP, "in_tep")                      /* int[m + 1]: test index pointers, rebased (stage_inputs) */ \
    X(WS_IN_TRI, "in_tri")                      /* int[nnz_train of the range] (HostRange's uploads) */ \
    X(WS_IN_TEI, "in_tei")                      /* int[nnz_test of the range] (HostRange's uploads) */ \
    X(WS_IN_TEV, "in_tev")                      /* T[nnz_test of the range] (HostRange's uploads) */ \
    X(WS_O_TOPK_IDX, "o_topk_idx")              /* int[m][K]: the ranking outputs of rm_rank_* and of the lists, for copy_out (the batches' passes, through Call::topk_idx ...) */ \
    X(WS_O_TOPK_SCORE, "o_topk_score")          /* T[m][K] */ \
    X(WS_O_POS_RANK, "o_pos_rank")              /* long long[nnz_test of the range] */ \
    X(WS_O_STATUS, "o_status")                  /* int[m] */ \
    X(WS_O_BLOCK, "o_block")                    /* T[block_size(largest batch)]: the metric block of a batch, [metric][users x width] (the finalisation) */ \
    X(WS_IN_S0, "in_S0")                        /* T (or 16-bit: ScoreType) [largest batch][n]: the caller's score rows of a batch ... (HostRange's uploads) */ \
    X(WS_IN_S1, "in_S1")                        /* ... and of the next one, which travels meanwhile */ \
    X(WS_NOISE_FLAG_RANGE, "noise_flag_range")  /* int[m]: fp32 tie noise over several batches: the flags of the range (zeroed by plan_batches; the batches' first passes) */ \
    X(WS_NOISE_FLAG_RANGE_SNAP, "noise_flag_range_snap")  /* int[m]: ... when the LAST batch launches its sweep */ \
    X(WS_O_EXACT_PACKED, "o_exact_packed")      /* T[count][rec_w]: an exact pass's results, a record per evaluated user (k_noise_gather) */ \
    /* ---- the device-pointer entry (run_dev), debug_scores ---- */ \
    X(WS_RECO_ZERO_P, "reco_zero_p")            /* int[m + 1]: zeros, the index pointers of lists without an exclusion matrix (run_dev) */ \
    X(WS_SORTED_TRI, "sorted_tri")              /* int[nnz_train]: the caller's unsorted CSR rows, sorted by the host (run_dev) */ \
    X(WS_SORTED_TEI, "sorted_tei")              /* int[nnz_test] */ \
    X(WS_SORTED_TEV, "sorted_tev")              /* T[nnz_test] */ \
    X(WS_DBG_ZEROS, "dbg_zeros")                /* int[m + 1 + n_groups]: zeros for slot_chunk, train_p, train_i and gj (debug_scores) */ \
    X(WS_DBG_DUMP, "dbg_dump")                  /* T[m][n]: every score (the sweep's DUMP variant, debug_scores) */
#define RM_WS_ID(id, name) id,
#define RM_WS_NAME(id, name) name,
enum WsBuf { RM_WS_BUFFERS(RM_WS_ID) WS_COUNT };
constexpr const char *WS_NAMES[WS_COUNT] = { RM_WS_BUFFERS(RM_WS_NAME) };
#undef RM_WS_ID
#undef RM_WS_NAME
// RM_DEBUG_WS_GUARD (tests): a buffer allocated while the switch is set lies between two red zones, and its payload is poisoned:
//     [ head zone, WS_ZONE bytes ][ payload: the bytes asked for ][ tail zone: the slack of an ordinary allocation + WS_ZONE bytes ]
// The tail zone starts at the byte count the request states, so a store one element past it is seen; whatever lies inside an ordinary
// allocation -- `cap` bytes from the pointer handed out -- lies inside a guarded one too (an over-read stays as harmless as it was).
// The allocation policy is the ordinary one: a later request that fits the buffer gets it as it is.  Where that request is LARGER than
// every one before (the batches of a host call, the next call at a few more slots: it fits the slack), the payload grows into the tail
// zone: the part taken over is checked first, then poisoned (guard_grow) -- the stores of that request's kernels are no damage.
// The zones repeat WS_RED, the payload the word of its request: WS_POISON_FLOAT behind ws.array<float / double> (a quiet NaN as a
// float and, in pairs, as a double; not the library's own 0xFFFFFFFF), WS_POISON_INT behind everything else -- small on purpose: a
// counter or flag nobody zeroed is visibly wrong, an index nobody wrote stays in range or one element behind it, inside the zone.
// Every byte of an allocation is byte (offset & 3) of its region's word, offsets counted from the 256-byte-aligned allocation.
// rm_debug_ws_check compares the zones with WS_RED, rm_debug_ws_poke damages one byte of one (both at the end of this file).
constexpr size_t WS_ZONE = 256, WS_CHECK_MAX = size_t(1) << 20;
constexpr unsigned WS_RED = 0xC3A55A3Cu, WS_POISON_FLOAT = 0x7FF87FF8u, WS_POISON_INT = 0x00000001u;
inline unsigned char ws_pattern_byte(unsigned word, size_t offset) { return (unsigned char)(word >> (8 * (offset & 3))); }
// the words [w0, w1) of a guarded allocation: `poison` where a byte lies in [lo, hi) (offsets in the allocation); every other byte of
// those words becomes WS_RED (`fresh`: the allocation's first fill) or stays what it is (a payload that grows into its tail zone)
__global__ void k_ws_guard_fill(unsigned *base, size_t w0, size_t w1, size_t lo, size_t hi, unsigned poison, bool fresh)
{
    for (size_t w = w0 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < w1; w += (size_t)gridDim.x * blockDim.x) {
        const size_t o = 4 * w;
        unsigned v = fresh ? WS_RED : base[w];
        for (int b = 0; b < 4; b++)
            if (o + b >= lo && o + b < hi) v = (v & ~(0xFFu << (8 * b))) | (poison & (0xFFu << (8 * b)));
        base[w] = v;
    }
}
struct Workspace {
    // `bytes`: what the buffer serves without a new allocation (the request that allocated it and its slack); `real`: what hipMalloc
    // gave -- the same, or in guard mode the zones too --; `req`: the byte count of the largest request the allocation has served,
    // where a guarded buffer's tail zone starts; `lost_*`: damage found in the part of the tail zone a larger request took over
    struct Buf {
        void *ptr = nullptr; size_t bytes = 0; unsigned long long stamp = 0; size_t real = 0, req = 0; bool guard = false;
        long long lost_first = -1, lost_last = -1; size_t lost_req = 0;
        void *base() const { return guard ? (char *)ptr - WS_ZONE : ptr; }
        size_t tail_bytes() const { return guard ? real - WS_ZONE - req : 0; }
    };
    Buf bufs[WS_COUNT];
    static void drop(Buf &b) { if (b.ptr) { (void)hipFree(b.base()); g_ws_bytes -= (long long)b.real; } b = Buf{}; }
    // poisons the bytes [lo, hi) of a guarded allocation and waits for the whole device (the streams beside the call's may be the next
    // to touch the buffer)
    static void guard_fill(WsBuf id, Buf &b, size_t lo, size_t hi, unsigned poison, bool fresh)
    {
        const size_t w0 = fresh ? 0 : lo / 4, w1 = fresh ? b.real / 4 : (hi + 3) / 4;
        hipError_t e = hipSuccess;
        if (w1 > w0) {
            hipLaunchKernelGGL(k_ws_guard_fill, dim3((unsigned)std::min<size_t>((w1 - w0 + 255) / 256, 4096)), dim3(256), 0, nullptr,
                               (unsigned *)b.base(), w0, w1, lo, hi, poison, fresh);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) { drop(b); throw RmError{RM_ERR_HIP, std::string("RM_DEBUG_WS_GUARD: filling ") + WS_NAMES[id] + ": " + hipGetErrorString(e)}; }
    }
    // A guarded buffer serves a request larger than any before, inside its slack: the payload grows into the tail zone.  What it takes
    // over is compared with WS_RED first (damage there is kept for rm_debug_ws_check: `lost_*`, the first such find) and then poisoned.
    static void guard_grow(WsBuf id, Buf &b, size_t req, unsigned poison)
    {
        HIP_CHECK(hipDeviceSynchronize());
        const size_t at = WS_ZONE + b.req, len = std::min(req - b.req, WS_CHECK_MAX);
        std::vector<unsigned char> host(len);
        HIP_CHECK(hipMemcpy(host.data(), (const char *)b.base() + at, len, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < len && b.lost_first < 0; i++)
            if (host[i] != ws_pattern_byte(WS_RED, at + i)) {
                b.lost_first = b.lost_last = (long long)i; b.lost_req = b.req;
                for (size_t j = len; j-- > i;) if (host[j] != ws_pattern_byte(WS_RED, at + j)) { b.lost_last = (long long)j; break; }
            }
        guard_fill(id, b, at, WS_ZONE + req, poison, false);
        b.req = req;
    }
    void *get(WsBuf id, size_t bytes, unsigned poison = WS_POISON_INT)
    {
        const size_t req = bytes;
        bytes = std::max<size_t>(bytes, 256);
        Buf &b = bufs[id];
        if (b.bytes < bytes) {
            drop(b);
            const size_t cap = bytes + bytes / 8;
            const bool guard = g_sw.ws_guard;
            const size_t real = guard ? WS_ZONE + (cap + 3) / 4 * 4 + WS_ZONE : cap;
            const long long sim = debug_free_cap();
            if (sim >= 0 && g_ws_bytes.load() + (long long)real > sim)
                throw RmError{RM_ERR_NOMEM, std::string("hipMalloc(") + WS_NAMES[id] + ", " + std::to_string(real) + " B): beyond RM_DEBUG_FREE_MB"};
            void *p = nullptr;
            hipError_t e = hipMalloc(&p, real);
            if (e != hipSuccess) throw RmError{RM_ERR_NOMEM, std::string("hipMalloc(") + WS_NAMES[id] + ", " + std::to_string(real) + " B): " + hipGetErrorString(e)};
            g_ws_bytes += (long long)real;
            b.ptr = guard ? (char *)p + WS_ZONE : p; b.bytes = cap; b.real = real; b.req = req; b.guard = guard; b.stamp = g_ws_stamp.fetch_add(1);
            if (guard) guard_fill(id, b, WS_ZONE, WS_ZONE + req, poison, true);
        } else if (b.guard && b.req < req) guard_grow(id, b, req, poison);
        return b.ptr;
    }
    template <class T> T *array(WsBuf id, size_t count) { return (T *)get(id, sizeof(T) * count, std::is_floating_point<T>::value ? WS_POISON_FLOAT : WS_POISON_INT); }
    // the buffer as it stands (never asked for, or released: null and stamp 0, which no valid record carries)
    const Buf &peek(WsBuf id) const { return bufs[id]; }
    void release() { for (Buf &b : bufs) drop(b); }      // (every slot: no stamp outlives its memory)
};
// What a workspace buffer was last filled with, for the callers that may find it filled already.  A record is valid only for the
// allocation it was made in (Workspace::Buf::stamp): `Filled<ID>` is that half of every record, bound to its buffer; each question a
// caller asks is a member of the record.
template <WsBuf ID> struct Filled {
    unsigned long long stamp = 0;                                // of the allocation the record was made in; 0 = no record
    bool current(const Workspace &ws) const { return stamp != 0 && stamp == ws.peek(ID).stamp; }
    void bind(const Workspace &ws) { stamp = ws.peek(ID).stamp; }
    void unbind() { stamp = 0; }
    const void *ptr(const Workspace &ws) const { return ws.peek(ID).ptr; }
};
struct PackedItems : Filled<WS_BP> {         // the packed item image, shared by the passes / batches of one call (Call::items_tag)
    unsigned long long tag = 0; int tile = 0, ng = 0;
    unsigned long long amax_b = 0; int nonfinite_b = 0;      // max |B| and its non-finite count as that call's plan found them
    bool of_call(unsigned long long t) const { return t != 0 && t == tag; }      // (the bound on |B| holds for the call; `holds`: so does the image, at this geometry)
    bool holds(const Workspace &ws, unsigned long long t, int tile_items, int NG) const { return of_call(t) && current(ws) && tile == tile_items && ng == NG; }      // (a tag comes with a stamp: set)
    void set(const Workspace &ws, unsigned long long t, int tile_items, int NG) { bind(ws); tag = t; tile = tile_items; ng = NG; }
    void invalidate() { unbind(); tag = 0; }
};
struct DenseRows : Filled<WS_TRAIN_BITS> {   // the dense train rows (set_train_bits)
    long long words = 0; int m = 0;
    bool masked = false, partial = false;                      // the test items marked too; a subset of the users only (Call::only_users)
    unsigned long long tag = 0; const int *train_p = nullptr;  // built by which call (Call::items_tag), over which rows
    // rows of this buffer for `m_` users, `words_` words, masked as asked, built for all users (a later pass of the same call)
    bool fits(const Workspace &ws, int m_, long long words_, bool masked_) const { return current(ws) && !partial && words == words_ && m == m_ && masked == masked_; }
    // rows built by call `t` over `train_p_` for `m_` users, not partial (the tie noise's exact pass beside that call's sweep)
    bool built_by(const Workspace &ws, unsigned long long t, const int *train_p_, int m_) const { return current(ws) && t != 0 && t == tag && train_p == train_p_ && m == m_ && !partial; }
    const unsigned *rows(const Workspace &ws) const { return (const unsigned *)ptr(ws); }
    void set(const Workspace &ws, long long words_, int m_, bool masked_, bool partial_, unsigned long long t, const int *train_p_)
    { bind(ws); words = words_; m = m_; masked = masked_; partial = partial_; tag = t; train_p = train_p_; }
    void invalidate() { unbind(); tag = 0; }
};
struct DiscountTable : Filled<WS_LOG2TAB> {  // log2(i + 2), the DCG discounts
    int K = 0;
    bool holds(const Workspace &ws, int K_) const { return current(ws) && K >= K_; }
    void set(const Workspace &ws, int K_) { bind(ws); K = K_; }
};
// What a context keeps of the train / test split of its last metric call, for the next call on the same split (one model after
// another on one split: a hyper-parameter search, an evaluation per epoch): copies of the five arrays, in buffers of their own, and
// the fact that everything the plan stage derives from them is still in the workspace -- the users' flags, the slot / group / block
// tables, the device Plan, the user of every test entry and whether it is a train item, the dense train rows (DenseRows), the
// ideal-DCG values of the long rows.  No later stage of a call writes any of these (k_finalize reads them), every other pass through
// run() on the context voids the record before it plans, and so does a new allocation of any of the buffers (stamps).
// `key`: the arrays' addresses and sizes and every decision of the plan stage that does not come from the arrays' contents; whether
// the CONTENTS are still the ones copied is k_split_same's answer, call by call.
constexpr long long SPLIT_CACHE_DEFAULT_MB = 1024;      // RM_SPLIT_CACHE_MB when it is not set
struct SplitKey {
    const void *arr[SPLIT_ARRAYS]; long long words[SPLIT_ARRAYS], nnz_train, nnz_test;
    int m, n, k, K, elem, req, min_items_pool, min_pos_test, heavy_npos, ng;
    int cold, cumulative, want_lane, ext_topk, allow_stream, force_stream, dense_ok, flat_early, csr_checked, rank_out;
    unsigned long long switches;                                // Switches::epoch
};
struct SplitCache {
    static constexpr WsBuf copies[SPLIT_ARRAYS] = {WS_SPLIT_TRAIN_P, WS_SPLIT_TRAIN_I, WS_SPLIT_TEST_P, WS_SPLIT_TEST_I, WS_SPLIT_TEST_V};
    bool valid = false; SplitKey key{}; Plan hp{}; bool check_nan = false, dense_masked = false;
    std::vector<std::pair<WsBuf, unsigned long long>> stamps;             // the buffers the record speaks of, as allocated then
    // WS_MERGED as allocated when the last plain pass on this split enqueued its k_finalize: the buffer then holds that pass's ordered
    // top-K lists, the advice of the next pass (k_hint_bounds).  Taken (and so voided) when a pass starts, set again when it has
    // enqueued everything: a pass that fails or is interrupted leaves none.
    Filled<WS_MERGED> lists;
    // Whether that advice is worth its kernel is the model's business, not the split's: a pass whose bounds mostly stayed BELOW what the
    // positives gave anyway (fewer than half of them raised a word: the model has little to do with the last one) makes the next
    // `hint_skip` passes run without the kernel -- 1, then 2, 4, ... up to HINT_BACKOFF_MAX for every further such pass, back to none
    // after a pass whose bounds did raise.  `hint_judge`: the last pass launched the kernel and its counts have not been looked at yet.
    static constexpr int HINT_BACKOFF_MAX = 16;
    int hint_skip = 0, hint_backoff = 0; bool hint_judge = false;
    void invalidate() { valid = false; lists.unbind(); hint_skip = hint_backoff = 0; hint_judge = false; }
    // the counts of the last launch (accepted, raised), then: does this pass launch?
    bool hints_due(const int *counts)
    {
        if (hint_judge) {
            hint_judge = false;
            if (2LL * counts[1] < counts[0]) { hint_backoff = hint_backoff ? std::min(2 * hint_backoff, HINT_BACKOFF_MAX) : 1; hint_skip = hint_backoff; }
            else hint_backoff = 0;
        }
        if (hint_skip > 0) { hint_skip--; return false; }
        return true;
    }
    bool take_lists(const Workspace &ws) { const bool kept = lists.current(ws); lists.unbind(); return kept; }
    void keep_lists(const Workspace &ws) { lists.bind(ws); }
    void keep(const Workspace &ws, WsBuf id) { stamps.emplace_back(id, ws.peek(id).stamp); }
    bool holds(const Workspace &ws, const SplitKey &k) const
    {
        if (!valid || std::memcmp(&key, &k, sizeof(SplitKey)) != 0) return false;
        for (const auto &s : stamps) if (s.second == 0 || ws.peek(s.first).stamp != s.second) return false;
        return true;
    }
    const void *copy(const Workspace &ws, int i) const { return ws.peek(copies[i]).ptr; }
};
// The roles of the events that order a context's two streams beside the call's against it: who records each and who waits is the
// table in DESIGN.md section 1.  One event per role; `Beside` (below) is the only code that touches them.
enum SideMark { SIDE_FORK, SIDE_JOIN, SIDE_PLAN_FORK, SIDE_CHECKS_DONE, SIDE_ROWS_AND_PACKS, SIDE_ROWS_FOR_POS, SIDE_TOP_VALUES,
                SIDE_SWEEP_FORK, SIDE_SWEEP_DEEP_DONE, SIDE_MERGED, SIDE_VERDICT, SIDE_SPLIT_KEPT, SIDE_MARKS };
enum PosMark { POS_PLAN_FORK, POS_MAXIMA_DONE, POS_SCORES_AFTER_COPY, POS_SCORES_DONE, POS_TABLES_INIT, POS_STREAMED_PLACED, POS_MARKS };
enum PassEvent { EV_START, EV_PREP_END /* = sweep launched: HostRange::exact_beside_last waits for it */, EV_SWEEP_END, EV_END, EV_COUNT };   // timing (Ctx::stage_ms)
// The page-locked words of a context through which the counts of the fp32 tie noise come back from the device (one 64-byte
// allocation per context, Ctx::need_noise_words)
struct NoiseWords {
    int first_early;         // users flagged when a first pass launches its sweep (Call::flag_count_host; for the last batch of a host
                             // call it is the word of the RANGE's context, also when that batch runs on the peer context)
    int first_final;         // ... and after that pass's k_finalize (run_call)
    int sequential;          // flagged users as a sequential exact pass counts them (ExactPass::sequential)
    int range_early;         // host entry: flagged users of the range as the pass beside the last batch counts them
    int batch_flagged;       // host entry: users the first pass of a batch on this context flagged
};
static_assert(sizeof(NoiseWords) <= 64, "the noise words share one 64-byte page-locked allocation");
// One context per (device, shard slot): the cached workspace plus the events / side stream that belong to that device.
// Slot 0 serves ordinary calls; a call sharded inside the library (rm_set_devices) uses slot i for the i-th entry of the device
// list, so that the same physical device can appear more than once ("virtual shards").  A context is used by ONE call at a
// time (`mu` is held while that call enqueues its work), and a call whose stream differs from the previous call's waits for
// that call's `done` event before it touches any workspace buffer: calls on different streams or threads serialise on the
// device instead of corrupting each other's buffers.
struct Ctx {
    int device = 0, slot = 0;
    std::mutex mu;
    Workspace ws;
    hipEvent_t ev[EV_COUNT] = {nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false, ev_recorded = false;
    hipStream_t side_stream = nullptr; std::array<hipEvent_t, SIDE_MARKS> side_marks{};     // the two streams beside a call's (Beside), one event per role
    hipStream_t pos_stream = nullptr; std::array<hipEvent_t, POS_MARKS> pos_marks{};
    hipEvent_t done = nullptr;               // end of the device work of the most recent call on this context
    hipStream_t own_stream = nullptr;        // stream of a shard worker (multi-device calls)
    hipStream_t up_stream = nullptr;         // host-pointer calls: uploads of the NEXT user batch run beside the current batch's kernels
    hipEvent_t up_ev[2] = {nullptr, nullptr};
    NoiseWords *noise_words = nullptr; hipEvent_t flags_ev = nullptr, pass_ev = nullptr;   // tie noise: flag counts read back, flags ready, exact pass done
    void need_noise_words()                    // (the words and the two events are created together, once per context)
    {
        if (noise_words) return;
        HIP_CHECK(hipHostMalloc((void **)&noise_words, 64, hipHostMallocDefault));
        HIP_CHECK(hipEventCreateWithFlags(&flags_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&pass_ev, hipEventDisableTiming));
    }
    void *pinned = nullptr; size_t pinned_bytes = 0;   // page-locked staging for the metric block of a batch (one D2H copy instead of ten)
    void *pinned_get(size_t bytes)
    {
        if (pinned_bytes < bytes) {
            if (pinned) { (void)hipHostFree(pinned); pinned = nullptr; pinned_bytes = 0; }
            if (hipHostMalloc(&pinned, bytes + bytes / 8, hipHostMallocDefault) != hipSuccess) { pinned = nullptr; throw RmError{RM_ERR_NOMEM, "hipHostMalloc of the output staging buffer failed"}; }
            pinned_bytes = bytes + bytes / 8;
        }
        return pinned;
    }
    // rm_get_timings' out[]: the four stage times, then the launch the "sweep" timing brackets (launches, item splits, blocks, LDS bytes)
    enum { TM_LAUNCHES = 4, TM_SPLITS, TM_BLOCKS, TM_LDS, TM_TIMED_SLOTS, TM_TOTAL_SLOTS, TM_SPLIT_REUSED, TM_HINTED, TM_COUNT };
    double timings[TM_TIMED_SLOTS] = {0, 0, 0, 0, 0, 0, 0, 0};
    int timed_slots = 0, total_slots = 0;     // slots (user lanes) of the sweep launch the "sweep" timing brackets / of the call
    void sweep_shape(double launches, double splits, double blocks, double lds, int slots)      // (slots < 0: nothing was launched, they stay)
    {
        timings[TM_LAUNCHES] = launches; timings[TM_SPLITS] = splits; timings[TM_BLOCKS] = blocks; timings[TM_LDS] = lds;
        if (slots >= 0) timed_slots = total_slots = slots;
    }
    double acc[4] = {0, 0, 0, 0};            // prep / sweep / finalize / total ms of the batches already read back (host entry)
    PackedItems packed; DenseRows dense; DiscountTable discounts;    // what WS_BP, WS_TRAIN_BITS and WS_LOG2TAB of `ws` hold
    SplitCache split;                                                // ... and what the plan stage's buffers hold of the last call's split
    int split_reused = -1;               // the most recent pass: 1 = it ran on what `split` kept, 0 = it planned itself, -1 = a pass that never reuses
    // the warm bounds of the most recent pass that launched k_hint_bounds: page-locked, the users that got a bound and those whose bound
    // raised the positives' (copied behind the sweep's launch; read behind a later host wait: rm_get_timings, the next pass's verdict)
    int *hint_counts = nullptr; bool hints_ran = false;
    bool high_priority = false;          // streams of this context are created with the highest priority (the exact passes of the tie noise)
    Plan *pinned_plan = nullptr;                                                    // page-locked landing place of the plan read-back
    void stage_ms(float ms[4]) const       // prep / sweep / finalize / total of the most recent pass, from its four events (which have completed)
    {
        const int from[4] = {EV_START, EV_PREP_END, EV_SWEEP_END, EV_START}, to[4] = {EV_PREP_END, EV_SWEEP_END, EV_END, EV_END};
        for (int i = 0; i < 4; i++) (void)hipEventElapsedTime(&ms[i], ev[from[i]], ev[to[i]]);
    }
};
// A stream of a context.  The NOISE_SLOT contexts ask for the highest priority the device offers: their work -- the exact pass of the
// tie noise over a few thousand users -- is enqueued BESIDE a sweep that fills every compute unit, and at normal priority its kernels
// are only served when that sweep has no more blocks to place (measured: the pass started when the sweep ended); at high priority its
// workgroups go first whenever a compute unit frees up.
inline hipError_t create_stream(hipStream_t *st, bool high_priority)
{
    if (high_priority) {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            return hipStreamCreateWithPriority(st, hipStreamNonBlocking, greatest);
        (void)hipGetLastError();
    }
    return hipStreamCreateWithFlags(st, hipStreamNonBlocking);
}
std::mutex g_ctx_mu;
std::map<std::pair<int, int>, std::unique_ptr<Ctx>> g_ctx;
thread_local Ctx *g_last_ctx = nullptr;      // context of the most recent call on this thread (rm_get_timings)

Ctx &context(int slot)
{
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto &p = g_ctx[std::make_pair(dev, slot)];
    if (!p) { p.reset(new Ctx()); p->device = dev; p->slot = slot; }
    return *p;
}
// the second context of a host-pointer call: its odd batches run there (own workspace, events, stream), so that a batch's
// prep -- two dozen short launches and a plan read-back -- overlaps the sweep of the batch before it
// (a third kind of context, NOISE_SLOT apart from its owner: the exact pass of the tie noise beside a first sweep -- also of a
// batch that itself runs on a peer context)
constexpr int PEER_SLOT = 1 << 12, NOISE_SLOT = 1 << 13;
Ctx &peer_context(const Ctx &cx, int offset = PEER_SLOT)
{
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    auto &p = g_ctx[std::make_pair(cx.device, cx.slot + offset)];
    if (!p) { p.reset(new Ctx()); p->device = cx.device; p->slot = cx.slot + offset; p->high_priority = offset == NOISE_SLOT; }
    return *p;
}

// The outputs of a request, as one value (a call that writes somewhere else assigns another one).  In a host request they are the
// caller's HOST arrays.
template <class T> struct Outputs {
    T *out[10] = {};                           // p, tp, r, ap, tap, ndcg, hit, rr, roc, pr
    // optional ranking outputs
    int *topk_idx = nullptr; T *topk_score = nullptr; long long *pos_rank = nullptr; int *status = nullptr;
    // the same arrays from user `u` on: `per` values per user of the eight top-K metrics, K per list (`pos_rank` is indexed by test
    // entry: the index pointers of those users carry the offset)
    Outputs from_user(size_t u, size_t per, int K) const
    {
        Outputs o = *this;
        for (int i = 0; i < 10; i++) if (out[i]) o.out[i] = out[i] + u * (i >= 8 ? 1 : per);
        if (topk_idx) o.topk_idx = topk_idx + u * (size_t)K;
        if (topk_score) o.topk_score = topk_score + u * (size_t)K;
        if (status) o.status = status + u;
        return o;
    }
};
// What a caller asked for: one metric or list call as the C-ABI states it.  Its pointers are HOST pointers in a host entry (HostRange
// stages the arrays batch by batch) and DEVICE pointers in a device entry and in every Call.
// The element type of a caller's score matrix: the call's own T, or 16-bit patterns (include/recometrics_hip_half.h; T is float then),
// which the three kernels that read S widen in registers (rm_scores.hpp: ScoreSrc) -- nothing behind them knows.
enum ScoreType { SCORE_SAME, SCORE_F16, SCORE_BF16 };
template <class T> struct Request : Outputs<T> {
    // the score source: factors, or the caller's score matrix (rm_calc_metrics_scores_*, rm_recommend_scores_*): score of item i for user u =
    // S[u * lds + i]; there are then no factors (A, B null, k = 0) and no tie noise.  Every evaluated user is streamed: k_score_rows copies
    // its row of S, masked, where the sweep would have written it, k_pos_scores_given gathers the test items' scores, and the
    // finalisation is the factor call's.
    // The factors' element type `f_type` is the call's own T, or 16-bit patterns (include/recometrics_hip_half_factors.h; T is float then):
    // A and B then hold 2-byte elements wherever they lie -- the caller's arrays, the upload buffers, the resident copies -- and the kernels
    // that read them widen in registers (rm_prep.hpp: FactorSrc).  lda / ldb count elements; whoever steps through A or B steps by f_elem().
    const void *A = nullptr; size_t lda = 0; const void *B = nullptr; size_t ldb = 0; int k = 0; ScoreType f_type = SCORE_SAME;
    size_t f_elem() const { return f_type == SCORE_SAME ? sizeof(T) : 2; }
    const void *A_from(size_t user) const { return (const char *)A + user * lda * f_elem(); }
    const void *S = nullptr; ScoreType s_type = SCORE_SAME; size_t lds = 0; bool scores = false;      // (lds in elements of S)
    size_t s_elem() const { return s_type == SCORE_SAME ? sizeof(T) : 2; }
    int m = 0, n = 0;
    const int *train_p = nullptr, *train_i = nullptr; long long nnz_train = 0;       // (lists: the exclusion matrix)
    const int *test_p = nullptr, *test_i = nullptr; const T *test_v = nullptr; long long nnz_test = 0;
    int K = 0; bool cumulative = false, noise = false, cold = false; int min_items_pool = 0, min_pos_test = 0;
    unsigned long long seed = 0;               // tie noise (rm_noise.hpp): the engine of user u of the request is seeded with seed + u
    // recommendation lists (rm_recommend_*): no test matrix (`test_p` is null on the device), no metric; every user with a candidate gets its
    // ordered list in `topk_idx` / `topk_score` (the caller's arrays, the scores optional) and every user a `status` -- k_finalize_reco
    bool reco = false;
    Outputs<T> &outputs() { return *this; }
};
// Which pass of a call this is (the tie noise, rm_noise.hpp, makes several of one call), and the three groups of fields that say so.
enum PassKind {
    PASS_ORDINARY,       // the users as they are, the scores as they are
    PASS_FIRST,          // fp32 tie noise: everybody on the plain scores; the users the noise can touch are flagged (PassFlags)
    PASS_EXACT,          // fp32 tie noise: a subset of the users, each with its row of noise (PassSubset; set_exact_pass)
    PASS_NOISE_ALL       // fp64 tie noise: everybody with its row of noise
};
template <class T> struct PassSubset {             // who is evaluated, and with which noise
    const unsigned char *only_users = nullptr;     // optional [m]: evaluate only these users, leave the others' outputs alone
    const int *noise_row = nullptr; int noise_row0 = 0;      // row of each user in noise_E (null: row = user)
    const T *noise_E = nullptr; long long noise_ld = 0;      // per-item noise rows; null = scores as they are
    long long eval_users = -1;                     // users this pass evaluates when fewer than m (only_users given); -1 = all m
};
struct PassFlags {                                 // who is told about the users the noise can change
    int *noise_flag = nullptr;                     // optional [m] out (fp32 first pass): users the noise can change
    // fp32 tie noise, first pass: right before the sweep is launched the flags set so far (users with a TEST item in the noise
    // zone: all of them are known by then) are copied to `flag_snapshot`, their number to `*flag_count_host` (page-locked), and
    // `flags_event` is recorded -- the exact pass of those users can start beside the sweep (run_call)
    int *flag_snapshot = nullptr; int *flag_count_host = nullptr; hipEvent_t flags_event = nullptr;
    // fp32 tie noise of a host-pointer call in user batches: the batch only runs its FIRST pass and flags the users the noise can
    // touch in this array (its slice of a range-wide one); the exact pass over all flagged users of the range follows the
    // last batch (HostRange::exact_late) -- per batch it costs two host-side waits that keep the next batch from being enqueued
    int *first_pass_flags = nullptr;
};
struct PassRows {                                  // dense train rows handed over or remembered
    // rows built by another pass of the same call over the same users (the exact noise pass beside the first sweep reads the
    // first pass's rows instead of building 463 MB of its own at BASELINE C2)
    const unsigned *ext_bits = nullptr; long long ext_words = 0; bool ext_masked = false;
    bool same_train_rows = false;                  // a later pass of the same call over the same users' rows: dense train rows may be reused
    // decided once per call (-1 = not yet: run() asks dense_rows_fit itself) -- every pass of a call gets the answer the first one
    // got, whatever the passes in between have allocated
    int dense_fit = -1;
};
template <class T> struct PassRole : PassSubset<T>, PassFlags, PassRows { PassKind kind = PASS_ORDINARY; };
// one pass over the users of a request, or over a batch of them: the request (every pointer a DEVICE pointer), the call's identity
// and the role of the pass
// f(Src *): the kernels' source-element type of a request's S (rm_scores.hpp); the 16-bit types exist for T = float only
template <class T, class F> void with_score_src(ScoreType st, F f)
{
    if (st == SCORE_SAME) return f((const T *)nullptr);
    if constexpr (std::is_same<T, float>::value) return st == SCORE_F16 ? f((const F16Bits *)nullptr) : f((const BF16Bits *)nullptr);
    throw RmError{RM_ERR_INVALID, "16-bit scores are evaluated in fp32"};
}
// f(Src *): the same for a request's factors (Request::f_type; rm_prep.hpp: FactorSrc)
template <class T, class F> void with_factor_src(ScoreType ft, F f)
{
    if (ft == SCORE_SAME) return f((const T *)nullptr);
    if constexpr (std::is_same<T, float>::value) return ft == SCORE_F16 ? f((const F16Bits *)nullptr) : f((const BF16Bits *)nullptr);
    throw RmError{RM_ERR_INVALID, "16-bit factors are evaluated in fp32"};
}
template <class T> struct Call : Request<T>, PassRole<T> {
    Call() = default;
    explicit Call(const Request<T> &r) : Request<T>(r) {}
    // batches of one host call share the item factors: a non-zero tag says "the packed image and the |B| bound made for this
    // tag are still valid" (set by run_host_range; 0 = always repack)
    unsigned long long items_tag = 0;
    long long user0 = 0;                           // tie noise: the engine of local user u is seeded with seed + user0 + u
    // the CSR arrays of these users have been validated by an earlier pass of the same call (plan kernels k_check_csr_*)
    bool csr_checked = false;
    // an ordinary pass of a call without noise (the only kind that keeps or reuses a split, Pipeline::make_split_key)
    bool plain() const { return this->kind == PASS_ORDINARY && !this->noise; }
};
// Layout of the ten metrics of a call (Call::out): the eight top-K metrics have `per` values per user (k_metrics when cumulative,
// else one), the two AUCs one.  The requested metrics of one user, packed, are a RECORD (what k_noise_gather writes); those of
// `users` users, metric by metric -- [metric][users x width] --, a BLOCK (what a batch of the host entry leaves the device as).
struct MetricLayout {
    bool want[10]; size_t per, rec_off[10], rec_w = 0;                // metric requested; offset in a record; values per record
    template <class P> MetricLayout(P *const *outs, size_t per_) : per(per_)
    {
        for (int i = 0; i < 10; i++) { want[i] = outs[i] != nullptr; rec_off[i] = rec_w; if (want[i]) rec_w += width(i); }
    }
    size_t width(int i) const { return i >= 8 ? 1 : per; }
    size_t block_off(int i, size_t users) const { return rec_off[i] * users; }
    size_t block_size(size_t users) const { return rec_w * users; }
    // the outputs of a call whose metric block of `users` users starts at `block`
    template <class T> void point_at(T *block, size_t users, T **out) const { for (int i = 0; i < 10; i++) out[i] = want[i] ? block + block_off(i, users) : nullptr; }
};
// The three places that give a call a role other than the ordinary one.
// A first pass of the fp32 tie noise, flagging into `flag` [m]:
template <class T> inline void set_first_pass(Call<T> &c, int *flag) { c.kind = PASS_FIRST; c.noise_flag = flag; }
// the fp64 pass: a row of noise in E for every user, in user order
template <class T> inline void set_noise_for_all(Call<T> &c, const T *E, long long ld)
{
    c.kind = PASS_NOISE_ALL; c.noise_row = nullptr; c.noise_row0 = 0; c.noise_E = E; c.noise_ld = ld;
}
// an EXACT pass of the fp32 tie noise: `rows` users (those marked in `only`), each with its row of noise in E; it tells nobody
template <class T>
inline void set_exact_pass(Call<T> &c, const unsigned char *only, const int *noise_row, int row0, const T *E, long long ld, int rows)
{
    c.kind = PASS_EXACT;
    static_cast<PassSubset<T> &>(c) = PassSubset<T>{only, noise_row, row0, E, ld, rows};
    static_cast<PassFlags &>(c) = PassFlags{};
    c.csr_checked = true;                                            // (the first pass looked at every row)
}
// internal status: some CSR row is not sorted (the entry points sort a copy of the rows and run again; never returned to a caller)
constexpr int RM_INTERNAL_UNSORTED = 1000;

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

template <class T> __global__ void k_iota(T *p, int count)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) p[i] = (T)i;
}

template <class S>
__global__ void k_export_rank(int m, int K, const Entry<S> *merged, int *topk_idx, S *topk_score, const int *flags)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long long)m * K || (flags[i / K] & UF_SKIP)) return;
    topk_idx[i] = merged[i].idx;
    topk_score[i] = merged[i].s;
}

__global__ void k_export_pos_rank(long long nnz, int m, const int *test_p, const int *flags, const int *pos_order,
                                  const long long *rank_sorted, long long *pos_rank, int have_ranks, const int *status)
{
    // one thread per user row (rows are short).  Users that were never ranked (skipped, or NDCG-only) have no entry in
    // pos_order -- whatever the workspace held before -- and report rank 0.  So does a user that k_finalize found invalid
    // (status 1: every candidate score the same, an infinite one): k_finalize clears its rows of rank_sorted, but the ranks of a
    // STREAMED user are still being counted on the side stream while it runs (auc_defer_slot0) and landed on top of the zeros.
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= m || (flags[u] & UF_SKIP)) return;
    const bool ranked = have_ranks && (flags[u] & UF_ACTIVE) && !(flags[u] & UF_ONLY_NDCG) && !(status && status[u] == 1);
    for (int e = test_p[u]; e < test_p[u + 1]; e++) pos_rank[e] = ranked ? rank_sorted[test_p[u] + pos_order[e]] : 0;
}

// factor groups of 8 a call with k factors runs as: the smallest count the table has a kernel for, beyond those whole chunks
template <class Args> int table_ng(int k, int chunk)
{
    const int ng = std::max(1, (k + 7) / 8);
    int best = 0;
    for (int u = 0;; u++) {
        const SweepRows<Args> r = sweep_rows<Args>(u);
        if (!r.row) break;
        for (int i = 0; i < r.n; i++) if (r.row[i].key.ng >= ng && (!best || r.row[i].key.ng < best)) best = r.row[i].key.ng;
    }
    return best ? best : (ng + chunk - 1) / chunk * chunk;
}

// ---- per-precision traits: which sweep kernel, which operand image, how many users ride on a wavefront ----
template <class T> struct Prec;
template <> struct Prec<float> {
    static constexpr int GU = GROUP_USERS;               // users per group
    typedef float4 PackT;  typedef u32x2 ListT;  typedef SweepArgs Args;
    static int supported_ng(int k) { return table_ng<Args>(k, 16); }      // beyond 512 factors: whole 128-factor chunks
    static const char *limit() { return "unsupported factor count"; }
    static size_t lds_b(int NG, int tile = TILE_ITEMS) { return 2ull * std::min(NG, 16) * 2 * tile * 16; }
    static long long items_units(int tiles, int NG, int tile = TILE_ITEMS) { return (long long)tiles * NG * 2 * tile; }
    static long long users_units(int groups, int NG) { return (long long)groups * NG * 2 * GU; }
    static constexpr bool has_pending = true, pending_for_append = false;   // appends of K > 32 are single stores already
    static constexpr size_t pend_key_bytes = 8;
    static constexpr int pend_cap_max = 8;                // keys per lane: measured flat from 3 to 8 at C2, best at 6-8
    static constexpr int max_nsub = 3;
    static size_t lists_b(int, int K) { return (size_t)GROUPS_PER_BLOCK * (K + 2) * GU * 8; }      // one list per group, shared by its waves
    // K > 32: entries per lane buffer of the sweep (rm_list.hpp; a multiple of 16, and a selection's K + slack survivors plus a tile's
    // sixteen appends must fit one lane: 2K + 16), lanes per user
    static int lane_cap(int K) { return (2 * K + 16 + 15) / 16 * 16; }
    static constexpr int lanes_per_user = 2, lane_tile = 16;
};
template <> struct Prec<double> {
    static constexpr int GU = GROUP_USERS64;
    typedef double2 PackT;  typedef u32x4 ListT;  typedef Sweep64Args Args;
    static int supported_ng(int k) { return table_ng<Args>(k, 8); }       // beyond 512 factors: whole 64-factor chunks
    static const char *limit() { return "unsupported factor count"; }
    static size_t lds_b(int NG, int = TILE_ITEMS) { return 2ull * std::min(NG, 8) * 4 * TILE_ITEMS * 16; }
    static long long items_units(int tiles, int NG, int = TILE_ITEMS) { return (long long)tiles * NG * 4 * TILE_ITEMS; }
    static long long users_units(int groups, int NG) { return (long long)groups * NG * 4 * GU; }
    static constexpr bool has_pending = true, pending_for_append = true;    // saves four 64-bit shuffles per candidate register
    static constexpr size_t pend_key_bytes = 12;
    static constexpr int pend_cap_max = 3;                // a user spans four lanes here: larger buffers only delay the bound (measured)
    static constexpr int max_nsub = 2;
    static size_t lists_b(int ns, int K) { return 4ull * ns * K * GU * sizeof(ListT); }               // one list per wave
    // (four lanes per user: K + slack + a tile's eight appends must fit ONE lane, the user's four hold ~5K together)
    static int lane_cap(int K) { return (K + lane_sel_slack(K) + 8 + 16 + 15) / 16 * 16; }
    static constexpr int lanes_per_user = 4, lane_tile = 8;
};

inline void check_launch(int rc)
{
    if (rc == -1) throw RmError{RM_ERR_UNSUPPORTED, "unsupported factor count"};
    if (rc != 0) throw RmError{RM_ERR_HIP, std::string("sweep launch: ") + hipGetErrorString((hipError_t)rc)};
}
// The launch ledger (tests: rm_debug_sweep_launched): successful launches per row of the table since the last reset, one counter per
// row and precision, in the order rm_debug_sweep_variants lists the rows.  Host only; the shards of one call launch from several
// host threads, hence the atomics (relaxed: a test reads them after its call has returned).
constexpr int LEDGER_ROWS = 512;                          // more than either table has (272 / 143): a longer table stops being counted behind it
std::atomic<int> g_sweep_launched[2][LEDGER_ROWS];
template <class Args> inline std::atomic<int> *sweep_ledger() { return g_sweep_launched[std::is_same<Args, Sweep64Args>::value ? 1 : 0]; }
template <class Args> inline void count_launch(const SweepRow<Args> *row)
{
    for (int u = 0, base = 0;; u++) {
        const SweepRows<Args> r = sweep_rows<Args>(u);
        if (!r.row) return;
        if (row >= r.row && row < r.row + r.n) {
            const int i = base + (int)(row - r.row);
            if (i < LEDGER_ROWS) sweep_ledger<Args>()[i].fetch_add(1, std::memory_order_relaxed);
            return;
        }
        base += r.n;
    }
}
template <class Args>
void dispatch_sweep(bool auc, bool dump, bool llds, int nsub, int NG, dim3 grid, size_t lds, hipStream_t stream, const Args &sa)
{
    SweepKey key;
    const SweepRow<Args> *row = sweep_key<Args>(NG, sa.ngt, auc, dump, llds ? LM_LDS : (sa.buffered_lists ? LM_HBM_APPEND : LM_HBM), nsub, sa.spec, key)
                                    ? find_sweep<Args>(key) : nullptr;
    const int rc = row ? row->launch(grid, lds, stream, sa) : -1;
    if (rc == 0) count_launch(row);
    check_launch(rc);
}

// (Src: float, or 16-bit patterns -- the images are the same fp32 images)
template <class Src>
inline void pack_operands(const Src *A, size_t lda, const Src *B, size_t ldb, int n, int k, int NG, int tile_items, const int *slot_user,
                          int n_slots, float4 *Ap, long long ap, float4 *Bp, long long bp, hipStream_t stream, bool items = true)
{
    if (items) {
        const size_t lds = pack_items_tile_lds(NG, tile_items);
        const long long tiles = bp / ((long long)NG * 2 * tile_items);
        // (the attribute is per DEVICE -- rm_set_devices drives several -- so it is set at every launch, like every other kernel of
        // the library that takes more than 64 KB; a refusal falls back to the kernel that needs no LDS)
        bool tiled = lds <= 96 * 1024 && tiles * NG * 2 * tile_items == bp;
        if (tiled && lds > 48 * 1024)
            tiled = hipFuncSetAttribute((const void *)k_pack_items_tile<float, Src>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess;
        if (tiled) {
            hipLaunchKernelGGL((k_pack_items_tile<float, Src>), dim3((unsigned)tiles), dim3(256), lds, stream, B, ldb, n, k, NG, tile_items, Bp);
            if (hipGetLastError() != hipSuccess) tiled = false;
        }
        if (!tiled) hipLaunchKernelGGL((k_pack_items<float, Src>), dim3(cdiv(bp, 256)), dim3(256), 0, stream, B, ldb, n, k, NG, tile_items, Bp, bp);
    }
    if (ap > 0) hipLaunchKernelGGL((k_pack_users<float, Src>), dim3(cdiv(ap, 256)), dim3(256), 0, stream, A, lda, k, NG, slot_user, n_slots, Ap, ap);
}
inline void pack_operands(const double *A, size_t lda, const double *B, size_t ldb, int n, int k, int NG, int, const int *slot_user,
                          int n_slots, double2 *Ap, long long ap, double2 *Bp, long long bp, hipStream_t stream, bool items = true)
{
    if (items) hipLaunchKernelGGL(k_pack_items64<double>, dim3(cdiv(bp, 256)), dim3(256), 0, stream, B, ldb, n, k, NG, Bp, bp);
    if (ap > 0) hipLaunchKernelGGL(k_pack_users64<double>, dim3(cdiv(ap, 256)), dim3(256), 0, stream, A, lda, k, NG, slot_user, n_slots, Ap, ap);
}

// a call's factors through pack_operands / k_absmax, typed by Request::f_type
template <class T, class PackT>
inline void pack_call_operands(const Request<T> &c, int n, int NG, int tile_items, const int *slot_user, int n_slots, PackT *Ap, long long ap,
                               PackT *Bp, long long bp, hipStream_t stream, bool items)
{
    with_factor_src<T>(c.f_type, [&](auto *src) {
        typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
        pack_operands((const Src *)c.A, c.lda, (const Src *)c.B, c.ldb, n, c.k, NG, tile_items, slot_user, n_slots, Ap, ap, Bp, bp, stream, items);
    });
}
template <class T>
inline void launch_absmax(ScoreType f_type, const void *X, size_t ld, long long rows, int k, unsigned blocks, hipStream_t stream,
                          unsigned long long *amax_bits, int *nonfinite)
{
    with_factor_src<T>(f_type, [&](auto *src) {
        typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
        hipLaunchKernelGGL((k_absmax<T, Src>), dim3(blocks), dim3(256), 0, stream, (const Src *)X, ld, rows, k, amax_bits, nonfinite);
    });
}

constexpr size_t LDS_LIMIT = 160 * 1024;
constexpr size_t SYNC_BYTES = 32;          // end of the sweep's LDS: arrival counters of the sub-tiles (4 words), list locks of the groups (4 words)

// HBM the score rows of streamed users (and of every user when k_metrics > 256) may take: a third of what is free now, or
// RM_STREAM_BUDGET_MB (tests)
// (what the workspace already holds of exactly these buffers counts as free: a later batch of the same size must get the
// same answer as the first one, whose rows are still cached -- otherwise its budget shrinks and an equal-sized batch fails)
inline long long free_plus_owned(const Workspace &ws, std::initializer_list<WsBuf> ids)
{
    size_t fr = 0, tot = 0;
    HIP_CHECK(hipMemGetInfo(&fr, &tot));
    const long long sim = debug_free_cap();
    if (sim >= 0) fr = (size_t)std::max<long long>(0, std::min<long long>((long long)fr, sim - g_ws_bytes.load()));
    long long owned = 0;
    for (WsBuf id : ids) owned += (long long)ws.peek(id).real;
    return (long long)fr + owned;
}
// elements between two stored score rows of n items (stream_scores, the tie noise's rows): whole tiles of either size of the sweep (64 / 96 items)
inline long long score_row_stride(long long n) { return (n + 191) / 192 * 192; }
inline long long stream_budget_bytes(const Workspace &ws)
{
    if (g_sw.stream_budget_mb >= 0) return g_sw.stream_budget_mb << 20;
    return free_plus_owned(ws, {WS_STREAM_SCORES, WS_SEL_HI, WS_SEL_LO}) / 3;
}

// Which top-K scheme a pass takes (rm_sweep.hpp LMODE):
//   lane lists   per-lane append buffers + lane-parallel selection + k_collect_topk (rm_list.hpp): k_metrics from `lane_min_k` (20 / 14; the
//                replace-the-minimum lists rescan K entries per insert: BASELINE C2's shape took 8.1 / 15.0 / 26.8 ms at K = 20 /
//                32 / 50 in LDS or HBM lists against 8.1 / 8.7 / 10.0 here, profiles/r6_ksweep_C2.txt) up to what k_collect_topk sorts in LDS (K + one lane buffer <= 4,096 entries: K <= 1,354), while the
//                buffers -- 8 waves x 64 lanes x lane_cap entries per block of the sweep's grid -- fit a third of the free memory;
//   lists        below that: in LDS while they fit, else replace-the-minimum in HBM;
//   ext_topk     beyond: one score row per user + k_select_topk.
// (Larger buffers -- sized so that one selection per item range is the rule -- were measured in round 6 and are SLOWER: what a range
// costs is the entries its selections scan in all, which hardly depends on the size, and larger buffers lose the L2: BASELINE C2's shape
// at K = 100: 12.9 ms with 304 entries per lane, 12.7 with 448, against 12.4 with the base size and 12.2 with 160; profiles/r6_ab_c2.txt)
template <class T> inline long long lane_list_bytes(int K, long long n_blocks) { return n_blocks * 8 * WAVE * (long long)Prec<T>::lane_cap(K) * (long long)(sizeof(T) + 4); }
// (`three_subtiles`: the kernel the replace-the-minimum lists would run on has three sub-tiles per step -- fp32 up to 64 factors -- which
// the lane buffers do not (a user's candidates over three waves: slower, r6h): there the lists hold out until K = 20.  Where both run
// two sub-tiles the lane buffers' lighter epilogue wins from K = 14: north-star shape K = 16 77.4 against 78.9 ms, K = 20 77.6 / 79.9,
// K = 12 77.45 / 77.41; C3 (cumulative K = 20) 110.9 / 115.2, K = 10 equal, K = 5 111.0 / 108.4; profiles/r6_ab_c2.txt r6m)
template <class T> inline bool lane_lists_possible(int K, bool three_subtiles = false)
{
    // (fp64: every k_metrics -- a user sits on four lanes there and the lists' owner lane collects from all of them: C5's shape K = 5
    // 73.4 against 74.8 ms, K = 10 73.6 / 76.4, K = 20 75.1 / 84.2; C2's shape in fp64 K = 10 4.50 / 5.22, K = 14 4.50 / 6.28)
    const long long min_k = g_sw.lane_min_k >= 0 ? g_sw.lane_min_k : (three_subtiles ? 20 : (sizeof(T) == 8 ? 1 : 14));
    return !g_sw.ext_topk && K >= min_k && K + Prec<T>::lane_cap(K) <= COLLECT_MAX_ENTRIES;
}
// (the grid of the sweep is only known behind the plan: user blocks of the call, or a few rounds of 256 blocks when there are few)
template <class T> inline long long lane_blocks_bound(long long m) { return (m + 4 * Prec<T>::GU - 1) / (4 * Prec<T>::GU) + 1024; }
inline long long lane_budget_bytes(const Workspace &ws) { return free_plus_owned(ws, {WS_GLISTS, WS_STREAM_SCORES, WS_SEL_HI, WS_SEL_LO}) / 3; }
template <class T> inline bool lane_lists_fit(const Workspace &ws, int K, long long m, bool three_subtiles)
{
    return lane_lists_possible<T>(K, three_subtiles) && lane_list_bytes<T>(K, lane_blocks_bound<T>(m)) <= lane_budget_bytes(ws);
}

// Dense train rows for the fp32 sweep when they are small (m * n / 8 bytes <= 1 GiB, e.g. 463 MB at BASELINE C2): with ~100
// train items per user among 27k items, some lane of a wave has one in nearly every 32-item sub-tile, and the per-item walk of
// the CSR cursor (compare, consume, reload, loop) was 9 % of the C2 sweep; one word per lane and tile replaces it.
// (rows are padded to 192 items = a whole tile of either size, 64 or 96: the row stride does not depend on the sweep's geometry,
// which is only known behind the plan read-back -- the rows are built before it, beside the plan kernels)
inline long long dense_row_words(long long n) { return score_row_stride(n) / 32; }
// Up to 1 GiB of rows always; beyond that (many users at a small item count: 1M users x 27k items = 3.4 GB) when they take no more
// than a quarter of the HBM that is free -- what the workspace already holds of the rows and of the streamed users' score rows counts
// as free, so that equal calls get equal answers -- and no more than 8 GiB: the sweep indexes the rows by 32-bit word offsets.
// (One answer per call: the first pass asks, Call::dense_fit carries the answer to the others.)
inline bool dense_rows_fit(const Workspace &ws, int m, long long n)
{
    const long long words = dense_row_words(n);
    if (words > TRAIN_BITS_MAX_WORDS || g_sw.no_train_bits) return false;
    const unsigned long long bytes = (unsigned long long)m * (unsigned long long)words * 4ull;
    if (bytes <= (1ull << 30)) return true;
    if (bytes > (8ull << 30)) return false;
    return (long long)bytes <= free_plus_owned(ws, {WS_TRAIN_BITS, WS_STREAM_SCORES, WS_SEL_HI, WS_SEL_LO}) / 4;
}
// `mask_test`: the rows mark the users' TEST items as well (k_merge_positives puts them back after the sweep; rm_noise.hpp clears
// the test items' bits in its own copy of a row)
// `early`: the rows were launched before the plan was known (run(): on the side stream, beside the plan kernels) with the guess
// `early_masked`; when the guess holds nothing is launched here
template <class C> inline void set_train_bits(SweepArgs &sa, Ctx &cx, const C &c, int m, int n, bool fit, hipStream_t stream, bool mask_test, bool early = false, bool early_masked = false,
                                              unsigned char *ent_masked = nullptr)
{
    Workspace &ws = cx.ws;
    const long long words = dense_row_words(n);
    const size_t bytes = (size_t)m * (size_t)words * 4;
    sa.train_bits = nullptr; sa.train_words = 0;
    if (!fit) { cx.dense.invalidate(); return; }
    unsigned *bits = (unsigned *)ws.get(WS_TRAIN_BITS, bytes);
    // (the exact second pass of the tie noise evaluates a subset of the same users: the rows of the first pass are still there)
    const bool ready = (early && early_masked == mask_test) || (c.same_train_rows && cx.dense.fits(ws, m, words, mask_test));
    if (!ready)
        launch_train_bits(stream, m, n, (int)words, c.train_p, c.train_i, (mask_test || ent_masked) ? c.test_p : nullptr, c.test_i, bits,
                          ws.array<Plan>(WS_PLAN, 1), c.only_users, ent_masked, mask_test);
    cx.dense.set(ws, words, m, mask_test, ready ? cx.dense.partial : c.only_users != nullptr, c.items_tag, c.train_p);
    sa.train_bits = bits; sa.train_words = (int)words;
}
template <class C> inline void set_train_bits(Sweep64Args &, Ctx &, const C &, int, int, bool, hipStream_t, bool, bool = false, bool = false, unsigned char * = nullptr) {}
inline void set_part_extra(SweepArgs &sa, int extra) { sa.part_extra = extra; }
inline void set_part_extra(Sweep64Args &, int) {}
// the sweep variant with the epilogue's switches as constants (rm_sweep.hpp k_sweep SPEC): 1 = dense train rows, 2 = CSR cursor,
// both with every score finite, no tie noise and the top-K lists in reach; anything else reads the switches at run time
inline void set_spec(SweepArgs &sa)
{
    sa.spec = (sa.check_nan || sa.noise_E || sa.ext_topk || g_sw.no_spec) ? 0 : (sa.train_bits ? 1 : 2);
}
inline void set_spec(Sweep64Args &sa) { sa.spec = (sa.check_nan || sa.noise_E || sa.ext_topk || g_sw.no_spec) ? 0 : 1; }
inline void set_ext_bits(SweepArgs &sa, const unsigned *bits, int words) { sa.train_bits = bits; sa.train_words = words; }
inline void set_ext_bits(Sweep64Args &, const unsigned *, int) {}

// Sample seeds for the lane buffers (k_seed_from_sample): how many items, and the two launches.  Not when a
// score may be non-finite (the NaN check wants every score looked at) and not under the tie noise (the sample is scored without it).
template <class T> inline int sample_seed_items(const Workspace &ws, int K, int n, long long n_slots, bool off, bool lists = false)
{
    if (off || g_sw.sample_seed == 0) return 0;
    int S;
    if (g_sw.sample_seed > 0) {          // forced (tests, A/B timing): the largest size at or below the value; 64 and 256 for small catalogues
        S = 64;
        for (int c : {256, 1024, 2048, 4096}) if (g_sw.sample_seed >= c) S = c;
    } else {
        // A sample of S items costs S / n of the sweep's matrix work and gives the K-th best of S as the bound.  Measured at BASELINE
        // C2's shape (26,744 items; profiles/r6_ab_c2.txt): 1,024 items beat 2,048 up to k_metrics ~ 128, 2,048 beyond, 4,096 from ~ 400.
        // (k_metrics = 500: sweep 22.5 ms without, 13.9 with 2,048, 10.9 with 4,096 in front of which the sample costs 1.9 ms more; 1,000: 36.8 / 22.8 / 16.0)
        S = K <= 128 ? 1024 : (K <= 384 ? 2048 : 4096);
        // The replace-the-minimum lists (fp32, k_metrics below the lane buffers') rescan their K entries per insert, and most inserts come
        // while the bound is still low: a sample of 256 pays from K = 12 -- C2's shape, M users/s without / with: K = 11 17.3 / 17.0, 12 16.6 / 16.8,
        // 14 15.8 / 16.5, 16 15.0 / 15.7, 18 14.7 / 15.2 (1,024 items: the same within 1 %); at K = 10 the sweep goes 6.34 -> 6.24 ms and the
        // sample costs 0.14
        if (lists) { if (K < 12) return 0; S = 256; }
        if ((long long)S * 6 > n || K * 2 > S) return 0;
        // (fp64 takes the lane buffers from k_metrics = 1: at C2's shape in fp64 the sample pays from ~ 16 -- step 19.6 -> 19.0 ms at 20,
        // 25.9 -> 22.2 at 100, 34.8 -> 30.7 at 256; even at 10)
        if (sizeof(T) == 8 && K < 16) return 0;
    }
    if (S > n || K > S) return 0;
    if ((long long)sizeof(T) * n_slots * S > free_plus_owned(ws, {WS_SAMPLE_SCORES}) / 8) return 0;
    return S;
}
template <class T, class Args>
inline void seed_from_sample(const Args &sa, Workspace &ws, int S, int NG, int n_slots, int n_ublocks, hipStream_t stream, const void *items64 = nullptr, void *lists = nullptr)
{
    typedef Prec<T> P;
    typedef typename std::remove_pointer<decltype(Args{}.thr_shared)>::type ThrT;
    T *sample = ws.array<T>(WS_SAMPLE_SCORES, (size_t)n_slots * (size_t)S);
    Args sd = sa;
    sd.n = S; sd.tiles_total = S / TILE_ITEMS; sd.K = 1; sd.n_splits = 1; sd.tail_ublocks = 0; sd.tail_splits = 1; sd.part_splits = 1;
    sd.buffered_lists = 0; sd.ext_topk = 0; sd.lane_cap = 0; sd.lane_cnt = nullptr; sd.spec = 0; sd.dump = sample;
    // (a sweep with three sub-tiles per step has its item image in 96-item tiles and its dense train rows in words of them: the DUMP
    // variant, two sub-tiles, gets an image of the sample of its own and no dense rows -- the seed kernel walks the sparse rows)
    if (items64) { sd.Bp = (decltype(sd.Bp))items64; sd.glists = (decltype(sd.glists))lists; set_ext_bits(sd, nullptr, 0); }
    sd.pend_cap = 0;  sd.pend_off = 0;
    sd.sync_off = (int)P::lds_b(NG);
    dispatch_sweep(false, true, false, 2, NG, dim3((unsigned)n_ublocks), P::lds_b(NG) + SYNC_BYTES, stream, sd);
    const dim3 grid((unsigned)cdiv(n_slots, 4)), block(256);
#define RM_SEED_LAUNCH(NV) hipLaunchKernelGGL((k_seed_from_sample<T, ThrT, NV>), grid, block, 0, stream, n_slots, sa.K, (const T *)sample, sa.slot_user, sa.slot_chunk, sa.train_p, sa.train_i, sa.thr_shared)
    switch (S) {
    case 4096: RM_SEED_LAUNCH(64); break;
    case 2048: RM_SEED_LAUNCH(32); break;
    case 1024: RM_SEED_LAUNCH(16); break;
    case 256: RM_SEED_LAUNCH(4); break;
    default: RM_SEED_LAUNCH(1); break;
    }
#undef RM_SEED_LAUNCH
    check_launch(hipGetLastError());
}

// what the plan's validation kernels found wrong with the caller's CSR arrays -> the error the entry points see
template <class T>
void throw_csr_defects(const Plan &hp, const Call<T> &c, Ctx &cx)
{
    const bool unsorted = hp.csr_desc_all[0] != hp.csr_desc_legit[0] || hp.csr_desc_all[1] != hp.csr_desc_legit[1];
    if (!hp.csr_bad && !unsorted) return;
    cx.dense.invalidate();                                         // (dense train rows launched beside the plan were not built)
    if (hp.csr_bad & CSR_BAD_INDPTR)
        throw RmError{RM_ERR_INVALID, "CSR index pointers of row " + std::to_string((long long)c.user0 + hp.csr_where) + " are negative, decreasing or beyond the index array"};
    if (hp.csr_bad & CSR_BAD_INDEX)
        throw RmError{RM_ERR_INVALID, "CSR column index out of range [0, " + std::to_string(c.n) + ") in row " + std::to_string((long long)c.user0 + hp.csr_where)};
    throw RmError{RM_INTERNAL_UNSORTED, "CSR rows are not sorted"};
}
// the validation of the index ARRAYS (the index pointers are k_classify's / k_check_csr_ptr's): `nnz_*` bound the grids -- the
// kernels look up the entry range of this call's rows themselves
inline void launch_csr_index_checks(int m, int n, const int *train_p, const int *train_i, long long nnz_train, const int *test_p, const int *test_i, long long nnz_test,
                                    Plan *plan, hipStream_t stream)
{
    hipLaunchKernelGGL(k_check_csr_starts, dim3(cdiv(m, 1024)), dim3(1024), 0, stream, m, train_p, train_i, test_p, test_i, plan);
    auto blocks = [](long long nnz) { return dim3((unsigned)std::min<long long>((nnz / 4 + 2 + CHECK_FLAT_THREADS - 1) / CHECK_FLAT_THREADS, CHECK_FLAT_BLOCKS)); };
    if (nnz_train > 0) hipLaunchKernelGGL(k_check_csr_flat, blocks(nnz_train), dim3(CHECK_FLAT_THREADS), 0, stream, m, n, train_p, train_i, plan, 0);
    if (nnz_test > 0) hipLaunchKernelGGL(k_check_csr_flat, blocks(nnz_test), dim3(CHECK_FLAT_THREADS), 0, stream, m, n, test_p, test_i, plan, 1);
}
inline void launch_csr_checks(int m, int n, const int *train_p, const int *train_i, long long nnz_train, const int *test_p, const int *test_i, long long nnz_test,
                              Plan *plan, hipStream_t stream)
{
    hipLaunchKernelGGL(k_check_csr_ptr, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, train_p, nnz_train, test_p, nnz_test, plan);
    launch_csr_index_checks(m, n, train_p, train_i, nnz_train, test_p, test_i, nnz_test, plan, stream);
}
// the validation alone, with its own wait: for the callers that index by the CSR arrays BEFORE the pipeline runs (the fp64 tie noise
// builds its noise rows -- candidate index = item - train items below it -- in front of run())
template <class T>
void check_csr_now(const Call<T> &c, hipStream_t stream, Ctx &cx)
{
    Plan *plan = cx.ws.array<Plan>(WS_PLAN, 1);
    cx.split.invalidate();                                         // (the Plan is zeroed below)
    if (cx.ev_valid) HIP_CHECK(hipStreamWaitEvent(stream, cx.done, 0));
    HIP_CHECK(hipMemsetAsync(plan, 0, sizeof(Plan), stream));
    launch_csr_checks(c.m, c.n, c.train_p, c.train_i, c.nnz_train, c.test_p, c.test_i, c.nnz_test, plan, stream);
    Plan hp;
    HIP_CHECK(hipMemcpyAsync(&hp, plan, sizeof(Plan), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    throw_csr_defects(hp, c, cx);
}

// ---------------------------------------------------------------------------------------------------------------------
// device pipeline (T = float: v_mfma_f32_32x32x2_f32 sweep; T = double: v_mfma_f64_16x16x4_f64 sweep)
// ---------------------------------------------------------------------------------------------------------------------
// A stream of the context beside the call's (the side stream, the positives' stream), created on first use with its events, and the
// order between the two (roles: SideMark / PosMark):
//   cut(role) / behind(role)  the call's stream records a point; the stream beside waits for it and is handed out (fork = both);
//   on()                      ... handed out again, with nothing new to wait for;
//   mark(role) / await(role, into)  the stream beside records what it was given so far; `into` -- the call's stream, or a third one --
//                             waits for that (join = mark + await by the call's stream).
// A handle is good until the next mark: work enqueued behind a mark asks for the stream again.  Every hand-out counts, a mark
// remembers the count, and the call's stream has JOINED what it awaited (or the host waited for: sync) and, the stream being in order,
// all before it.  An error between a hand-out and its join must not leave the stream reading the call's buffers behind the caller's
// back: the destructor waits when something is outstanding.  Switched off (RM_DEBUG_NO_SIDE) every hand-out is the call's stream.
struct Beside {
    hipStream_t &st; hipEvent_t *const ev; const int n_ev; const hipStream_t call; const bool high_priority; bool enabled;
    long long handed = 0, joined = 0, at[SIDE_MARKS] = {};      // at[role]: 0 = no mark the call's stream has yet to await
    static_assert((int)POS_MARKS <= (int)SIDE_MARKS, "at[] holds the roles of either stream");
    Beside(hipStream_t &s, hipEvent_t *e, int n, hipStream_t call_, bool hp, bool on_) : st(s), ev(e), n_ev(n), call(call_), high_priority(hp), enabled(on_) {}
    ~Beside() { if (handed > joined && st) (void)hipStreamSynchronize(st); }
    hipStream_t get()
    {
        if (!st) {
            HIP_CHECK(create_stream(&st, high_priority));
            for (int i = 0; i < n_ev; i++) HIP_CHECK(hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
        }
        return st;
    }
    hipStream_t on() { if (!enabled) return call; handed++; return get(); }
    void cut(int role) { if (enabled) { get(); HIP_CHECK(hipEventRecord(ev[role], call)); } }
    hipStream_t behind(int role) { if (!enabled) return call; HIP_CHECK(hipStreamWaitEvent(st, ev[role], 0)); handed++; return st; }
    hipStream_t fork(int role) { cut(role); return behind(role); }
    void mark(int role) { if (enabled) { HIP_CHECK(hipEventRecord(ev[role], st)); at[role] = handed; } }
    void joined_at(int role) { joined = std::max(joined, at[role]); at[role] = 0; }
    void await(int role, hipStream_t into) { if (enabled) { HIP_CHECK(hipStreamWaitEvent(into, ev[role], 0)); if (into == call) joined_at(role); } }
    void join(int role) { mark(role); await(role, call); }
    bool marked(int role) const { return at[role] != 0; }              // marked, and the call's stream has not been told to wait yet
    void sync() { if (enabled && st) { HIP_CHECK(hipStreamSynchronize(st)); joined = handed; } }      // the HOST waits (the second plan)
    void host_wait(int role) { if (enabled) { HIP_CHECK(hipEventSynchronize(ev[role])); joined_at(role); } }      // ... for a mark only
};

// LDS of a sweep block of depth j (each group's positives table is aligned to its own size, 2^j rows of GU scores: worst-case
// padding = one table)
template <class T> inline size_t sweep_lds(int NG, int K, bool want_auc, bool with_lists, int ns, int j)
{
    typedef Prec<T> P;
    const size_t head = P::lds_b(NG, 32 * ns) + (with_lists ? P::lists_b(ns, K) : 0);
    const size_t tb = ((size_t)1 << j) * P::GU * sizeof(T);
    return want_auc ? (head + tb - 1) / tb * tb + (size_t)GROUPS_PER_BLOCK * (1 << j) * P::GU * (sizeof(T) + 4) : head;
}

// The sweep's geometry: sub-tiles, the two-level grid, the list scheme, the LDS carve-up and the depth split.  A pure function of
// the plan's read-back, the call's shape and the switches.
struct Geometry {
    int jmax, n_ublocks, nsub, tile_items, n_waves, tiles_total;
    int n_splits, tail_ublocks, tail_splits, part_splits;
    bool mask_test, use_ext_bits, list_in_lds, want_pending;
    int n_part, part_extra;
    size_t per_key, lds_total, sync_off; int pend_cap;
    int u_split, j_shallow; size_t lds_l;                  // depth split: the shallow user blocks [0, u_split) with their lists in LDS
};
// blocks of a sweep launch over `n_ublocks` user blocks of the two-level grid, `tail_ublocks` of them cut into the tail's item ranges
inline unsigned sweep_blocks(int n_ublocks, int tail_ublocks, const Geometry &g) { return (unsigned)((n_ublocks - tail_ublocks) * g.n_splits + tail_ublocks * g.tail_splits); }
template <class T>
Geometry sweep_geometry(const Call<T> &c, const Plan &hp, int NG, bool want_auc, bool want_lane, bool ext_topk, bool check_nan, bool dense_ok,
                        const Switches &sw)
{
    typedef Prec<T> P;
    const int n = c.n, K = c.K;
    Geometry g{};
    g.jmax = want_auc ? hp.jmax : 0;
    g.n_ublocks = (hp.n_groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK;
    const int n_ublocks = g.n_ublocks;
    auto lds_need_n = [&](bool with_lists, int ns) { return sweep_lds<T>(NG, K, want_auc, with_lists, ns, g.jmax); };
    // sub-tiles per step (waves per block = 4 nsub): three when the fp32 kernel for <= 64 factors keeps its lists in LDS
    // next to the larger item tile -- the third wave per SIMD fills the vector pipe the epilogue leaves idle
    // (three sub-tiles with the lane buffers of larger k_metrics were built and measured in round 6 -- 162-168 VGPRs, no spills -- and are
    // SLOWER: a user's candidates are then spread over three waves whose bounds each see a third of the items; BASELINE C2's shape at
    // K = 100: 13.4 against 12.4 ms, profiles/r6_ab_c2.txt)
    g.nsub = 2;
    if (!ext_topk && !want_lane && P::max_nsub >= 3 && NG <= 8 && lds_need_n(true, 3) + SYNC_BYTES <= LDS_LIMIT && !sw.hbm_lists && !sw.nsub2)
        g.nsub = 3;
    // (four sub-tiles -- sixteen waves, four per SIMD, 128 registers each -- were built in round 5, passed the parity tests and were
    // 1.9 % SLOWER at BASELINE C2: profiles/r5_ab_c2.txt r5a; the patches are scratch/dropped/r5_nsub4*)
    const int nsub = g.nsub;
    g.tile_items = 32 * nsub; g.n_waves = 4 * nsub;
    g.tiles_total = (n + g.tile_items - 1) / g.tile_items;
    const int tiles_total = g.tiles_total;
    // LDS admits one block per CU, so the grid runs in rounds of 256 blocks, and a block costs its tiles plus a fixed part:
    //   block(s) = tiles_total / s + 13 (tables into LDS, the top-K lists filling up, list sort, histogram flush)
    //              + 0.4 % of the sweep per 10 of k_metrics (every item range restarts the streaming top-K lists)
    // (coefficients measured on MI355X, profiles/r2_splits*: C2, NS, C3- and C4-shaped runs).  One split count for the whole
    // grid leaves the last round partly empty -- 8.45 rounds cost 9 at C2 -- so the grid has two levels: whole rounds of
    // blocks with n_splits item ranges, then the `tail_ublocks` cheapest user blocks cut into `tail_splits` (more, smaller)
    // ranges that fill the last round.  Blocks differ in duration by ~ +-20 % (depth of the positive trees, streamed
    // users), so a part that ends the grid is charged max(whole rounds, rounds + 0.2).
    int n_splits = 1, tail_ublocks = 0, tail_splits = 0;
    if (n_ublocks > 0) {
        const int n_cu = 256;
        // (ranges of at least 16 tiles: a call with few users -- the second, exact pass of the tie noise over the flagged
        // users, a small batch -- is cut into many ranges so that its few user blocks still fill the chip)
        const int max_splits = std::max(1, std::min(MAX_PARTS / nsub, tiles_total / 16));
        const int max_tail = max_splits;
        const double fixed = 13.0 + 0.004 * std::max(0.25, K / 10.0) * tiles_total;
        auto block = [&](int sct) { return (double)tiles_total / sct + fixed; };
        // (0.2 of a round with the lane buffers, whose blocks differ by their selections; 0.1 with the lists: round 6, scratch/r6_slack.sh --
        // tutorial shape 2.57 -> 2.54 ms, 20,000 users of C2 1.14 -> 1.11, north-star shape 77.3 -> 77.2; C4 / C5 lose 5 % / 1 % below 0.2)
        const double slack = want_lane ? 0.2 : 0.1;
        auto last = [&](double rounds) { return std::max(std::ceil(rounds - 1e-9), rounds + slack); };
        double best = 1e300;
        for (int sct = 1; sct <= max_splits; sct++) {
            const double t1 = last((double)n_ublocks * sct / n_cu) * block(sct);
            if (t1 < best - 1e-9) { best = t1; n_splits = sct; tail_ublocks = 0; tail_splits = 0; }
            const long long full = (long long)n_ublocks * sct / n_cu;               // whole rounds of the main part
            const int main_ub = (int)(full * n_cu / sct), tail_ub = n_ublocks - main_ub;
            if (full == 0 || tail_ub == 0) continue;
            for (int ts = sct + 1; ts <= max_tail; ts++) {
                const double t2 = (double)main_ub * sct / n_cu * block(sct) + last((double)tail_ub * ts / n_cu) * block(ts);
                if (t2 < best * 0.99) { best = t2; n_splits = sct; tail_ublocks = tail_ub; tail_splits = ts; }
            }
        }
    }
    if (!sw.splits.empty()) {                                // A/B timing and tests: "S" or "S,tail_ublocks,tail_splits"
        int v[3] = {1, 0, 0};
        sscanf(sw.splits.c_str(), "%d,%d,%d", &v[0], &v[1], &v[2]);
        n_splits = std::max(1, std::min(v[0], std::max(1, MAX_PARTS / nsub)));
        tail_ublocks = std::max(0, std::min(v[1], n_ublocks)); tail_splits = std::max(1, std::min(v[2], std::max(1, MAX_PARTS / nsub)));
        if (tail_ublocks == 0) tail_splits = 0;
    }
    g.n_splits = n_splits; g.tail_ublocks = tail_ublocks; g.tail_splits = tail_splits;
    g.part_splits = std::max(n_splits, tail_splits);
    // fp32, small item counts (dense train rows), ROC / PR-AUC wanted: the rows mark the users' test items too, the sweep never
    // meets a candidate that IS one of the user's positives (an exact tie, resolved by the tie rule three tiles out of four at
    // 27k items), and k_merge_positives puts the test items back.  Not when a score can be non-finite (a test item masked by the
    // train row is marked +inf in the tables), not with chunked long rows (more slots than users: their best positives are not in the primary slot),
    // not beyond the lists (k_select_topk works on the stored rows).
    g.mask_test = std::is_same<T, float>::value && want_auc && !ext_topk && !check_nan && hp.n_slots > 0 &&
                  dense_ok && hp.n_slots == hp.n_active && hp.n_only_ndcg == 0 &&
                  nsub * g.part_splits + 1 <= MAX_PARTS && !sw.no_test_mask;
    // rows handed over by another pass: usable when they were built the way this pass would build them (unmasked rows are
    // always valid: the old scheme)
    g.use_ext_bits = c.ext_bits != nullptr && c.ext_words == dense_row_words(n) && (!c.ext_masked || g.mask_test);
    if (g.use_ext_bits) g.mask_test = c.ext_masked;
    g.n_part = nsub * g.part_splits + (g.mask_test ? 1 : 0);
    g.part_extra = g.mask_test ? 1 : 0;
    g.list_in_lds = !ext_topk && !want_lane && lds_need_n(true, nsub) + SYNC_BYTES <= LDS_LIMIT && !sw.hbm_lists;
    // per-lane pending buffers for top-K candidates behind everything else (fp32: not for the append-buffer lists of K > 32, whose
    // appends are already single stores).  The kernel sizes its tables per block (by the block's own depth) and computes the
    // pending capacity from what is left below the counter: allocate for the deepest block plus, if it still fits, the keys per lane
    g.want_pending = !ext_topk && !want_lane && P::has_pending && !sw.no_pending;
    g.per_key = (size_t)g.n_waves * WAVE * P::pend_key_bytes;            // one key per lane and wave
    g.pend_cap = g.want_pending ? P::pend_cap_max : 0;
    g.lds_total = std::min<size_t>(LDS_LIMIT, lds_need_n(g.list_in_lds, nsub) + SYNC_BYTES + g.pend_cap * g.per_key);
    g.sync_off = g.lds_total - SYNC_BYTES;                              // split-barrier counter of the sweep, last 16 bytes
    // Depth split: when only the deepest user blocks force the lists out of LDS (the allocation is sized per launch, the tables per
    // block), the shallow blocks [0, u_split) get their own launch with LDS lists.
    g.u_split = 0; g.j_shallow = -1; g.lds_l = 0;
    if (!g.list_in_lds && !want_lane && K <= 32 && want_auc && !sw.hbm_lists) {
        for (int j = g.jmax - 1; j >= 0 && g.j_shallow < 0; j--)
            if (sweep_lds<T>(NG, K, want_auc, true, nsub, j) + SYNC_BYTES <= LDS_LIMIT) g.j_shallow = j;
        if (g.j_shallow >= 0) g.u_split = hp.class_offset[g.j_shallow + 1] / (GROUPS_PER_BLOCK * P::GU);
    }
    if (g.u_split > 0)
        g.lds_l = std::min<size_t>(LDS_LIMIT, sweep_lds<T>(NG, K, want_auc, true, nsub, g.j_shallow) + SYNC_BYTES + g.pend_cap * g.per_key);
    return g;
}

// The caller's scores (Call::scores): there is no sweep, so no grid and no lists -- what the other stages read of the geometry is the
// row stride of the streamed users' score rows (whole 64-item tiles, as the two-sub-tile sweep of the same plan would leave them)
// and ONE part of validity statistics per slot (k_score_rows writes it).
inline Geometry scores_geometry(const Plan &hp, int n, bool want_auc)
{
    Geometry g{};
    g.jmax = want_auc ? hp.jmax : 0;
    g.n_ublocks = (hp.n_groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK;
    g.nsub = 2; g.tile_items = TILE_ITEMS; g.n_waves = 8;
    g.tiles_total = (n + TILE_ITEMS - 1) / TILE_ITEMS;
    g.n_splits = 1; g.part_splits = 1; g.n_part = 1;
    g.u_split = 0; g.j_shallow = -1;
    return g;
}

// One call through the device pipeline: the stages of DESIGN.md section 1 as members, the state they hand on as fields.
template <class T>
struct Pipeline {
    typedef Prec<T> P;
    typedef typename std::remove_pointer<decltype(typename P::Args{}.thr_shared)>::type ThrT;
    static constexpr int GU = P::GU;
    Call<T> c;                              // (a copy: a pass on a kept split reads the context's copies of the five arrays)
    hipStream_t stream; Ctx &cx; Workspace &ws;
    const int m, n, k, K;
    const bool use_side = !g_sw.no_side;    // (decides what is launched; where it only decides a stream, a record or a wait, Beside does)
    Beside side, pos;                       // kernels that do not depend on one another run beside the call's stream
    // begin
    int min_items_pool = 0, min_pos_test = 0, req = 0, NG = 0; bool want_auc = false;
    // plan
    int *flags = nullptr, *user_nslots = nullptr, *uslot_base = nullptr, *heavy_users = nullptr; Plan *plan = nullptr;
    int *slot_user = nullptr, *slot_chunk = nullptr, *slot_index = nullptr, *gj = nullptr, *sc_user = nullptr, *sc_chunk = nullptr;
    long long *grow = nullptr; double *log2tab = nullptr;
    unsigned char *slot_j = nullptr; int *tile_total = nullptr, *tile_offset = nullptr, n_tiles = 0;      // (the plan chain's own)
    ClassifyArgs ca{}; long long stream_cap = 0;          // (score rows of streamed users the budget admits)
    int *ent_user = nullptr; unsigned char *ent_masked = nullptr;      // the scores by entry (flat_early); what every positives' kernel gets:
    PosArgs<T> pa{};
    bool want_lane = false, ext_topk = false, items_known = false, dense_ok = false;
    bool row_topk = false;                  // lists from the caller's scores, selected while the row is read (k_topk_rows): no score row is stored
    bool bits_early = false, bits_early_masked = false, masked_from_bits = false, flat_early = false;
    // the split the context kept (SplitCache): may this pass run on it, does it, may the next one run on this pass's
    bool allow_reuse = true, reused = false, keepable = false; SplitKey split_key{};
    std::array<const void *, SPLIT_ARRAYS> theirs{};      // the caller's five arrays (a pass on the kept split reads the copies: `c`)
    bool hints = false; int *hint_counts_dev = nullptr;  // ... and its previous lists give this pass bounds (k_hint_bounds)
    Plan hp{};
    int n_slots = 0, n_stream = 0, stream_slot0 = 0; bool check_nan = false;
    // geometry
    Geometry g{};
    // prep
    FinalArgs<T, T> fa{};
    Entry<T> *merged = nullptr; long long *rank_sorted = nullptr;
    T *pos_score = nullptr; unsigned *hist = nullptr; int *pos_order = nullptr, *pos_item = nullptr;
    Entry<T> *pl = nullptr; PartialStat<T> *pst = nullptr;
    T *stream_scores = nullptr, *spos_score = nullptr; int *spos_item = nullptr; unsigned *shist = nullptr;
    long long stream_ld = 0;
    typename P::Args sa{};
    typename P::ListT *glists = nullptr; int *lane_cnt = nullptr; ThrT *thr_shared = nullptr;
    bool lane_lists = false;
    // sweep
    bool collect = false; CollectGeom collect_g{};

    Pipeline(const Call<T> &c_, hipStream_t s, Ctx &cx_)
        : c(c_), stream(s), cx(cx_), ws(cx_.ws), m(c_.m), n(c_.n), k(c_.k), K(c_.K),
          side(cx_.side_stream, cx_.side_marks.data(), SIDE_MARKS, s, cx_.high_priority, use_side),
          pos(cx_.pos_stream, cx_.pos_marks.data(), POS_MARKS, s, cx_.high_priority, use_side) {}

    // ---- begin: the reference's clamps, the metrics asked for, the context's events ----
    void begin()
    {
        // reference recometrics.hpp:390-393
        min_items_pool = std::max(std::max(c.min_items_pool, K), 2);
        min_pos_test = std::min(c.min_pos_test, 1);
        if (c.reco) { min_items_pool = 1; min_pos_test = 0; }          // (lists for whoever has a candidate: k_classify's `reco`)
        for (int i = 0; i < 10; i++) if (c.out[i] && !c.reco) req |= (1 << i);
        want_auc = req & (RQ_ROC | RQ_PR);
        NG = c.scores ? 2 : P::supported_ng(k);                        // (scores: no factors, no sweep -- the value is never used)
        if (NG < 0) throw RmError{RM_ERR_UNSUPPORTED, std::string(P::limit()) + " (got " + std::to_string(k) + ")"};
        if (!cx.ev_valid) {
            for (int i = 0; i < EV_COUNT; i++) HIP_CHECK(hipEventCreate(&cx.ev[i]));
            HIP_CHECK(hipEventCreateWithFlags(&cx.done, hipEventDisableTiming));
            cx.ev_valid = true;
        } else {
            HIP_CHECK(hipStreamWaitEvent(stream, cx.done, 0));          // the previous call on this context may still be running on another stream
        }
        g_last_ctx = &cx;
        HIP_CHECK(hipEventRecord(cx.ev[EV_START], stream));
        RM_TRACE_POINT("run: start");
    }

    // ---- plan: classify the users, slots and groups; beside it the CSR checks, the maxima, the early dense rows; read back ----
    void plan_stage()
    {
        user_buffers();
        list_scheme();
        slot_buffers();
        discount_table();
        beside_scheme();
        kept_split();
        if (flat_early) fill_pos_args();                               // (else positives() does: the scores by slot)
        if (reused) plan_reused();
        else for (int attempt = 0; ; attempt++) {
            plan_chain(attempt);
            beside_chain(attempt);
            enqueue_read_back(attempt);
            if (!plan_again(attempt)) break;
        }
        n_slots = hp.n_slots;
        // streamed users own the last slots; the tables and their kernels cover slots [0, stream_slot0)
        n_stream = (want_auc || ext_topk) ? hp.class_count[STREAM_CLASS] : 0;
        stream_slot0 = n_stream > 0 ? hp.class_offset[STREAM_CLASS] : n_slots;
        if (!reused) check_nan = scores_may_overflow();                // (a pass on a kept split assumes the kept answer until verdict())
    }
    void user_buffers()                     // the per-user buffers and k_classify's arguments
    {
        flags = ws.array<int>(WS_FLAGS, (size_t)m);
        user_nslots = ws.array<int>(WS_USER_NSLOTS, (size_t)m); uslot_base = ws.array<int>(WS_USLOT_BASE, (size_t)m);
        plan = ws.array<Plan>(WS_PLAN, 1);
        heavy_users = ws.array<int>(WS_HEAVY_USERS, (size_t)m);
        ca = ClassifyArgs{m, n, K, c.train_p, c.test_p, req, c.cold ? 1 : 0, min_items_pool, min_pos_test, want_auc ? 1 : 0,
                          flags, user_nslots, heavy_users, plan};
        ca.only = c.only_users; ca.reco = c.reco ? 1 : 0;
        ca.heavy_npos = K > FIN_TOPV ? FIN_TOPV : HEAVY_NPOS;
        // the caller's CSR arrays are validated in front of everything that indexes by them (an out-of-range column index in
        // k_train_bits would be a memory fault; on the CPU reference it is a segfault): the index pointers by k_classify itself, the
        // 80 MB of indices of BASELINE C2 by k_check_csr_rows beside the plan chain (~40 us)
        ca.check_ptr = c.csr_checked ? 0 : 1; ca.nnz_train = c.nnz_train; ca.nnz_test = c.nnz_test;
    }
    void list_scheme()                      // the list scheme and the stream budget (both ask for the FREE memory: they stay between the two groups of buffers)
    {
        // Users with more than POS_CHUNK test items are "streamed" (rm_device.hpp STREAM_CLASS) when a score row for each of
        // them fits the HBM budget: a third of the free memory unless RM_STREAM_BUDGET_MB says otherwise (0 = never; such
        // users then take one sweep slot per chunk of their test row -- same results, the contraction repeated per chunk).
        // The plan assumes they fit; the host looks at their number in the read-back and, should the rows not fit, plans once more
        // without streaming (what used to be two launches in front of k_classify -- count, decide -- on every call).
        const long long stream_ld_max = score_row_stride(n);
        // (a pass over a subset of the users -- the exact second pass of the fp32 tie noise -- stores rows for that subset only)
        const long long m_rows = c.eval_users >= 0 ? std::min<long long>(c.eval_users, m) : m;
        // k_metrics beyond the sweep's lists (append buffers + wave compaction reach 256): every user is streamed and
        // k_select_topk picks its top-K from the stored row -- any k_metrics <= n, at one score row of HBM per user
        want_lane = !c.scores && lane_lists_fit<T>(ws, K, m_rows, P::max_nsub >= 3 && NG <= 8);
        // (the caller's scores: the same plan -- the row every user needs is a copy of its row of S with the train items masked;
        // lists of up to ROW_TOPK_MAX_K items from them need no stored row at all: k_topk_rows, rm_rowtopk.hpp)
        row_topk = c.reco && c.scores && K <= ROW_TOPK_MAX_K && !g_sw.no_row_topk;
        ext_topk = !row_topk && ((!want_lane && K > 256) || g_sw.ext_topk || c.scores);
        if (want_auc || ext_topk) {
            stream_cap = stream_budget_bytes(ws) / (stream_ld_max * (long long)sizeof(T));
            if (ext_topk) {
                if (m_rows > stream_cap) throw RmError{RM_ERR_NOMEM, std::string(c.scores && c.reco ? "lists of more than 1024 items from a score matrix keep one masked score row (" : c.scores ? "metrics from a score matrix keep one masked score row (" : "k_metrics > 256 keeps one score row (") + std::to_string(stream_ld_max * (long long)sizeof(T)) +
                                           " B) per user in device memory: " + std::to_string(m_rows) + " users do not fit, at most " + std::to_string(stream_cap) + " per call"};
                ca.force_stream = 1;
            } else if (stream_cap > 0) ca.allow_stream = 1;
        }
    }
    void slot_buffers()                     // the per-slot and per-group tables, the tiles of the scan
    {
        const long long slot_bound = (long long)m + c.nnz_test / POS_CHUNK + 1;
        const long long group_bound = slot_bound / GU + 2;
        slot_user = ws.array<int>(WS_SLOT_USER, (size_t)slot_bound); slot_chunk = ws.array<int>(WS_SLOT_CHUNK, (size_t)slot_bound);
        slot_index = ws.array<int>(WS_SLOT_INDEX, (size_t)slot_bound); slot_j = ws.array<unsigned char>(WS_SLOT_J, (size_t)slot_bound);
        gj = ws.array<int>(WS_GJ, (size_t)group_bound); grow = ws.array<long long>(WS_GROW, (size_t)group_bound);
        sc_user = ws.array<int>(WS_SC_USER, (size_t)slot_bound); sc_chunk = ws.array<int>(WS_SC_CHUNK, (size_t)slot_bound);
        n_tiles = (int)cdiv(m, 1024);
        if (m <= 8192) return;                                   // one block walking the whole array costs ~0.5 us per 1024 entries
        tile_total = ws.array<int>(WS_SCAN_TILE_TOTAL, (size_t)n_tiles); tile_offset = ws.array<int>(WS_SCAN_TILE_OFFSET, (size_t)n_tiles);
    }
    // log2(i + 2) for the DCG discounts, from the host's libm like the reference's (:620,:902, int -> double log2).  The table
    // depends on K alone: it stays in the workspace, and only a longer one (or one for a new allocation) is uploaded again -- the
    // copy comes from pageable memory, which blocks the host and waits for the stream
    void discount_table()
    {
        if (!c.reco) log2tab = ws.array<double>(WS_LOG2TAB, (size_t)K);
        if (!c.reco && !cx.discounts.holds(ws, K)) {
            std::vector<double> lt((size_t)K);
            for (int i = 0; i < K; i++) lt[i] = std::log2(i + 2);
            HIP_CHECK(hipMemcpy(log2tab, lt.data(), sizeof(double) * (size_t)K, hipMemcpyHostToDevice));       // (synchronous: `lt` is on the stack)
            cx.discounts.set(ws, K);
        }
    }
    void beside_scheme()                    // what the call's kind lets run beside the plan chain, and where the read-back lands
    {
        items_known = cx.packed.of_call(c.items_tag);                          // a later batch of the same host call
        if (!cx.pinned_plan) HIP_CHECK(hipHostMalloc((void **)&cx.pinned_plan, sizeof(Plan), hipHostMallocDefault));
        // (one answer per call: a later pass -- the exact passes of the tie noise, on this or on a peer context with less free memory --
        // carries the first pass's answer; rows handed over by another pass are proof that they fit)
        dense_ok = !c.scores && std::is_same<T, float>::value && (c.ext_bits ? true : c.dense_fit >= 0 ? c.dense_fit != 0 : dense_rows_fit(ws, m, n));
        // the positives' stream: the streamed users' chain beside the table users', and what is made per test entry beside the plan chain
        // (the caller's scores: the test entries' scores are gathered by entry whatever the switch says -- there is no kernel by slot)
        flat_early = want_auc && !c.only_users && c.nnz_test > 0 && (!g_sw.no_pos_flat || c.scores);
    }
    // The split the context kept: when this call's key is the kept one, the pass reads the context's COPIES of the five arrays --
    // validated when they were made, and the arrays every kept table was derived from -- while k_split_same finds out whether the
    // caller's arrays still equal them: nothing is ever indexed through an array that has not been validated.
    void kept_split()
    {
        theirs = {c.train_p, c.train_i, c.test_p, c.test_i, c.test_v};
        keepable = make_split_key(split_key);
        cx.split_reused = keepable ? 0 : -1;
        reused = keepable && allow_reuse && cx.split.holds(ws, split_key) &&
                 (!dense_ok || cx.dense.fits(ws, m, dense_row_words(n), cx.split.dense_masked));
        // The lists the last pass on the kept split left in `merged` are this pass's advice (k_hint_bounds), whichever pass this is takes the
        // record away: export_ranks() of a plain pass on the kept or newly kept split makes the next one.  (Same key = same m, K,
        // precision and list scheme; the calls whose lists are the replace-the-minimum ones, seeded by k_seed_thresholds.)
        const bool lists_kept = cx.split.take_lists(ws);
        cx.hints_ran = false;
        hints = reused && lists_kept && !g_sw.no_warm_bounds && !g_sw.no_seed && want_auc && !want_lane && !ext_topk && K <= HINT_MAX_K;
        if (reused) {
            c.train_p = (const int *)cx.split.copy(ws, 0); c.train_i = (const int *)cx.split.copy(ws, 1);
            c.test_p = (const int *)cx.split.copy(ws, 2); c.test_i = (const int *)cx.split.copy(ws, 3);
            if (c.test_v) c.test_v = (const T *)cx.split.copy(ws, 4);
        } else cx.split.invalidate();                                 // (the kernels below overwrite what the record speaks of)
    }
    // `pa`, the arguments of the positives' kernels, as far as they are known in front of the first of them: with the scores by entry
    // (flat_early, which implies nnz_test > 0) the plan stage asks, and the two per-entry buffers come with them; else positives() does,
    // which adds what it allocates either way.  The factors and the CSR arrays are read BEHIND kept_split(): a pass on the kept split
    // scores through the context's copies.
    void fill_pos_args()
    {
        const size_t nz = (size_t)std::max<long long>(c.nnz_test, 1);
        if (flat_early) { ent_user = ws.array<int>(WS_ENT_USER, nz); ent_masked = ws.array<unsigned char>(WS_ENT_MASKED, nz); }
        pa.m = m; pa.n = n; pa.k = k; pa.A = c.A; pa.lda = c.lda; pa.B = c.B; pa.ldb = c.ldb;
        pa.train_p = c.train_p; pa.train_i = c.train_i; pa.test_p = c.test_p; pa.test_i = c.test_i; pa.flags = flags;
        pa.pos_tmp = ws.array<T>(WS_POS_TMP, nz);
        if (sizeof(T) == 4) pa.pos_key = (unsigned long long *)ws.get(WS_POS_KEY, 8 * (nz + 8));
        pa.noise_row = c.noise_row; pa.noise_row0 = c.noise_row0; pa.noise_E = c.noise_E; pa.noise_ld = c.noise_ld;
        pa.noise_flag = c.noise_flag; pa.plan = plan;
    }
    // ---- the plan chain: five launches that depend on one another, on the call's stream (index pointers only) ----
    void plan_chain(int attempt)
    {
        if (attempt == 0) HIP_CHECK(hipMemsetAsync(plan, 0, sizeof(Plan), stream));
        else {
            // (a second plan keeps the count of the users the tie noise's first pass has flagged so far: the positives' scores of the
            // first attempt, which count them, are not made again)
            const size_t at = offsetof(Plan, n_noise_flagged);
            HIP_CHECK(hipMemsetAsync(plan, 0, at, stream));
            HIP_CHECK(hipMemsetAsync((char *)plan + at + sizeof(int), 0, sizeof(Plan) - at - sizeof(int), stream));
        }
        hipLaunchKernelGGL(k_classify, dim3(cdiv(m, 1024)), dim3(1024), 0, stream, ca);
        // (the two forks behind k_classify, recorded BEFORE the rest of the chain is enqueued: the host needs ~4 us per launch, and the
        // chain's kernels used to reach the device 60 us late, behind everything that was enqueued for the other streams)
        side.cut(SIDE_PLAN_FORK); pos.cut(POS_PLAN_FORK);
        if (tile_total) {
            hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(1024), 0, stream, user_nslots, uslot_base, m, tile_total);
            hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, stream, tile_total, tile_offset, n_tiles, &plan->n_slots, plan, GU);
        } else hipLaunchKernelGGL(k_scan_exclusive, dim3(1), dim3(1024), 0, stream, user_nslots, uslot_base, m, &plan->n_slots, plan, GU);
        AssignArgs aa{m, c.test_p, flags, user_nslots, uslot_base, want_auc ? 1 : 0, plan, slot_user, slot_chunk, slot_index, slot_j, sc_user, sc_chunk,
                      ext_topk ? 1 : 0, tile_offset};
        hipLaunchKernelGGL(k_assign_slots, dim3(cdiv(m, ASSIGN_THREADS)), dim3(ASSIGN_THREADS), 0, stream, aa);
        hipLaunchKernelGGL(k_block_tables, dim3(1), dim3(1024), 0, stream, plan, slot_j, gj, grow, GU);
    }
    // ---- beside it: what reads the index arrays and the factors ----
    void beside_chain(int attempt)
    {
        // On the side stream the CSR rows' validation (gated on the index pointers k_classify has just checked), then the dense train
        // rows (fp32, small item counts; set_train_bits), which depend on the CSR inputs alone: they run during the rest of the plan
        // chain, the read-back -- the host's one wait of the call -- and the positives' scores.  Whether the rows also mark the test
        // items (`mask_test`) is only decided behind the read-back; the guess here is the usual answer, and a wrong guess costs one
        // more launch of the kernel behind it.  On the positives' stream max |A| and max |B| and the user of every test entry.  The
        // plan carries the checks' verdicts and the maxima: its read-back waits for both streams.
        const hipStream_t aux = side.behind(SIDE_PLAN_FORK), aux2 = pos.behind(POS_PLAN_FORK);
        if (!c.csr_checked) launch_csr_index_checks(m, n, c.train_p, c.train_i, c.nnz_train, c.test_p, c.test_i, c.nnz_test, plan, aux);
        side.mark(SIDE_CHECKS_DONE);
        if (!c.scores) launch_absmax<T>(c.f_type, c.A, c.lda, (long long)m, k, 512, aux2, &plan->amax_a, &plan->nonfinite);
        if (!items_known && !c.scores) launch_absmax<T>(c.f_type, c.B, c.ldb, (long long)n, k, 1024, aux2, &plan->amax_b, &plan->nonfinite_b);
        pos.mark(POS_MAXIMA_DONE);
        if (attempt != 0) return;                                      // (the second plan makes neither again)
        // (the user of every test entry, for the positives' scores by entry: index pointers only)
        if (flat_early) hipLaunchKernelGGL(k_entry_users, dim3(cdiv(cdiv(m, WAVE) * WAVE, 256)), dim3(256), 0, pos.on(), m, c.test_p, ent_user, plan);
        // (463 MB of writes at BASELINE C2; four resident blocks per CU leave half of the wave slots to the plan's kernels and the
        // read-back's copy.  With the positives' scores by entry the kernel also says which test items are train items, `ent_masked`:
        // a bit of the row it has just built.)
        if (std::is_same<T, float>::value && use_side && !c.ext_bits && dense_ok) {
            SweepArgs probe{};
            const bool guess = want_auc && !ext_topk && !g_sw.no_test_mask;
            (void)ws.get(WS_TRAIN_BITS, (size_t)m * (size_t)dense_row_words(n) * 4);
            if (!(c.same_train_rows && cx.dense.fits(ws, m, dense_row_words(n), guess))) {
                set_train_bits(probe, cx, c, m, n, dense_ok, side.on(), guess, false, false, flat_early ? ent_masked : nullptr);
                side.mark(SIDE_ROWS_AND_PACKS); side.mark(SIDE_ROWS_FOR_POS);
                bits_early = true; bits_early_masked = guess; masked_from_bits = flat_early;
            }
        }
    }
    // ---- the read-back's copy, behind the verdicts and the maxima of the two streams beside; behind the copy the scores by entry ----
    // The scores of the test entries (k_pos_scores_flat) depend on the inputs and on the users' flags alone: they run on the
    // positives' stream beside the read-back and the host's work behind it.  They index the item factors by the test items, so
    // they follow the index checks (and return when those found a defect) -- and they follow the plan's last kernel and the
    // copy: their blocks take every wave slot they find, and a plan kernel's block of 1,024 threads then waits for sixteen
    // slots of one CU to fall free at once (measured: the read-back 0.2 ms late).  Without dense train rows k_test_masked says
    // which test items are train items, behind the scores.
    void enqueue_read_back(int attempt)
    {
        side.await(SIDE_CHECKS_DONE, stream); pos.await(POS_MAXIMA_DONE, stream);
        HIP_CHECK(hipMemcpyAsync(cx.pinned_plan, plan, sizeof(Plan), hipMemcpyDeviceToHost, stream));
        if (attempt == 0 && flat_early) launch_entry_scores(pos.fork(POS_SCORES_AFTER_COPY), masked_from_bits ? MASKED_BY_ROWS : MASKED_BY_KERNEL);
    }
    // The positives' scores by entry on `sc`, the last thing the positives' stream is given in the plan stage (POS_SCORES_DONE).  Which
    // test items are train items (`ent_masked`) is KEPT from the pass that planned the split, a bit of the dense train rows' kernel
    // beside the chain, or k_test_masked's answer.
    enum EntryMasked { MASKED_KEPT, MASKED_BY_ROWS, MASKED_BY_KERNEL };
    void launch_entry_scores(hipStream_t sc, EntryMasked from)
    {
        auto test_masked = [&] { hipLaunchKernelGGL(k_test_masked, dim3(cdiv(m, TM_USERS)), dim3(256), 0, sc, m, c.test_p, c.test_i, c.train_p, c.train_i, ent_user, ent_masked, plan); };
        if (c.scores) {
            // (the caller's scores: which test items are train items first -- S is never read at a train item --, then the gather)
            test_masked();
            with_score_src<T>(c.s_type, [&](auto *src) {
                typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
                hipLaunchKernelGGL((k_pos_scores_given<T, Src>), dim3(cdiv(c.nnz_test, 256)), dim3(256), 0, sc, pa, (const Src *)c.S, c.lds, (const int *)ent_user, (const unsigned char *)ent_masked);
            });
        } else {
            with_factor_src<T>(c.f_type, [&](auto *src) {
                typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
                hipLaunchKernelGGL((k_pos_scores_flat<T, Src>), dim3(cdiv(c.nnz_test, POSF_WAVES * WAVE)), dim3(POSF_WAVES * WAVE), 0, sc, pa, (const int *)ent_user);
            });
            // test items that are train items: +inf, once the answer (the dense train rows' kernel, or k_test_masked) is there
            if (from == MASKED_BY_ROWS) side.await(SIDE_ROWS_FOR_POS, sc);
            else if (from == MASKED_BY_KERNEL) test_masked();
            hipLaunchKernelGGL(k_pos_apply_masked<T>, dim3(cdiv(c.nnz_test, 256)), dim3(256), 0, sc, pa, ent_masked);
        }
        pos.mark(POS_SCORES_DONE);
    }
    bool plan_again(int attempt)            // the host's wait, the checks' verdicts, and whether the call has to be planned once more
    {
        RM_TRACE_POINT("run: plan chain + side kernels enqueued");
        HIP_CHECK(hipStreamSynchronize(stream));
        RM_TRACE_POINT("run: plan read back");
        hp = *cx.pinned_plan;
        throw_csr_defects(hp, c, cx);
        // the streamed users' score rows must fit the budget; if not (memory pressure), plan again with those users in chunks
        if (!(ca.allow_stream && !ca.force_stream && hp.class_count[STREAM_CLASS] > stream_cap && attempt == 0)) return false;
        ca.allow_stream = 0; ca.check_ptr = 0; keepable = false;     // (a second plan is never kept)
        // (attempt 0's kernels on BOTH side streams read `flags` and `plan`, which the second plan rewrites: wait for them)
        side.sync(); pos.sync();
        return true;
    }
    // |any partial sum| <= k * max|A| * max|B|: if that is comfortably finite in T, no score is NaN / Inf
    bool scores_may_overflow()
    {
        if (items_known) { hp.amax_b = cx.packed.amax_b; hp.nonfinite_b = cx.packed.nonfinite_b; }
        else { cx.packed.amax_b = hp.amax_b; cx.packed.nonfinite_b = hp.nonfinite_b; }
        double amax_a, amax_b;
        std::memcpy(&amax_a, &hp.amax_a, 8); std::memcpy(&amax_b, &hp.amax_b, 8);
        const double tmax = std::is_same<T, float>::value ? 3.0e38 : 1.0e308;
        if (c.scores) return false;                                    // (k_score_rows looks at every candidate score whatever it is)
        return hp.nonfinite || hp.nonfinite_b || !((double)k * amax_a * 1.001 < tmax / std::max(amax_b, 1e-300));
    }

    // ---- the split the context kept (SplitCache) ----
    // Which calls keep and reuse: plain metric calls by device pointers over all their users.  The passes of the tie noise, the
    // batches of a host-pointer call, lists and score matrices plan for themselves (and void the record).
    bool make_split_key(SplitKey &key) const
    {
        std::memset(&key, 0, sizeof(SplitKey));
        if (g_sw.no_split_cache || !use_side || c.reco || c.scores || !c.plain() || c.items_tag != 0 || !c.test_p || m <= 0) return false;
        const long long words[SPLIT_ARRAYS] = {(long long)m + 1, std::max<long long>(c.nnz_train, 0), (long long)m + 1, std::max<long long>(c.nnz_test, 0),
                                               c.test_v ? std::max<long long>(c.nnz_test, 0) * (long long)(sizeof(T) / 4) : 0};
        long long total = 0;
        for (int i = 0; i < SPLIT_ARRAYS; i++) { key.arr[i] = theirs[i]; key.words[i] = words[i]; total += words[i]; }
        if (total * 4 > ((g_sw.split_cache_mb >= 0 ? g_sw.split_cache_mb : SPLIT_CACHE_DEFAULT_MB) << 20)) return false;
        key.nnz_train = c.nnz_train; key.nnz_test = c.nnz_test;
        key.m = m; key.n = n; key.k = k; key.K = K; key.elem = (int)sizeof(T); key.req = req;
        key.min_items_pool = min_items_pool; key.min_pos_test = min_pos_test; key.heavy_npos = ca.heavy_npos; key.ng = NG;
        key.cold = c.cold; key.cumulative = c.cumulative; key.want_lane = want_lane; key.ext_topk = ext_topk;
        key.allow_stream = ca.allow_stream; key.force_stream = ca.force_stream; key.dense_ok = dense_ok; key.flat_early = flat_early;
        key.csr_checked = c.csr_checked; key.rank_out = (c.topk_idx ? 1 : 0) | (c.pos_rank ? 2 : 0) | (c.status ? 4 : 0);
        key.switches = g_sw.epoch;
        return true;
    }
    // The plan stage of a pass on the kept split.  On the side stream k_split_same, the maxima and the read-back of the call's words
    // of the Plan (SIDE_VERDICT: the host's one wait, verdict()); on the positives' stream, at once, the scores of the test entries.
    // Every kernel of this pass reads the copies, so none of them waits for k_split_same.
    void plan_reused()
    {
        const SplitCache &kept = cx.split;
        const size_t at = offsetof(Plan, split_differs);
        HIP_CHECK(hipMemsetAsync((char *)plan + at, 0, offsetof(Plan, csr_bad) - at, stream));
        // (the comparison first: the host waits for it, and the blocks of the positives' scores take every wave slot they find)
        const hipStream_t aux = side.fork(SIDE_PLAN_FORK);
        SplitSameArgs ss{};
        long long longest = 1;
        for (int i = 0; i < SPLIT_ARRAYS; i++) {
            ss.theirs[i] = (const unsigned *)theirs[i]; ss.ours[i] = (const unsigned *)kept.copy(ws, i); ss.words[i] = kept.key.words[i];
            longest = std::max(longest, ss.words[i]);
        }
        ss.plan = plan;
        const unsigned blocks = (unsigned)std::min<long long>(SPLIT_SAME_BLOCKS, cdiv(cdiv(longest, 4), SPLIT_SAME_THREADS));
        hipLaunchKernelGGL(k_split_same, dim3(blocks), dim3(SPLIT_SAME_THREADS), 0, aux, ss);
        launch_absmax<T>(c.f_type, c.A, c.lda, (long long)m, k, 512, aux, &plan->amax_a, &plan->nonfinite);
        launch_absmax<T>(c.f_type, c.B, c.ldb, (long long)n, k, 1024, aux, &plan->amax_b, &plan->nonfinite_b);
        HIP_CHECK(hipMemcpyAsync(cx.pinned_plan, plan, sizeof(Plan), hipMemcpyDeviceToHost, aux));
        side.mark(SIDE_VERDICT);
        if (flat_early) launch_entry_scores(pos.fork(POS_PLAN_FORK), MASKED_KEPT);
        hints = hints && kept.hp.n_slots > 0;
        if (hints) {
            // (the kernel's two counters, zeroed here where the call's stream is idle; the launch itself follows the verdict: sweep())
            try { hint_counts_dev = ws.array<int>(WS_HINT_COUNTS, 2); } catch (const RmError &) { hints = false; }
            if (hints && !cx.hint_counts) { HIP_CHECK(hipHostMalloc((void **)&cx.hint_counts, 64, hipHostMallocDefault)); cx.hint_counts[0] = cx.hint_counts[1] = 0; }
            if (hints) HIP_CHECK(hipMemsetAsync(hint_counts_dev, 0, 2 * sizeof(int), stream));
        }
        check_launch(hipGetLastError());
        hp = kept.hp; check_nan = kept.check_nan;
        bits_early = dense_ok; bits_early_masked = kept.dense_masked; masked_from_bits = true;
        RM_TRACE_POINT("run: kept split, comparison + positives enqueued");
    }
    // The bounds the previous pass's lists give this one (k_hint_bounds, rm_prep.hpp): on the call's stream behind the preparation --
    // k_seed_thresholds has written thr_shared, the kernel raises it -- and in front of the sweep, in the sweep's stage of the timings: the
    // positives' chain, which fills the device until then, is left alone.  The finalisation, which overwrites the lists the kernel
    // reads, follows on the same stream.
    // Behind verdict(): the host has waited for this pass's comparison, which the stream runs behind the whole pass before -- that pass's
    // counts have landed, and SplitCache::hints_due says whether its advice was worth repeating.
    void launch_hints()
    {
        if (!cx.split.hints_due(cx.hint_counts)) { hints = false; return; }
        const int users_per_wave = K <= WAVE ? WAVE / K : 1;
        const long long waves = cdiv(m, users_per_wave);
        HintArgs<T, ThrT> ha{m, n, k, K, c.A, c.lda, c.B, c.ldb, c.train_p, c.train_i, flags, user_nslots, uslot_base, slot_index,
                             (const Entry<T> *)merged, thr_shared, hint_counts_dev};
        with_factor_src<T>(c.f_type, [&](auto *src) {
            typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
            hipLaunchKernelGGL((k_hint_bounds<T, ThrT, Src>), dim3(cdiv(waves, HINT_WAVES)), dim3(HINT_WAVES * WAVE), 0, stream, ha);
        });
        cx.split.hint_judge = true; cx.hints_ran = true;
    }
    // The host's wait of a pass on the kept split, in front of the sweep's launch (the device is busy with the positives' chain):
    // are the caller's arrays the kept ones, and does the sweep variant that was prepared fit this call's factors?  If not, the pass is
    // abandoned -- the host waits for what was enqueued, the record is void -- and run() plans the call from its own arrays.
    bool verdict()
    {
        side.host_wait(SIDE_VERDICT);
        RM_TRACE_POINT("run: verdict read back");
        const Plan &rb = *cx.pinned_plan;
        hp.amax_a = rb.amax_a; hp.amax_b = rb.amax_b; hp.nonfinite = rb.nonfinite; hp.nonfinite_b = rb.nonfinite_b;
        if (!rb.split_differs && scores_may_overflow() == check_nan) { cx.split_reused = 1; return true; }
        side.sync(); pos.sync();
        HIP_CHECK(hipStreamSynchronize(stream));
        cx.split.invalidate(); cx.dense.invalidate(); cx.packed.invalidate();
        cx.split_reused = 0;
        return false;
    }
    // A pass that planned for itself leaves its split to the next call: the copies are made on the side stream beside the sweep,
    // export_ranks() joins them and declares the record valid.
    void keep_split()
    {
        if (!keepable || reused) return;
        SplitCache &kept = cx.split;
        void *dst[SPLIT_ARRAYS] = {};
        try { for (int i = 0; i < SPLIT_ARRAYS; i++) if (split_key.words[i] > 0) dst[i] = ws.get(SplitCache::copies[i], (size_t)split_key.words[i] * 4); }
        catch (const RmError &) { keepable = false; return; }          // (no memory for the copies: nothing is kept)
        const hipStream_t st = side.on();
        for (int i = 0; i < SPLIT_ARRAYS; i++)
            if (dst[i]) HIP_CHECK(hipMemcpyAsync(dst[i], split_key.arr[i], (size_t)split_key.words[i] * 4, hipMemcpyDeviceToDevice, st));
        side.mark(SIDE_SPLIT_KEPT);
        std::memcpy(&kept.key, &split_key, sizeof(SplitKey));
        kept.hp = hp; kept.check_nan = check_nan; kept.dense_masked = dense_ok && cx.dense.masked;
        kept.stamps.clear();
        for (WsBuf id : {WS_FLAGS, WS_USER_NSLOTS, WS_USLOT_BASE, WS_PLAN, WS_HEAVY_USERS, WS_SLOT_USER, WS_SLOT_CHUNK, WS_SLOT_INDEX, WS_SLOT_J, WS_GJ, WS_GROW, WS_SC_USER, WS_SC_CHUNK})
            kept.keep(ws, id);
        if (flat_early) { kept.keep(ws, WS_ENT_USER); kept.keep(ws, WS_ENT_MASKED); }
        if (dense_ok) kept.keep(ws, WS_TRAIN_BITS);
        if (fa.heavy_topv) { kept.keep(ws, WS_HEAVY_TOPV); kept.keep(ws, WS_HEAVY_NAN); }
        for (int i = 0; i < SPLIT_ARRAYS; i++) if (dst[i]) kept.keep(ws, SplitCache::copies[i]);
    }

    // ideal-DCG values of the users with very long test rows (k_top_values: a wavefront per such user, a chain of K dependent
    // rounds -- latency, 0.16 ms at BASELINE C2): they depend on the test rows alone, so they are computed on the side stream
    // beside the preparation kernels instead of between the sweep and k_finalize, which waits for them
    // (launched BEHIND the operand packing on the side stream, which the sweep waits for: with k_metrics > 64 every row of more than
    // 64 test items is listed and the kernel is half a millisecond at BASELINE C2's shape)
    void launch_top_values()
    {
        if (!(fa.ndcg && hp.n_heavy > 0)) return;
        // (min(K, longest test row) values per user: with a cap of 256 the rows beyond it fell back to k_finalize's repeated selection on
        // one thread -- L x positives dependent loads: 160 of the 190 ms of a K = 300 step at BASELINE C2's shape)
        fa.heavy_ld = std::max(1, std::min(K, hp.max_npos));
        fa.heavy_topv = ws.array<T>(WS_HEAVY_TOPV, (size_t)m * (size_t)fa.heavy_ld);
        fa.heavy_nan = ws.array<unsigned char>(WS_HEAVY_NAN, (size_t)m);
        fa.heavy_users = heavy_users; fa.n_heavy = hp.n_heavy;
        if (reused) return;                                          // (the values depend on the test rows and k_metrics alone: kept)
        hipLaunchKernelGGL((k_top_values<T, T>), dim3(cdiv((long long)hp.n_heavy * WAVE, 256)), dim3(256), 0, side.fork(SIDE_FORK), fa);
        side.mark(SIDE_TOP_VALUES);
    }

    // ---- prep: the finalisation's arguments, operand packing, dense train rows, positives tables, seeds ----
    void prep()
    {
        // (recommendation lists: only k_collect_topk / k_select_topk go through `merged`; the lists in parts are merged into the caller's arrays)
        if (!c.reco || want_lane || ext_topk) merged = ws.array<Entry<T>>(WS_MERGED, (size_t)m * K);
        if (c.pos_rank) rank_sorted = ws.array<long long>(WS_RANK_SORTED, (size_t)std::max<long long>(c.nnz_test, 1));
        if (rank_sorted) HIP_CHECK(hipMemsetAsync(rank_sorted, 0, sizeof(long long) * (size_t)std::max<long long>(c.nnz_test, 1), stream));
        // the argument block of the finalisation kernels is filled in as the pieces come into being
        fa.m = m; fa.n = n; fa.K = K; fa.req = req; fa.cumulative = c.cumulative ? 1 : 0; fa.noise = c.noise ? 1 : 0; fa.gu = GU;
        fa.train_p = c.train_p; fa.test_p = c.test_p; fa.test_i = c.test_i; fa.test_v = c.test_v;
        fa.flags = flags; fa.user_nslots = user_nslots; fa.uslot_base = uslot_base; fa.slot_index = slot_index;
        fa.gj = gj; fa.grow = grow; fa.log2tab = log2tab;
        fa.p = c.out[0]; fa.tp = c.out[1]; fa.r = c.out[2]; fa.ap = c.out[3]; fa.tap = c.out[4];
        fa.ndcg = c.out[5]; fa.hit = c.out[6]; fa.rr = c.out[7]; fa.roc = c.out[8]; fa.pr = c.out[9];
        fa.merged = merged; fa.rank_sorted = rank_sorted; fa.status = c.status;
        fa.noise_flag = c.noise_flag; fa.plan = plan;
        fa.n_slots = n_slots; fa.slot_user = slot_user; fa.slot_chunk = slot_chunk;
        fa.stream_slot0 = stream_slot0;
        if (want_auc && n_slots > 0) fa.auc_part = ws.array<AucPart>(WS_AUC_PART, (size_t)n_slots);
        fa.heavy_npos = ca.heavy_npos;
        stream_ld = (long long)g.tiles_total * g.tile_items;
        if (n_slots == 0) return;
        if (c.scores) {
            // the caller's scores: nothing is packed, sampled or seeded and there are no dense train rows or lists -- what is left of
            // the preparation is the ideal-DCG values, the positives' tables and the two buffers k_score_rows fills
            launch_top_values();
            if (want_auc) positives();
            stream_scores = ws.array<T>(WS_STREAM_SCORES, (size_t)std::max(n_stream, 1) * (size_t)stream_ld);
            pst = ws.array<PartialStat<T>>(WS_PST, (size_t)n_slots * g.n_part);
            RM_TRACE_POINT("run: preparation enqueued");
            return;
        }
        const int n_groups = hp.n_groups, tiles_total = g.tiles_total, tile_items = g.tile_items;

        // ---- pack operands into the MFMA images ----
        const long long bp_units = P::items_units(tiles_total, NG, tile_items), ap_units = P::users_units(n_groups, NG);
        typename P::PackT *Bp = (typename P::PackT *)ws.get(WS_BP, 16 * (size_t)bp_units);
        typename P::PackT *Ap = (typename P::PackT *)ws.get(WS_AP, 16 * (size_t)ap_units);
        // the packed item image survives between the batches of one host call (same B, same geometry)
        const bool items_packed = cx.packed.holds(ws, c.items_tag, tile_items, NG);
        // Only the sweep reads the packed images: with a side stream they are made there, behind the dense train rows and beside the
        // positives' kernels (120 us of BASELINE C2's preparation that sat in front of k_pos_scores); the sweep's launch waits for both.
        const bool packs_side = use_side && want_auc && cx.side_stream != nullptr;
        pack_call_operands<T>(c, n, NG, tile_items, slot_user, n_slots, Ap, ap_units, Bp, bp_units, packs_side ? side.on() : stream, !items_packed);
        if (packs_side) side.mark(SIDE_ROWS_AND_PACKS);                 // (behind the rows, when they were launched: the sweep waits for both)
        cx.packed.set(ws, c.items_tag, tile_items, NG);
        launch_top_values();

        // ---- dense train rows (fp32, small item counts) ----
        // (measured: on the side stream beside the positives' kernels they gain nothing -- both are bound by memory; r3_ab_c2.txt)
        // (rows launched beside the plan read-back that turn out not to be the ones wanted -- a wrong guess of `mask_test`, rows handed over
        // by another pass -- are waited for here, before anything is launched over them; the usual case waits in front of the sweep)
        if (bits_early && (bits_early_masked != g.mask_test || (g.use_ext_bits && dense_ok))) side.await(SIDE_ROWS_AND_PACKS, stream);
        if (g.use_ext_bits && dense_ok) set_ext_bits(sa, c.ext_bits, (int)c.ext_words);
        else set_train_bits(sa, cx, c, m, n, dense_ok, stream, g.mask_test, bits_early, bits_early_masked);

        if (want_auc) positives();

        if (n_stream > 0) stream_scores = ws.array<T>(WS_STREAM_SCORES, (size_t)n_stream * (size_t)stream_ld);
        if (!ext_topk) pl = ws.array<Entry<T>>(WS_PL, (size_t)n_slots * g.n_part * K);
        pst = ws.array<PartialStat<T>>(WS_PST, (size_t)n_slots * g.n_part);
        const unsigned n_blocks = sweep_blocks(g.n_ublocks, g.tail_ublocks, g);
        lane_lists = want_lane && !ext_topk;                     // per-lane append buffers + k_collect_topk (rm_list.hpp)
        int lane_cap = lane_lists ? P::lane_cap(K) : 0;
        if (lane_lists && g_sw.lane_cap_set > 0) lane_cap = (int)std::min<long long>(std::max<long long>(P::lane_cap(K), (g_sw.lane_cap_set + 15) / 16 * 16), (COLLECT_MAX_ENTRIES - K) / 16 * 16);
        if (lane_lists && g_sw.lane_cap_min >= 0)        // K + slack survivors and one tile's appends (16: both precisions' bound) in one lane
            lane_cap = std::min(lane_cap, (K + lane_sel_slack(K) + 16 + 1 + 15) / 16 * 16);
        if (lane_lists) {
            glists = (typename P::ListT *)ws.get(WS_GLISTS, (size_t)n_blocks * g.n_waves * WAVE * (size_t)lane_cap * (sizeof(T) + 4));
            lane_cnt = ws.array<int>(WS_LANE_CNT, (size_t)n_blocks * g.n_waves * WAVE);
        } else if (!g.list_in_lds && !ext_topk) {
            glists = ws.array<typename P::ListT>(WS_GLISTS, (size_t)n_blocks * g.n_waves * GU * (2 * K + 32));
        }

        thr_shared = ws.array<ThrT>(WS_THR_SHARED, (size_t)n_slots);
        if (want_auc && !ext_topk && !g_sw.no_seed)
            hipLaunchKernelGGL((k_seed_thresholds<T, ThrT>), dim3(cdiv(n_slots, 256)), dim3(256), 0, stream, n_slots, stream_slot0, K, GU, slot_user, slot_chunk,
                               user_nslots, flags, c.test_p, grow, pos_score, spos_score, thr_shared);
        else HIP_CHECK(hipMemsetAsync(thr_shared, 0, sizeof(ThrT) * (size_t)n_slots, stream));
        sa.thr_shared = thr_shared;
        sa.n = n; sa.K = K; sa.ngt = NG; sa.n_slots = n_slots; sa.n_groups = n_groups; sa.n_ublocks = g.n_ublocks;
        sa.n_splits = g.n_splits; sa.tail_ublocks = g.tail_ublocks; sa.tail_splits = g.tail_splits; sa.part_splits = g.part_splits; sa.tiles_total = tiles_total; sa.jmax = g.jmax; sa.check_nan = check_nan ? 1 : 0; sa.buffered_lists = (want_lane || ext_topk) ? 1 : 0; sa.ext_topk = ext_topk ? 1 : 0;
        sa.Ap = (decltype(sa.Ap))Ap; sa.Bp = (decltype(sa.Bp))Bp; sa.slot_user = slot_user; sa.slot_chunk = slot_chunk;
        sa.train_p = c.train_p; sa.train_i = c.train_i; sa.gj = gj; sa.grow = grow;
        sa.pos_score = pos_score; sa.pos_item = pos_item; sa.hist = hist; sa.glists = glists; sa.lane_cap = lane_cap; sa.lane_cnt = lane_cnt; sa.pl = pl; sa.pst = pst; sa.dump = nullptr;
        sa.pend_cap = g.pend_cap;  sa.pend_off = 0;
        sa.sync_off = (int)g.sync_off;
        sa.stream_slot0 = stream_slot0; sa.stream_ld = stream_ld; sa.stream_scores = stream_scores;
        set_part_extra(sa, g.part_extra);
        sa.noise_row = c.noise_row; sa.noise_row0 = c.noise_row0; sa.noise_E = c.noise_E; sa.noise_ld = c.noise_ld;
        set_spec(sa);

        // the dense train rows, launched beside the plan read-back: the sweep reads them, and so do the passes that start at
        // `flags_event` (their noise rows, their own sweeps) -- nothing in front of this point does
        if (side.marked(SIDE_ROWS_AND_PACKS)) side.await(SIDE_ROWS_AND_PACKS, stream);
        // Sample seeds (k_seed_from_sample, rm_prep.hpp): the sweep's DUMP variant scores the first S items for every slot, a
        // wavefront per slot takes the K-th best candidate of them, and the lane buffers start with a pass rate of K / S.
        const bool sample_lists = !lane_lists && !ext_topk && sizeof(T) == 4;      // (the LDS / HBM lists: seeded as well, from a smaller sample)
        const int sample_S = (lane_lists || sample_lists) ? sample_seed_items<T>(ws, K, n, n_slots, check_nan || c.noise_E != nullptr, sample_lists) : 0;
        if (sample_S > 0 && !sample_lists) seed_from_sample<T>(sa, ws, sample_S, NG, n_slots, g.n_ublocks, stream);
        else if (sample_S > 0) {
            const long long units = P::items_units(sample_S / TILE_ITEMS, NG);
            typename P::PackT *Bs = (typename P::PackT *)ws.get(WS_SAMPLE_ITEMS, 16 * (size_t)units);
            void *Ls = ws.array<typename P::ListT>(WS_SAMPLE_LISTS, (size_t)g.n_ublocks * 8 * GU * (2 + 32));
            pack_call_operands<T>(c, sample_S, NG, TILE_ITEMS, slot_user, 0, Ap, 0, Bs, units, stream, true);
            seed_from_sample<T>(sa, ws, sample_S, NG, n_slots, g.n_ublocks, stream, Bs, Ls);
        }
        RM_TRACE_POINT("run: preparation enqueued");
    }

    // the positives' tables: scores of the test items, their ranks among themselves, placed per group (prep)
    void positives()
    {
        const int n_groups = hp.n_groups;
        const long long rows = hp.total_rows + n_groups;       // 2^j rows per group (one +inf pad row each)
        pos_score = ws.array<T>(WS_POS_SCORE, (size_t)(rows + 1) * GU);
        pos_item = ws.array<int>(WS_POS_ITEM, (size_t)(rows + 1) * GU);
        hist = ws.array<unsigned>(WS_HIST, (size_t)(rows + 1) * GU);
        if (!flat_early) fill_pos_args();                      // (the scores by slot: nothing has asked for the arguments yet)
        pos_order = ws.array<int>(WS_POS_ORDER, (size_t)std::max<long long>(c.nnz_test, 1));
        pa.user_nslots = user_nslots; pa.uslot_base = uslot_base; pa.slot_index = slot_index; pa.grow = grow;
        pa.pos_order = pos_order; pa.pos_score = pos_score; pa.pos_item = pos_item; pa.gu = GU;
        // Scores of the test entries: by entry (k_pos_scores_flat, launched beside the plan chain: every lane busy) unless the call
        // evaluates a few of its users only -- then a wavefront per slot is less work.
        const bool flat = flat_early;
        // The streamed users' positives (the all-pairs rank of long test rows: vector work) run on a stream of their own beside
        // the table users'
        // (not the side stream: that one carries the dense train rows and the operand packing, 0.3 ms the streamed users' chain
        // used to queue behind.  The host has waited for the call's stream since: nothing to wait for over there.)
        const bool pos_beside = use_side && n_stream > 0 && stream_slot0 > 0 && !g_sw.no_pos_beside;
        hipStream_t ps = pos_beside ? pos.on() : stream;
        PosArgs<T> pb = pa;
        // (with the scores by entry the positives' stream is busy with them: the tables are filled on the call's stream meanwhile)
        const hipStream_t fill = (flat && pos_beside) ? stream : ps;
        if (n_stream > 0) {
            const size_t nz = (size_t)std::max<long long>(c.nnz_test, 1);
            spos_score = ws.array<T>(WS_SPOS_SCORE, nz);
            spos_item = ws.array<int>(WS_SPOS_ITEM, nz);
            shist = ws.array<unsigned>(WS_SHIST, nz);
            pb.stream = 1; pb.spos_score = spos_score; pb.spos_item = spos_item;
            // (+inf in every rank: entries that repeat an item -- a non-canonical CSR row -- share a rank and leave one unused)
            hipLaunchKernelGGL(k_init_tables<T>, dim3(cdiv((long long)nz, 256)), dim3(256), 0, fill, spos_score, shist, (long long)nz);
        }
        const int nsc = hp.n_stream_chunks;
        hipLaunchKernelGGL(k_init_tables<T>, dim3(cdiv(rows * GU, 256)), dim3(256), 0, stream, pos_score, hist, rows * GU);
        if (flat) {
            if (pos_beside) ps = pos.fork(POS_TABLES_INIT);
            // (the scores are the last thing on the positives' stream: whoever is not on it waits for them)
            pos.await(POS_SCORES_DONE, stream);
        } else {
            with_factor_src<T>(c.f_type, [&](auto *src) {
                typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
                if (n_stream > 0) hipLaunchKernelGGL((k_pos_scores<T, Src>), dim3(cdiv(nsc, POSS_WAVES)), dim3(POSS_WAVES * WAVE), 0, ps, pb, (const int *)sc_user, (const int *)sc_chunk, nsc);
                if (stream_slot0 > 0) hipLaunchKernelGGL((k_pos_scores<T, Src>), dim3(cdiv(stream_slot0, POSS_WAVES)), dim3(POSS_WAVES * WAVE), 0, stream, pa, (const int *)slot_user, (const int *)slot_chunk, stream_slot0);
            });
        }
        if (n_stream > 0) hipLaunchKernelGGL(k_pos_place<T>, dim3(cdiv((long long)nsc * WAVE, 256)), dim3(256), 0, ps, pb, sc_user, sc_chunk, nsc);
        if (stream_slot0 > 0) hipLaunchKernelGGL(k_pos_place<T>, dim3(cdiv((long long)stream_slot0 * WAVE, 256)), dim3(256), 0, stream, pa, slot_user, slot_chunk, stream_slot0);
        if (pos_beside) pos.join(POS_STREAMED_PLACED);
    }

    // ---- sweep: the flags for the tie noise's exact pass, then the sweep launch (two with a depth split) ----
    void sweep()
    {
        if (c.flag_snapshot) {
            if (n_slots > 0) {
                HIP_CHECK(hipMemcpyAsync(c.flag_snapshot, c.noise_flag, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, stream));
                HIP_CHECK(hipMemcpyAsync(c.flag_count_host, &plan->n_noise_flagged, sizeof(int), hipMemcpyDeviceToHost, stream));
            } else {                                                 // (no user to evaluate: nothing is flagged)
                HIP_CHECK(hipMemsetAsync(c.flag_snapshot, 0, sizeof(int) * (size_t)m, stream));
                *c.flag_count_host = 0;
            }
            HIP_CHECK(hipEventRecord(c.flags_event, stream));
        }
        HIP_CHECK(hipEventRecord(cx.ev[EV_PREP_END], stream));
        if (n_slots == 0) {
            HIP_CHECK(hipEventRecord(cx.ev[EV_SWEEP_END], stream));
            cx.sweep_shape(0, 0, 0, 0, -1);
            return;
        }
        if (c.scores) {
            // the caller's scores: k_score_rows in the sweep's place -- a block per user copies the user's row of S into its masked
            // score row and leaves the candidates' statistics (rm_scores.hpp); the "sweep" timing brackets this launch
            if (n_stream > 0) with_score_src<T>(c.s_type, [&](auto *src) {
                typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
                ScoreRowArgs<T, Src> ra{n, n_stream, stream_slot0, g.n_part, slot_user, c.train_p, c.train_i, (const Src *)c.S, c.lds, stream_scores, stream_ld, pst};
                hipLaunchKernelGGL((k_score_rows<T, Src>), dim3((unsigned)n_stream), dim3(SCORE_ROW_THREADS), 0, stream, ra);
            });
            check_launch(hipGetLastError());
            RM_TRACE_POINT("run: score rows enqueued");
            HIP_CHECK(hipEventRecord(cx.ev[EV_SWEEP_END], stream));
            cx.sweep_shape(1, 1, n_stream, 0, n_slots);
            return;
        }
        const unsigned n_blocks = sweep_blocks(g.n_ublocks, g.tail_ublocks, g);
        if (hints && merged && thr_shared) launch_hints();
        if (g.u_split > 0) {
            // Depth split: the two launches run side by side on two streams so that neither pays a partially filled last round of its own.
            const int u_split = g.u_split, n_ublocks = g.n_ublocks;
            side.enabled = true;                                   // (the second launch runs beside the first whatever RM_DEBUG_NO_SIDE says)
            typename P::Args sb = sa;                              // the deep blocks: lists in HBM, as computed above
            sb.ublock0 = u_split;  sb.n_ublocks = n_ublocks - u_split;
            typename P::Args sl = sa;                              // the shallow blocks: lists in LDS
            sl.ublock0 = 0;  sl.n_ublocks = u_split;
            // (the tail of the two-level grid = the cheapest user blocks = the first ones: the shallow launch's, then the deep one's)
            sl.tail_ublocks = std::min(g.tail_ublocks, u_split);
            sb.tail_ublocks = g.tail_ublocks - sl.tail_ublocks;
            sl.pend_cap = g.pend_cap;  sl.pend_off = 0;
            sl.sync_off = (int)(g.lds_l - SYNC_BYTES);
            dispatch_sweep(want_auc, false, false, g.nsub, NG, dim3(sweep_blocks(sb.n_ublocks, sb.tail_ublocks, g)), g.lds_total, side.fork(SIDE_SWEEP_FORK), sb);
            side.mark(SIDE_SWEEP_DEEP_DONE);
            dispatch_sweep(want_auc, false, true, g.nsub, NG, dim3(sweep_blocks(sl.n_ublocks, sl.tail_ublocks, g)), g.lds_l, stream, sl);
            side.await(SIDE_SWEEP_DEEP_DONE, stream);
            side.enabled = use_side;
        } else {
            // (Measured and dropped: the blocks made of streamed users only as a second launch of the sweep variant without rank
            // counting on a side stream, followed there by k_rank_streamed, beside the main launch.  At C2 the step time did
            // not move -- 11.61 vs 11.59 ms -- and at the north-star shape, where one launch is exactly one round of 256
            // blocks, the side launch ran AFTER the main one instead of beside it: 61 ms of tail.  gpurun_out r2q.)
            dispatch_sweep(want_auc, false, g.list_in_lds, g.nsub, NG, dim3(n_blocks), g.lds_total, stream, sa);
        }
        RM_TRACE_POINT("run: sweep enqueued");
        HIP_CHECK(hipEventRecord(cx.ev[EV_SWEEP_END], stream));
        if (hints) HIP_CHECK(hipMemcpyAsync(cx.hint_counts, hint_counts_dev, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
        if (lane_lists) {
            collect = true;
            collect_g = CollectGeom{sa.ublock0, sa.n_ublocks, g.n_splits, g.tail_ublocks, g.tail_splits, g.nsub, GU, P::lanes_per_user, sa.lane_cap, g.part_extra ? g.n_part - 1 : -1};
        }
        cx.sweep_shape(g.u_split > 0 ? 2 : 1, g.n_splits, n_blocks, (double)g.lds_total, n_slots);
    }

    // ---- lists from the caller's scores (row_topk): k_topk_rows in the place of preparation, sweep and finalisation -- a block per
    // user of the call reads the user's row of S once and writes its list and status; the "sweep" timing brackets this launch ----
    void topk_rows()
    {
        HIP_CHECK(hipEventRecord(cx.ev[EV_PREP_END], stream));
        const void *kernel = nullptr;
        with_score_src<T>(c.s_type, [&](auto *src) {
            typedef std::remove_cv_t<std::remove_pointer_t<decltype(src)>> Src;
            RowTopkArgs<T, Src> ra{n, K, c.train_p, c.train_i, (const Src *)c.S, c.lds, c.topk_idx, c.topk_score, c.status};
            hipLaunchKernelGGL((k_topk_rows<T, Src>), dim3((unsigned)m), dim3(SCORE_ROW_THREADS), 0, stream, ra);
            kernel = (const void *)k_topk_rows<T, Src>;
        });
        HIP_CHECK(hipGetLastError());
        RM_TRACE_POINT("run: row top-K enqueued");
        HIP_CHECK(hipEventRecord(cx.ev[EV_SWEEP_END], stream));
        hipFuncAttributes at{};
        HIP_CHECK(hipFuncGetAttributes(&at, kernel));
        cx.sweep_shape(1, 1, m, (double)at.sharedSizeBytes, hp.n_slots);
    }

    int stream_parts() const { return (int)cdiv(n, STREAM_RANK_THREADS * STREAM_RANK_ITEMS); }
    void rank_streamed_rows(int r0, int r1, hipStream_t st)
    {
        if (r1 <= r0) return;
        const int parts = stream_parts();
        const int ipt = ((int)cdiv(n, (long long)parts * STREAM_RANK_THREADS) + 7) / 8 * 8;     // equal pieces of the row
        hipLaunchKernelGGL((k_rank_streamed<T, T>), dim3((unsigned)((long long)(r1 - r0) * parts)), dim3(STREAM_RANK_THREADS), 0, st, fa, parts, ipt, r0);
    }
    void auc_streamed_rows(int r0, int r1, hipStream_t st)
    {
        if (r1 <= r0) return;
        hipLaunchKernelGGL((k_auc_streamed<T, T>), dim3(cdiv((long long)(r1 - r0) * WAVE, 256)), dim3(256), 0, st, fa, r0, r1);
    }
    void finalize_slots(int s0, int s1, size_t fin_lds)
    {
        if (s1 <= s0) return;
        fa.fin_slot0 = s0; fa.fin_slot1 = s1;
        hipLaunchKernelGGL((k_finalize<T, T>), dim3(cdiv(s1 - s0, FIN_THREADS)), dim3(FIN_THREADS), fin_lds, stream, fa);
    }

    // the ordered top-K of every user into `merged`, where the lists did not stay in parts: out of the sweep's lane buffers
    // (k_collect_topk), or picked from the stored score rows (k_select_topk, k_metrics beyond the lists)
    void collect_lists()
    {
        if (!collect) return;
        // k_metrics beyond the LDS lists: the users' ordered top-K out of the sweep's lane buffers, straight into `merged` (behind
        // k_merge_positives, whose part of `pl` -- the streamed users' own test items -- is one of the inputs)
        fa.collected = 1;
        const char *gl = (const char *)glists;
        if (collect_capw(K, collect_g.lane_cap) == 512)
            hipLaunchKernelGGL((k_collect_topk<T, T, ThrT, 512>), dim3(collect_grid(cdiv(n_slots, 4))), dim3(256), 0, stream, fa, collect_g, gl, lane_cnt, (const ThrT *)thr_shared);
        else if (collect_capw(K, collect_g.lane_cap) == 1024)
            hipLaunchKernelGGL((k_collect_topk<T, T, ThrT, 1024>), dim3(collect_grid(cdiv(n_slots, 4))), dim3(256), 0, stream, fa, collect_g, gl, lane_cnt, (const ThrT *)thr_shared);
        else
            hipLaunchKernelGGL((k_collect_topk<T, T, ThrT, 4096>), dim3(collect_grid(n_slots)), dim3(64), 0, stream, fa, collect_g, gl, lane_cnt, (const ThrT *)thr_shared);
    }
    void select_lists()
    {
        if (!(n_slots > 0 && ext_topk)) return;
        int sel_ld = 2;
        while (sel_ld < K) sel_ld <<= 1;
        fa.ext_topk = 1; fa.sel_ld = sel_ld;
        fa.sel_hi = ws.array<unsigned long long>(WS_SEL_HI, (size_t)n_slots * sel_ld);
        fa.sel_lo = ws.array<unsigned>(WS_SEL_LO, (size_t)n_slots * sel_ld);
        hipLaunchKernelGGL((k_select_topk<T, T>), dim3(n_slots), dim3(SELECT_THREADS), 0, stream, fa);
    }

    // ---- finalize (recommendation lists): the lists and a status per user straight into the caller's arrays ----
    void finalize_reco()
    {
        fa.n_part = g.n_part; fa.pl = pl; fa.pst = pst;
        fa.stream_slot0 = stream_slot0; fa.stream_scores = stream_scores; fa.stream_ld = stream_ld;
        collect_lists();
        select_lists();
        const bool merged_ready = n_slots > 0 && (collect || ext_topk);
        RecoArgs<T> ra{m, n, K, g.n_part, flags, uslot_base, slot_index, c.train_p, pl, pst, merged_ready ? merged : nullptr,
                       c.topk_idx, c.topk_score, c.status};
        const size_t lds = reco_lds_bytes<T>(g.n_part, merged_ready);
        if (lds > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *)k_finalize_reco<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_finalize_reco<T>, dim3(cdiv(m, RECO_THREADS)), dim3(RECO_THREADS), lds, stream, ra);
        HIP_CHECK(hipGetLastError());
    }

    // ---- finalize: merge, streamed ranks and AUC, top-K collection / selection, the metrics ----
    void finalize()
    {
        fa.n_part = g.n_part; fa.pl = pl; fa.pst = pst; fa.hist = hist; fa.pos_score = pos_score; fa.pos_item_tab = pos_item;
        // the streamed users' ranks (HBM-bound: the stored score rows) run on the side stream beside the short kernels of the others
        fa.stream_slot0 = stream_slot0; fa.stream_scores = stream_scores; fa.stream_ld = stream_ld;
        fa.spos_score = spos_score; fa.spos_item = spos_item; fa.shist = shist;
        fa.rank_generic = (g_sw.rank_generic ? 1 : 0);
        const bool ranks_beside = use_side && n_slots > 0 && want_auc && n_stream > 0;
        // one block of k_rank_streamed per row (rows up to 32,768 items) with the user's table in LDS: the block also walks its counts
        // (k_auc_streamed's job); k_auc_streamed is then only launched when some row is too long for that
        bool auc_launch = true;
        if (stream_parts() == 1 && !g_sw.no_fused_auc) {
            fa.fused_auc = 1 | (g.mask_test ? 2 : 0);
            long long top = 1;
            while (top <= hp.max_npos) top <<= 1;
            // (k_metrics > 256 streams everybody without counting the long rows first: the longest one is not known then)
            auc_launch = ext_topk || !(top * (long long)(sizeof(T) / 4) + hp.max_npos + 1 <= STREAM_RANK_LDS / 4);
        }
        hipStream_t rank_stream = stream;
        if (ranks_beside) { rank_stream = side.fork(SIDE_FORK); rank_streamed_rows(0, n_stream, rank_stream); }
        if (g.mask_test) {
            // (the table users' test items were put back by the sweep, rm_sweep.hpp; the streamed users' are this kernel's)
            if (n_slots > stream_slot0)
                hipLaunchKernelGGL((k_merge_positives<T, T>), dim3(cdiv(n_slots - stream_slot0, MERGE_WAVES)), dim3(MERGE_WAVES * WAVE), 0, stream, fa, g.n_part - 1, stream_slot0);
            if (ranks_beside && auc_launch) rank_stream = side.fork(SIDE_MERGED);     // (it counts the streamed users' own test items: before k_auc_streamed)
        }
        if (ranks_beside && auc_launch) auc_streamed_rows(0, n_stream, rank_stream);
        hipLaunchKernelGGL((k_finalize_skipped<T, T>), dim3(cdiv(m, 256)), dim3(256), 0, stream, fa);
        if (side.marked(SIDE_TOP_VALUES)) side.await(SIDE_TOP_VALUES, stream);       // (k_top_values, launched beside the preparation)
        collect_lists();
        select_lists();
        if (n_slots > 0) {
            if (want_auc) {
                if (n_stream > 0 && !ranks_beside) { rank_streamed_rows(0, n_stream, stream); if (auc_launch) auc_streamed_rows(0, n_stream, stream); }
                if (stream_slot0 > 0) hipLaunchKernelGGL((k_auc_slots<T, T>), dim3(cdiv(stream_slot0, 256)), dim3(256), 0, stream, fa);
            }
            const size_t fin_lds = finalize_lds_bytes<T>(K, g.n_part);
            HIP_CHECK(hipFuncSetAttribute((const void *)k_finalize<T, T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fin_lds));
            fa.auc_defer_slot0 = n_slots;
            if (ranks_beside && (req & (RQ_ROC | RQ_PR)) && !g_sw.no_defer_auc) {
                // nothing of k_finalize but the two AUC values of the streamed users needs the side stream: it runs for everybody while
                // their ranks are still being counted there, and a short kernel fills those two in behind the join
                fa.auc_defer_slot0 = stream_slot0;
                finalize_slots(0, n_slots, fin_lds);
                side.join(SIDE_JOIN);
                hipLaunchKernelGGL((k_finalize_auc<T, T>), dim3(cdiv(n_slots - stream_slot0, 256)), dim3(256), 0, stream, fa);
            } else if (ranks_beside) {
                finalize_slots(0, stream_slot0, fin_lds);
                side.join(SIDE_JOIN);
                finalize_slots(stream_slot0, n_slots, fin_lds);
            } else finalize_slots(0, n_slots, fin_lds);
        }
        HIP_CHECK(hipGetLastError());
    }

    // ---- export: the ranking outputs of rm_rank_*, the context's events ----
    void export_ranks()
    {
        if (c.topk_idx && !c.reco)
            hipLaunchKernelGGL(k_export_rank<T>, dim3(cdiv((long long)m * K, 256)), dim3(256), 0, stream, m, K, merged, c.topk_idx, c.topk_score, flags);
        if (c.pos_rank)           // (per user, never a memset of the whole array: a batch must not clear what other batches wrote)
            hipLaunchKernelGGL(k_export_pos_rank, dim3(cdiv(m, 128)), dim3(128), 0, stream, c.nnz_test, m, c.test_p, flags, pos_order, rank_sorted, c.pos_rank,
                               (want_auc && n_slots > 0) ? 1 : 0, c.status);
        RM_TRACE_POINT("run: finalisation enqueued");
        if (side.marked(SIDE_SPLIT_KEPT)) { side.await(SIDE_SPLIT_KEPT, stream); cx.split.valid = true; }      // (keep_split's copies)
        // (`merged` now holds this pass's lists, or will when the stream gets there: the advice of the next pass on this split)
        if (keepable && cx.split.valid && merged && !c.reco && n_slots > 0) cx.split.keep_lists(ws);
        HIP_CHECK(hipEventRecord(cx.ev[EV_END], stream));
        HIP_CHECK(hipEventRecord(cx.done, stream));
        cx.ev_recorded = true;
        HIP_CHECK(hipGetLastError());
    }
};

// One pass of a call: DESIGN.md section 1, stage by stage; what runs on the context's side stream and on the positives' stream, and
// which event orders it against the call's stream, is the table at the end of that section.
template <class T>
void run(const Call<T> &c, hipStream_t stream, Ctx &cx)
{
    // (a pass on the split the context kept may find, in front of its sweep, that the caller's arrays are no longer the kept ones:
    // the second round plans the call from them, as every call did before there was anything to keep)
    for (int round = 0; round < 2; round++) {
        Pipeline<T> p(c, stream, cx);
        p.allow_reuse = round == 0;
        p.begin();
        p.plan_stage();
        if (p.row_topk) { p.topk_rows(); p.export_ranks(); return; }
        p.g = c.scores ? scores_geometry(p.hp, c.n, p.want_auc)
                       : sweep_geometry<T>(p.c, p.hp, p.NG, p.want_auc, p.want_lane, p.ext_topk, p.check_nan, p.dense_ok, g_sw);
        p.prep();
        if (p.reused && !p.verdict()) continue;
        p.sweep();
        p.keep_split();
        if (c.reco) p.finalize_reco(); else p.finalize();
        p.export_ranks();
        return;
    }
}

// ---- tie noise on top of run() (rm_noise.hpp) ---------------------------------------------------------------------------
// fp64: the noise (|e| <= 1e-12) is far above an ulp of any ordinary score, every score changes: every user is evaluated
// with its noise row, in user batches whose rows (draws + noise values, 2 x 8 n bytes per user) fit the memory budget.
// fp32: the noise only changes scores below 2^-15 in magnitude; a first pass evaluates everybody on the plain scores and
// flags the users who have such a score among their test items or their top-K -- the only ones whose ranking the noise
// can touch -- and only those are evaluated again, exactly.
std::atomic<unsigned long long> g_call_counter{1};       // tags of calls: the packed item image survives between the passes / batches of one

template <class T> struct NoiseGeom {
    int per; long long e_ld, d_ld, cap;
    NoiseGeom(const Workspace &ws, int n)
    {
        per = sizeof(T) == 4 ? 1 : 2;
        e_ld = score_row_stride(n);
        d_ld = ((long long)n * per + MT_N - 1) / MT_N * MT_N;
        const long long row_bytes = e_ld * (long long)sizeof(T) + d_ld * 4;
        long long budget;
        if (g_sw.noise_budget_mb >= 0) budget = g_sw.noise_budget_mb << 20;
        else budget = free_plus_owned(ws, {WS_NOISE_DRAWS, WS_NOISE_ROWS}) / 3;
        cap = std::max<long long>(1, std::min<long long>(budget / row_bytes, 1 << 20));
    }
};
// per-user mt19937(seed + user) draws -> per-item noise rows for `rows` users (row_user: their indices, null = users 0 .. rows - 1)
template <class T>
void noise_make_rows(Ctx &cx, const Call<T> &c0, const NoiseGeom<T> &g, const int *row_user, int rows, const int *train_p, long long user0,
                     unsigned *D, T *E, hipStream_t stream, const unsigned *own_bits = nullptr, long long own_words = 0)
{
    const int n = c0.n, m = c0.m;
    hipLaunchKernelGGL(k_mt_draws, dim3(cdiv(rows, MT_WAVES)), dim3(MT_WAVES * WAVE), 0, stream, row_user, rows, c0.seed, user0,
                       train_p, n, g.per, D, g.d_ld);
    // the dense train rows of this call's own first pass (fp32, small item counts), when they cover exactly these users
    const bool dense = row_user != nullptr && cx.dense.built_by(cx.ws, c0.items_tag, train_p, m);
    if (own_bits)                                                  // unmasked dense rows built for exactly these users (run_host_range)
        hipLaunchKernelGGL(k_noise_rows_bits<T>, dim3(rows), dim3(NOISE_ROWS_THREADS), sizeof(int) * (size_t)(2 * own_words + 1), stream, row_user, rows,
                           own_bits, (int)own_words, n, 0, train_p, c0.train_i, c0.test_p, c0.test_i, D, g.d_ld, E, g.e_ld);
    else if (dense)
        hipLaunchKernelGGL(k_noise_rows_bits<T>, dim3(rows), dim3(NOISE_ROWS_THREADS), sizeof(int) * (size_t)(2 * cx.dense.words + 1), stream, row_user, rows,
                           cx.dense.rows(cx.ws), (int)cx.dense.words, n, cx.dense.masked ? 1 : 0, train_p, c0.train_i, c0.test_p, c0.test_i,
                           D, g.d_ld, E, g.e_ld);
    else
        hipLaunchKernelGGL(k_noise_rows<T>, dim3(cdiv((long long)rows * g.e_ld, 256)), dim3(256), 0, stream, row_user, rows, train_p, c0.train_i, n,
                           D, g.d_ld, E, g.e_ld);
}

// The exact pass of the fp32 tie noise over flagged users: a row of noise for each of them, the whole pipeline again for exactly
// those users.  One driver for its two forms:
//   sequential  constructed on the call's own context and stream; sequential() evaluates the flagged users in pieces of what the
//               memory budget allows (NoiseGeom::cap);
//   beside      BESIDE a running sweep: constructed on the call's context alone and opened on its NOISE_SLOT context and that one's
//               high-priority stream, behind `flags_ev` -- the users flagged by the time a first pass launches its sweep (every user
//               with a TEST item in the noise zone), in one piece, into a metric block of that context (block()).  run_call (device
//               entry, un-ranged batches) and the host entry (beside the last batch of a range) each bring their count and deliver
//               the results themselves.
template <class T> struct ExactPass {
    Ctx &cx;                                                         // the call's context: whose `flags_ev` a pass beside waits for; g_last_ctx again afterwards
    Ctx *pc = nullptr; hipStream_t ps = nullptr;                     // where the pass runs: that context, or its NOISE_SLOT context; the stream
    std::unique_lock<std::mutex> lock;                               // beside: the NOISE_SLOT context's mutex, held until this object goes
    int *noise_row = nullptr, *row_user = nullptr; unsigned char *only = nullptr;
    explicit ExactPass(Ctx &c) : cx(c) {}                            // (beside: open() follows)
    ExactPass(Ctx &c, hipStream_t stream) : cx(c), pc(&c), ps(stream) {}
    bool beside() const { return pc != &cx; }
    void open(hipEvent_t other = nullptr)
    {
        pc = &peer_context(cx, NOISE_SLOT);
        lock = std::unique_lock<std::mutex>(pc->mu);
        if (!pc->own_stream) HIP_CHECK(create_stream(&pc->own_stream, pc->high_priority));
        ps = pc->own_stream;
        HIP_CHECK(hipStreamWaitEvent(ps, cx.flags_ev, 0));           // flags, their snapshot and the dense train rows are in place
        if (other) HIP_CHECK(hipStreamWaitEvent(ps, other, 0));
    }
    // A row for every user flagged in `flags` [m] and not in `skip` (optional).  `known` >= 0: their number; else they are counted
    // on the pass's stream and the count is read back through `*word` (one wait for that stream).  Returns the number.
    int assign(int m, const int *flags, const int *skip, int known, int *word)
    {
        Workspace &pw = pc->ws;
        noise_row = pw.array<int>(WS_NOISE_ROW, (size_t)m);
        row_user = pw.array<int>(WS_NOISE_ROW_USER, (size_t)(known >= 0 ? std::max(known, 1) : m));
        int *counter = pw.array<int>(WS_NOISE_COUNTER, 1);
        only = pw.array<unsigned char>(WS_NOISE_ONLY, (size_t)m);
        HIP_CHECK(hipMemsetAsync(counter, 0, sizeof(int), ps));
        hipLaunchKernelGGL(k_noise_assign_rows, dim3(cdiv(m, 256)), dim3(256), 0, ps, m, flags, skip, noise_row, row_user, counter);
        if (known >= 0) return known;
        HIP_CHECK(hipMemcpyAsync(word, counter, sizeof(int), hipMemcpyDeviceToHost, ps));
        HIP_CHECK(hipStreamSynchronize(ps));
        return *word;
    }
    // the metric block of a pass that must not write into the call's outputs, [metric][users x width], in the pass's workspace
    void block(Call<T> &c, const MetricLayout &lay) const
    {
        lay.point_at(pc->ws.array<T>(WS_O_EXACT, std::max<size_t>(lay.block_size((size_t)c.m), 1)), (size_t)c.m, c.out);
    }
    // The flagged users of rows [r0, r0 + rows) through the pipeline, as passes of call `c` (over all its m users): their noise rows,
    // then run().  Dense train rows of a pass beside: the first pass's when `cx` still holds them for exactly these users, or with
    // `own_rows` rows built here for the flagged users alone (train items only; fp32, when they fit the PEER workspace).  A
    // sequential pass finds the rows of its own context itself (Call::same_train_rows).
    void step(Call<T> c, const NoiseGeom<T> &g, long long r0, int rows, bool own_rows = false)
    {
        Workspace &pw = pc->ws;
        const int m = c.m, n = c.n;
        hipLaunchKernelGGL(k_noise_select, dim3(cdiv(m, 256)), dim3(256), 0, ps, m, noise_row, (int)r0, (int)r0 + rows, only);
        unsigned *D = pw.array<unsigned>(WS_NOISE_DRAWS, (size_t)rows * (size_t)g.d_ld);
        T *E = pw.array<T>(WS_NOISE_ROWS, (size_t)rows * (size_t)g.e_ld);
        const long long words = dense_row_words(n);
        unsigned *bits = nullptr;
        if (own_rows) {
            const bool fit = std::is_same<T, float>::value && dense_rows_fit(pw, m, n);
            if (fit) {
                bits = (unsigned *)pw.get(WS_TRAIN_BITS, (size_t)m * (size_t)words * 4);
                pc->dense.invalidate();
                launch_train_bits(ps, m, n, (int)words, c.train_p, c.train_i, (const int *)nullptr, c.test_i, bits, (const Plan *)nullptr, only);
                c.ext_bits = bits; c.ext_words = words; c.ext_masked = false;
            }
            c.dense_fit = fit ? 1 : 0;
        } else if (beside() && cx.dense.built_by(cx.ws, c.items_tag, c.train_p, m)) {
            c.ext_bits = cx.dense.rows(cx.ws); c.ext_words = cx.dense.words; c.ext_masked = cx.dense.masked;             // the first pass's rows
        }
        noise_make_rows<T>(own_rows ? *pc : cx, c, g, row_user + r0, rows, c.train_p, c.user0, D, E, ps, bits, words);
        set_exact_pass<T>(c, only, noise_row, (int)r0, E, g.e_ld, rows);
        // (beside: whatever fails in there -- the peer context duplicates workspace under memory pressure --, nothing of it may still
        // be reading the call's context's buffers (flag snapshot, dense train rows, A / B) when the error reaches the caller)
        try { run<T>(c, ps, *pc); }
        catch (...) {
            if (beside()) { sync(); if (pc->side_stream) (void)hipStreamSynchronize(pc->side_stream); }
            g_last_ctx = &cx;
            throw;
        }
        g_last_ctx = &cx;                                            // rm_get_timings reports the main pass, not the small exact one
    }
    // the sequential pass: every flagged user, in pieces of `cap` rows; returns their number
    int sequential(const Call<T> &c, const int *flags, const int *skip, int known, int *word)
    {
        const NoiseGeom<T> g(pc->ws, c.n);
        const int n_flagged = assign(c.m, flags, skip, known, word);
        for (long long r0 = 0; r0 < n_flagged; r0 += g.cap) step(c, g, r0, (int)std::min<long long>(g.cap, n_flagged - r0));
        return n_flagged;
    }
    void sync() { if (pc) (void)hipStreamSynchronize(ps); }
};

// `defer` (host-pointer calls in user batches): the fp32 noise path ends with a look at what the first pass flagged on top of the
// users evaluated beside it -- a wait for the whole batch.  With `defer` that tail is handed back instead of run: the caller
// enqueues its next batch first and runs the tail when it needs this batch's results (true = a sequential exact pass rewrote
// outputs behind whatever the caller had enqueued after this call).
template <class T>
void run_call(const Call<T> &c_in, hipStream_t stream, Ctx &cx, std::function<bool()> *defer = nullptr)
{
    if (defer) *defer = nullptr;
    if (!c_in.noise) { run<T>(c_in, stream, cx); return; }
    Call<T> c0 = c_in;
    if (c0.items_tag == 0) c0.items_tag = g_call_counter.fetch_add(1);                   // (a device-pointer call: its passes share B)
    Workspace &ws = cx.ws;
    const int m = c0.m;
    cx.need_noise_words();
    if (sizeof(T) == 4 && c0.first_pass_flags) {                    // a batch of a host-pointer call: see PassFlags::first_pass_flags
        Call<T> c1 = c0;
        set_first_pass(c1, c0.first_pass_flags);
        run<T>(c1, stream, cx);
        return;
    }
    if (sizeof(T) == 4 && c0.dense_fit < 0) c0.dense_fit = dense_rows_fit(ws, m, c0.n) ? 1 : 0;
    const NoiseGeom<T> g(ws, c0.n);
    const MetricLayout lay(c0.out, c0.cumulative ? (size_t)c0.K : 1);
    if (sizeof(T) == 8) {
        if (!c0.csr_checked) { check_csr_now<T>(c0, stream, cx); c0.csr_checked = true; }     // (the noise rows below index by the CSR arrays)
        for (long long b0 = 0; b0 < m; b0 += g.cap) {
            const int mb = (int)std::min<long long>(g.cap, m - b0);
            Call<T> c = c0;
            c.A = c0.A_from((size_t)b0); c.m = mb; c.train_p = c0.train_p + b0; c.test_p = c0.test_p + b0; c.user0 = c0.user0 + b0;
            c.outputs() = c0.from_user((size_t)b0, lay.per, c0.K);
            if (c0.only_users) c.only_users = c0.only_users + b0;
            unsigned *D = ws.array<unsigned>(WS_NOISE_DRAWS, (size_t)mb * (size_t)g.d_ld);
            T *E = ws.array<T>(WS_NOISE_ROWS, (size_t)mb * (size_t)g.e_ld);
            noise_make_rows<T>(cx, c0, g, nullptr, mb, c.train_p, c.user0, D, E, stream);
            set_noise_for_all(c, E, g.e_ld);
            run<T>(c, stream, cx);
        }
        return;
    }
    int *flag = ws.array<int>(WS_NOISE_FLAG, (size_t)m);
    HIP_CHECK(hipMemsetAsync(flag, 0, sizeof(int) * (size_t)m, stream));
    Call<T> c1 = c0;
    set_first_pass(c1, flag);
    // Every user the noise can touch through a TEST item in the zone -- in practice all the flagged users -- is known once the
    // positives are scored, before the first sweep starts: their exact pass (noise rows, a small sweep, two dozen short
    // launches: 1.4 ms at BASELINE C2) runs on the PEER context and its stream BESIDE the first sweep, writes into a metric block of
    // its own, and a scatter behind both puts its results over the first pass's.  Users flagged only by the first pass's
    // k_finalize (a top-K score in the zone) get the sequential exact pass below, as does everybody when the ranking outputs
    // of rm_rank_* are wanted.
    const bool beside = !c0.topk_idx && !c0.only_users && !g_sw.noise_sequential;
    int *snap = nullptr;
    if (beside) {
        snap = ws.array<int>(WS_NOISE_FLAG_SNAP, (size_t)m);
        cx.noise_words->first_early = 0;
        c1.flag_snapshot = snap; c1.flag_count_host = &cx.noise_words->first_early; c1.flags_event = cx.flags_ev;
    }
    Plan *plan = ws.array<Plan>(WS_PLAN, 1);
    int n_beside = 0;
    ExactPass<T> nb(cx);
    run<T>(c1, stream, cx);
    // The exact pass beside the first sweep: enqueued right behind the first pass, on the NOISE_SLOT context's HIGH-PRIORITY streams
    // (create_stream) -- at normal priority its kernels would only be served when the sweep, which fills every compute unit, drains.
    // (Measured and dropped: enqueueing it from inside the first pass's run(), in front of the sweep's dispatch:
    // the host-side chain of the pass, two waits, keeps the sweep off the device for 0.8 ms.)
    if (beside) {
        HIP_CHECK(hipEventSynchronize(cx.flags_ev));                 // (early: the sweep has only just been launched)
        const int n_early = cx.noise_words->first_early;
        if (n_early > 0 && n_early <= g.cap) {
            nb.open();
            nb.assign(m, snap, nullptr, n_early, nullptr);
            Call<T> c = c0;
            nb.block(c, lay);
            ScatterArgs<T> sc{};
            for (int i = 0; i < 10; i++) { sc.width[i] = (int)lay.width(i); sc.dst[i] = c0.out[i]; sc.src[i] = c.out[i]; }
            nb.step(c, g, 0, n_early);
            HIP_CHECK(hipEventRecord(cx.pass_ev, nb.ps));
            HIP_CHECK(hipStreamWaitEvent(stream, cx.pass_ev, 0));    // behind the first pass (stream order) AND the exact one
            hipLaunchKernelGGL(k_noise_scatter<T>, dim3(cdiv(m, 256)), dim3(256), 0, stream, m, snap, sc);
            HIP_CHECK(hipEventRecord(cx.done, stream));              // (the context's "last work" now ends with the scatter)
            n_beside = n_early;
        }
    }
    int *n_flagged_host = &cx.noise_words->first_final;
    HIP_CHECK(hipMemcpyAsync(n_flagged_host, &plan->n_noise_flagged, sizeof(int), hipMemcpyDeviceToHost, stream));
    auto tail = [=, &cx]() -> bool {
        HIP_CHECK(hipStreamSynchronize(stream));
        cx.timings[Ctx::TM_LAUNCHES] = 0;
        const int n_flagged = *n_flagged_host - n_beside;               // what the first pass's k_finalize flagged on top (top-K in the zone)
        if (n_flagged <= 0) return false;
        Call<T> c = c0;
        c.same_train_rows = true;
        ExactPass<T>(cx, stream).sequential(c, flag, n_beside > 0 ? (const int *)snap : (const int *)nullptr, n_flagged, nullptr);
        return true;
    };
    if (defer) *defer = tail;
    else tail();
}

template <class F> int guarded(F &&f)
{
    g_err.clear();
    try { f(); return RM_OK; }
    catch (const RmError &e) { g_err = e.msg; return e.code; }
    catch (const std::bad_alloc &) { g_err = "host allocation failed"; return RM_ERR_NOMEM; }
    catch (const std::exception &e) { g_err = e.what(); return RM_ERR_HIP; }
}

// ---- interruption (reference src/recometrics.hpp:114-174: SignalSwitcher) ---------------------------------------------
// While a host-pointer call runs, SIGINT sets a flag instead of killing the process; the call looks at the flag between its
// user batches, stops, restores the previous handler, re-raises the signal (so that the caller's own handler -- Python's
// KeyboardInterrupt -- sees it) and reports the reference's message.  As in the reference only the first of several
// concurrent calls owns the handler (:141-143).  rm_request_interrupt() sets the same flag without a signal.
volatile std::sig_atomic_t g_interrupt = 0, g_interrupt_by_signal = 0;
std::atomic<bool> g_handler_locked{false};
extern "C" void rm_on_sigint(int) { g_interrupt = 1; g_interrupt_by_signal = 1; }
struct SignalGuard {
    void (*old_handler)(int) = nullptr;
    bool active = false;
    SignalGuard()
    {
        bool expected = false;
        if (g_handler_locked.compare_exchange_strong(expected, true)) {
            g_interrupt = 0; g_interrupt_by_signal = 0;
            old_handler = std::signal(SIGINT, rm_on_sigint);
            active = true;
        }
    }
    void restore()
    {
        if (active) { std::signal(SIGINT, old_handler); active = false; g_handler_locked.store(false); }
    }
    ~SignalGuard() { const bool mine = active; restore(); if (mine) { g_interrupt = 0; g_interrupt_by_signal = 0; } }
    void check()                                  // reference :166-173
    {
        if (!g_interrupt) return;
        const bool by_signal = g_interrupt_by_signal != 0;
        const bool mine = active;
        restore();
        if (mine) { g_interrupt = 0; g_interrupt_by_signal = 0; }
        if (by_signal && mine) std::raise(SIGINT);
        throw RmError{RM_ERR_INTERRUPTED, "Error: procedure was interrupted.\n"};
    }
};

// devices of the calls sharded inside the library (rm_set_devices); empty = the calling thread's current device only
std::mutex g_dev_mu;
std::vector<int> g_devices;

// item factors of a sharded call: uploaded from the host by shard 0, copied device-to-device (xGMI) by the others
struct SharedItems {
    std::mutex mu; std::condition_variable cv;
    bool ready = false, failed = false;
    const void *src = nullptr; int src_device = 0;
    // shards that have not finished (or given up on) their device-to-device copy of `src` yet: shard 0 keeps its context --
    // and with it the buffer `src` points to -- locked until this is 0, so that no later call can overwrite or free the
    // buffer under a slow shard
    int copies_pending = 0;
    void copy_done() { std::lock_guard<std::mutex> lk(mu); copies_pending--; cv.notify_all(); }
};

// direct device-to-device copies (xGMI on a multi-GPU node): enabled once per ordered pair, by the copying side
inline void enable_peer_access(int dst_device, int src_device)
{
    static std::mutex mu;
    static std::map<std::pair<int, int>, bool> done;
    if (dst_device == src_device) return;
    std::lock_guard<std::mutex> lk(mu);
    bool &d = done[std::make_pair(dst_device, src_device)];
    if (d) return;
    d = true;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst_device, src_device) == hipSuccess && can) {
        const hipError_t e = hipDeviceEnablePeerAccess(src_device, 0);          // (the current device is dst_device)
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();   // not fatal: hipMemcpyPeer stages through the host
        else (void)hipGetLastError();
    }
}


// RM_HOST_TRACE: the host entry's time stamps and run()'s, on stderr at the end of a host call
inline void print_host_trace(int n_batches, const std::vector<std::pair<const char *, double>> &stamps)
{
    std::string line = "rm host trace (" + std::to_string(n_batches) + " batches, ms):";
    for (auto &st : stamps) { char buf[96]; snprintf(buf, sizeof buf, " [%s %.3f]", st.first, st.second); line += buf; }
    fprintf(stderr, "%s\n", line.c_str());
    std::lock_guard<std::mutex> tl(g_run_trace.mu);
    std::string l2 = "rm run trace (ms since the library was loaded):";
    for (auto &pt : g_run_trace.pts) { char buf[112]; snprintf(buf, sizeof buf, " [%s %.3f]", pt.first, pt.second); l2 += buf; }
    fprintf(stderr, "%s\n", l2.c_str());
    g_run_trace.pts.clear();
}

// Users per batch of a host call at most: ~0.4 s of device work at the rate the sweep sustains (2 n k flop per user), whole user
// blocks, or RM_BATCH_USERS (tests: equal batches of this size); with k_metrics > 256 what one context's lane buffers or score rows hold.
// The caller's scores (`scores`): a user of a batch costs its row of S in each of the two upload buffers (ws.get rounds an allocation
// up by an eighth) and its masked row, which run() wants inside a third of what is then free: b (2.25 + 3) rows <= free memory, taken
// with a margin for the top-K scratch; what the workspace already holds of exactly these buffers counts as free.
// 16-bit scores (`s_elem` = 2 with T = float): the two upload rows are half as large, the masked row is not -- b (1.125 + 3) rows with
// the same margin, 5.5 rows in the place of 7.
template <class T> long long batch_users_max(const Workspace &ws, int n, int k, int K, bool scores = false, size_t s_elem = sizeof(T))
{
    if (scores) {
        const long long row = score_row_stride(n) * (long long)sizeof(T);
        const long long per_user = s_elem == sizeof(T) ? 7 * row : (8 * row + 6 * score_row_stride(n) * (long long)s_elem) / 2;
        long long batch = free_plus_owned(ws, {WS_STREAM_SCORES, WS_SEL_HI, WS_SEL_LO, WS_IN_S0, WS_IN_S1}) / per_user;
        if (g_sw.stream_budget_mb >= 0) batch = std::min<long long>(batch, stream_budget_bytes(ws) * 3 / 4 / row);
        if (g_sw.batch_users > 0) batch = std::min<long long>(batch, (long long)g_sw.batch_users);
        return std::max<long long>(1, std::min<long long>(batch, 1 << 20));
    }
    const double rate = std::is_same<T, float>::value ? 6.0e13 : 2.5e13;
    double bu = 0.4 * rate / (2.0 * (double)n * (double)k);
    if (g_sw.batch_users > 0) bu = g_sw.batch_users;
    long long batch = (long long)std::min<double>(std::max(bu, 1024.0), 2.0e9);
    batch = (batch + 1023) / 1024 * 1024;
    // k_metrics > 256: the lane buffers when they fit at all (run(): want_lane; one block's worth per 4 GU users on top of the grid's
    // floor -- lane_blocks_bound), sized so that run() finds every batch fitting; else score rows (ext_topk)
    const long long lane_blocks = K > 256 && lane_lists_possible<T>(K) ? lane_budget_bytes(ws) * 3 / 4 / lane_list_bytes<T>(K, 1) - lane_blocks_bound<T>(0) : 0;
    if (lane_blocks >= 8) batch = std::max<long long>(1024, std::min<long long>(batch, lane_blocks * 4 * Prec<T>::GU / 1024 * 1024));
    else if (K > 256) {                                            // one score row per user of the batch (run(): ext_topk),
        const long long row = score_row_stride(n) * (long long)sizeof(T);    // with a margin for what run() allocates first
        batch = std::max<long long>(1, std::min<long long>(batch, stream_budget_bytes(ws) * 3 / 4 / row));
    }
    return batch;
}
// Batch boundaries of m users, at most `batch` per batch (`forced`: all of that size): a first batch of a QUARTER of the users (whole
// kilo-users) when the range is large enough for the pipeline to matter -- its upload is the only one nothing hides --, then three
// times the batch before (its upload hides behind the batch before, whose kernels take ~2.5 x as long per user as the copy).
// BASELINE C2: 34,816 + 103,677 users.
// Every batch pays the fixed parts of preparation and finalisation again and its plan only comes back when the sweep in front
// of it has drained, so fewer batches win once the first upload is paid for: round 5 (preparation 0.88 -> 0.56 ms) 9.6 ms per
// call against 9.9 with (1/8, 3/8, 1/2), and with the tie noise 10.3 against 10.85 (one batch fewer for the exact pass to
// wait behind; `profiles/r5_host_entry.txt`).  Round 3, when a batch's fixed parts cost twice as much: (1/8, 3/8, 1/2) 10.4,
// (1/4, 3/4) 10.6, without the second context 11.7 (`profiles/r3_host_entry.txt`).
inline std::vector<long long> batch_cuts(long long m, long long batch, bool forced)
{
    std::vector<long long> cuts{0};
    long long next = (forced || m <= 16384) ? batch : std::min<long long>(batch, std::max<long long>(8192, (m / 4 + 1023) / 1024 * 1024));
    while (cuts.back() < m) {
        long long b1 = std::min<long long>(m, cuts.back() + next);
        if (m - b1 < 2048 && m - cuts.back() <= batch) b1 = m;                  // no crumb at the end
        cuts.push_back(b1);
        next = forced ? batch : std::min<long long>(batch, next * 3);
    }
    return cuts;
}

// The item factors of a host call, dense rows of k, into `dB` on the upload stream.  In a sharded call shard 0 uploads them from
// the host and publishes the buffer; the others copy it device-to-device (xGMI) and report when they are done with it.
// Whatever happens, the other shards must neither wait for item factors that never come nor copy from a buffer that is being
// reused: the destructor has shard 0 publish (possibly a failure) and then wait for every copy, and the others report theirs.
template <class T> struct ItemUpload {
    const Request<T> &h; SharedItems *sh; int shard; bool published = false, reported = false;
    ~ItemUpload()
    {
        if (!sh) return;
        if (shard == 0) {
            std::unique_lock<std::mutex> sl(sh->mu);
            if (!published) { sh->ready = true; sh->failed = true; sh->cv.notify_all(); }
            sh->cv.wait(sl, [&] { return sh->copies_pending <= 0; });
        } else if (!reported) sh->copy_done();
    }
    void run(void *dB, int device, hipStream_t up)
    {
        const int n = h.n, k = h.k;
        const size_t fe = h.f_elem();                                // (16-bit factors travel as they are: half the bytes, here and between the shards)
        if (h.scores) {                                              // no item factors: the shards' handshake alone
            if (sh && shard == 0) { std::lock_guard<std::mutex> sl(sh->mu); sh->ready = true; sh->failed = false; sh->src = dB; sh->src_device = device; published = true; sh->cv.notify_all(); }
            else if (sh) { reported = true; sh->copy_done(); }
            return;
        }
        if (!sh || shard == 0) {
            // (dense rows: ONE plain copy -- a 2-D copy of pageable memory goes through a staging buffer and a second,
            // device-side pass: 1.1 ms more for BASELINE C2's A and B)
            hipError_t e = h.ldb == (size_t)k ? hipMemcpyAsync(dB, h.B, fe * (size_t)n * k, hipMemcpyHostToDevice, up)
                                              : hipMemcpy2DAsync(dB, fe * k, h.B, fe * h.ldb, fe * k, n, hipMemcpyHostToDevice, up);
            if (sh) {
                if (e == hipSuccess) e = hipStreamSynchronize(up);
                std::lock_guard<std::mutex> sl(sh->mu);
                sh->ready = true; sh->failed = e != hipSuccess; sh->src = dB; sh->src_device = device;
                published = true;
                sh->cv.notify_all();
            }
            HIP_CHECK(e);
        } else {
            {
                std::unique_lock<std::mutex> sl(sh->mu);
                sh->cv.wait(sl, [&] { return sh->ready; });
                if (sh->failed) throw RmError{RM_ERR_HIP, "upload of the item factors failed on the first device"};
            }
            enable_peer_access(device, sh->src_device);
            HIP_CHECK(hipMemcpyPeerAsync(dB, device, sh->src, sh->src_device, fe * (size_t)n * k, up));
            HIP_CHECK(hipStreamSynchronize(up));                      // the source buffer is shard 0's: tell it when we are done with it
            reported = true;
            sh->copy_done();
        }
    }
};

// Users [u0, u1) of a host call on the current device.  The inputs are staged into HBM batch by batch and the batches are
// pipelined: while the kernels of batch i run on the call's stream, the rows of batch i + 1 (user factors, train / test CSR
// rows) are uploaded on a second stream into their places in the range's device arrays -- a batch only ever reads its own
// rows, so nothing is double-buffered.  The first batch is small (its upload is the only one nothing hides) and the batches
// double in size from there; they are also what the interrupt flag is looked at between (reference :488-489).  Each batch's
// outputs go straight into the caller's arrays.  `shared` (sharded calls) says where the item factors come from.
// One member function per stage; run_host_range() below is the sequence.
template <class T> struct HostRange {
    // a batch in flight on one of the two contexts (`tail`: what the fp32 tie noise still has to look at once the batch is through, run_call)
    struct InFlight { bool on = false; long long b0 = 0; int mb = 0; std::function<bool()> tail; };
    // Members are destroyed in reverse order of declaration, and these four must go in this order: the lock of the pass beside the
    // last batch (in `bes`), the peer context's lock, the item upload's guard (shard 0 waits there for the other shards' copies of
    // in_B) and last the range's own context.  `items` is constructed before anything that can throw: its destructor completes the
    // handshake with the other shards, whatever happens.
    std::lock_guard<std::mutex> lk;
    ItemUpload<T> items;
    std::unique_lock<std::mutex> peer_lock;
    ExactPass<T> bes;
    bool bes_ran = false; int bes_count = 0; T *bes_hx = nullptr; int *bes_hu = nullptr;     // what the pass beside the last batch left in page-locked memory

    const Request<T> &h; const int u0, m, n, k, K; Ctx &cx; Workspace &ws; hipStream_t stream, up = nullptr;
    SharedItems *shared; int shard; unsigned long long tag;
    const MetricLayout lay;                                           // (per: values per user of the eight top-K metrics)
    // stage_inputs()
    long long tr0 = 0, te0 = 0, nnz_tr = 0, nnz_te = 0;
    void *dS[2] = {nullptr, nullptr}; const void *cur_S = nullptr;        // the caller's scores: upload buffers of the batches, the one of the batch being enqueued
    char *dB = nullptr, *dA = nullptr;                                // the factors' resident copies, dense rows of k elements of Request::f_elem() bytes
    T *dtev = nullptr; int *dtrp = nullptr, *dtep = nullptr, *dtri = nullptr, *dtei = nullptr;
    std::vector<int> rb;                                              // rebased index pointers (only when the range does not start at 0)
    const int *trp = nullptr, *tep = nullptr;
    Outputs<T> d_rank;                                                // the ranking outputs of the range on the device (rm_rank_*, lists)
    // plan_batches()
    std::vector<long long> cuts; int n_batches = 0;
    Ctx *ctxs[2]; hipStream_t streams[2]; bool two_ctx = false;
    T *dblocks[2] = {nullptr, nullptr}, *hblocks[2] = {nullptr, nullptr};
    bool range_noise = false; int *range_flag = nullptr, *range_snap = nullptr;
    // the batches
    long long users_copied = 0;                                       // users [0, users_copied) of the range have been handed over to the caller
    long long flagged_total = 0;                                      // fp32 tie noise over the range: users the batches' first passes flagged
    InFlight fl[2];
    // RM_HOST_TRACE (timing studies only): host-side time stamps of the pipeline, printed at the end of the call
    std::vector<std::pair<const char *, double>> stamps; std::chrono::steady_clock::time_point t_start;
    void stamp(const char *what) { if (g_sw.host_trace) stamps.emplace_back(what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count()); }

    HostRange(const Request<T> &h_, int u0_, int u1, Ctx &cx_, hipStream_t stream_, SharedItems *shared_, int shard_, unsigned long long tag_)
        : lk(cx_.mu), items{h_, shared_, shard_}, bes(cx_), h(h_), u0(u0_), m(u1 - u0_), n(h_.n), k(h_.k), K(h_.K), cx(cx_), ws(cx_.ws), stream(stream_),
          shared(shared_), shard(shard_), tag(tag_), lay(h_.out, h_.cumulative ? (size_t)h_.K : 1), ctxs{&cx_, &cx_}, streams{stream_, stream_}
    {
        cx.acc[0] = cx.acc[1] = cx.acc[2] = cx.acc[3] = 0; cx.ev_recorded = false;
        g_last_ctx = &cx;
    }

    // workspace buffers of the range, index pointers rebased to it and uploaded, ranking outputs; false = no user (the item factors' handshake only)
    bool stage_inputs()
    {
        if (!cx.up_stream) {
            HIP_CHECK(hipStreamCreateWithFlags(&cx.up_stream, hipStreamNonBlocking));
            for (int i = 0; i < 2; i++) HIP_CHECK(hipEventCreateWithFlags(&cx.up_ev[i], hipEventDisableTiming));
        }
        up = cx.up_stream;
        if (cx.ev_valid) HIP_CHECK(hipStreamWaitEvent(up, cx.done, 0));   // the previous call on this context may still read the buffers
        // item factors, dense rows of k (typed where they are T: the guard mode's poison is the type's)
        const auto factors = [&](WsBuf id, size_t elems) { return h.f_type == SCORE_SAME ? (char *)ws.array<T>(id, elems) : ws.array<char>(id, elems * h.f_elem()); };
        dB = factors(WS_IN_B, (size_t)n * k);
        if (m <= 0) { items.run(dB, cx.device, up); HIP_CHECK(hipStreamSynchronize(up)); return false; }
        // this range's users: factors, CSR rows with the index pointers rebased to the range
        tr0 = h.train_p[u0]; te0 = h.test_p[u0];
        nnz_tr = (long long)h.train_p[u0 + m] - tr0; nnz_te = (long long)h.test_p[u0 + m] - te0;
        dA = factors(WS_IN_A, (size_t)m * k);
        dtrp = ws.array<int>(WS_IN_TRP, (size_t)(m + 1));
        dtep = h.reco ? nullptr : ws.array<int>(WS_IN_TEP, (size_t)(m + 1));
        dtri = ws.array<int>(WS_IN_TRI, (size_t)std::max<long long>(nnz_tr, 1));
        dtei = ws.array<int>(WS_IN_TEI, (size_t)std::max<long long>(nnz_te, 1));
        dtev = h.test_v ? ws.array<T>(WS_IN_TEV, (size_t)std::max<long long>(nnz_te, 1)) : nullptr;
        trp = h.train_p + u0; tep = h.test_p + u0;
        if (tr0 || te0) {
            rb.resize(2 * (size_t)(m + 1));
            for (int i = 0; i <= m; i++) { rb[i] = h.train_p[u0 + i] - (int)tr0; rb[m + 1 + i] = h.test_p[u0 + i] - (int)te0; }
            trp = rb.data(); tep = rb.data() + m + 1;
        }
        HIP_CHECK(hipMemcpyAsync(dtrp, trp, sizeof(int) * (size_t)(m + 1), hipMemcpyHostToDevice, up));
        if (dtep) HIP_CHECK(hipMemcpyAsync(dtep, tep, sizeof(int) * (size_t)(m + 1), hipMemcpyHostToDevice, up));
        if (h.topk_idx) {
            d_rank.topk_idx = ws.array<int>(WS_O_TOPK_IDX, (size_t)m * K);
            if (h.topk_score) d_rank.topk_score = ws.array<T>(WS_O_TOPK_SCORE, (size_t)m * K);
            if (h.pos_rank) d_rank.pos_rank = ws.array<long long>(WS_O_POS_RANK, (size_t)std::max<long long>(nnz_te, 1));
            d_rank.status = ws.array<int>(WS_O_STATUS, (size_t)m);
        }
        return true;
    }

    // the batches' boundaries, the second context and its lock, the metric block of a batch on either context, the flags of the tie noise
    void plan_batches()
    {
        const bool forced = g_sw.batch_users > 0;                        // tests: equal batches of this size
        cuts = batch_cuts(m, batch_users_max<T>(ws, n, k, K, h.scores, h.s_elem()), forced);
        n_batches = (int)cuts.size() - 1;
        long long mb_max = 0;
        for (int bi = 0; bi < n_batches; bi++) mb_max = std::max(mb_max, cuts[bi + 1] - cuts[bi]);
        // the metric block of a batch: [metric][users of the batch x width], one device buffer, one D2H copy into page-locked
        // staging, scattered into the caller's arrays by the host (ten pageable copies cost 35-140 us EACH in host time)
        // Batches alternate between this context and its peer (own workspace, events and stream): batch i + 1 is planned and
        // packed while batch i sweeps, and its sweep takes over the compute units as batch i's blocks drain.
        // (not with k_metrics > 256: a batch is then sized by the score rows ONE context may hold -- a third of the free memory --
        // and a second context holding as much again leaves the first one's next batch short: RM_ERR_NOMEM on the third batch)
        const bool rows_bound = K > 256 || g_sw.ext_topk || h.scores; // (the lane buffers of k_metrics > 256 are as large; the caller's scores: see upload_users)
        if (n_batches > 1 && !rows_bound && !g_sw.one_context) {
            Ctx &pc = peer_context(cx);
            peer_lock = std::unique_lock<std::mutex>(pc.mu);
            if (!pc.own_stream) HIP_CHECK(hipStreamCreateWithFlags(&pc.own_stream, hipStreamNonBlocking));
            if (cx.ev_valid) HIP_CHECK(hipStreamWaitEvent(pc.own_stream, cx.done, 0));       // (buffers of the range may still be read by an earlier call)
            ctxs[1] = &pc; streams[1] = pc.own_stream;
        }
        for (int i = 0; i < 2; i++) {
            if (i == 1 && ctxs[1] == ctxs[0]) { dblocks[1] = dblocks[0]; hblocks[1] = hblocks[0]; break; }
            dblocks[i] = ctxs[i]->ws.array<T>(WS_O_BLOCK, std::max<size_t>(lay.block_size((size_t)mb_max), 1));
            hblocks[i] = lay.rec_w ? (T *)ctxs[i]->pinned_get(sizeof(T) * lay.block_size((size_t)mb_max)) : nullptr;
        }
        two_ctx = ctxs[1] != ctxs[0];
        // the caller's scores: the rows of a batch, dense, in one of two buffers -- batch i + 1 travels while batch i runs, and with one
        // context batch i - 1 has been waited for by then
        if (h.scores) for (int i = 0; i < std::min(n_batches, 2); i++) dS[i] = ws.array<char>(i ? WS_IN_S1 : WS_IN_S0, (size_t)mb_max * (size_t)n * h.s_elem());
        // fp32 tie noise over several batches: every batch runs its first pass only and flags the users the noise can touch in its
        // slice of `range_flag`; ONE exact pass over the flagged users of the whole range follows the last batch.  (Per batch, the
        // exact pass costs two waits on the host -- for the flags, for its own plan -- during which the next batch is not enqueued:
        // 14.6 ms against 10.2 without noise at BASELINE C2, profiles/r4_host_entry.txt.)  Not with the ranking outputs of rm_rank_*.
        range_noise = h.noise && std::is_same<T, float>::value && n_batches > 1 && !h.topk_idx && !g_sw.noise_per_batch;
        if (!range_noise) return;
        // ... and the users flagged by the time the LAST batch launches its sweep -- every user with a test item in the noise zone, in
        // practice all of them -- are evaluated exactly BESIDE that sweep on a context of their own (exact_beside_last), as the device entry
        // does (run_call); what remains behind the last batch is the host-side scatter of their values, and an exact pass over the few
        // users only a batch's k_finalize flagged (a top-K score in the zone), usually none
        range_flag = ws.array<int>(WS_NOISE_FLAG_RANGE, (size_t)m);
        HIP_CHECK(hipMemsetAsync(range_flag, 0, sizeof(int) * (size_t)m, up));      // (in front of batch 0's rows: every batch waits for its rows' event)
        range_snap = ws.array<int>(WS_NOISE_FLAG_RANGE_SNAP, (size_t)m);
        cx.need_noise_words();
    }

    void upload_users(int bi)                                         // rows [cuts[bi], cuts[bi + 1]) into their places, on `up`
    {
        const long long b0 = cuts[bi], b1 = cuts[bi + 1];
        if (h.scores) {
            const size_t es = h.s_elem();
            const char *src = (const char *)h.S + ((size_t)u0 + b0) * h.lds * es;
            if (h.lds == (size_t)n) HIP_CHECK(hipMemcpyAsync(dS[bi & 1], src, es * (size_t)(b1 - b0) * n, hipMemcpyHostToDevice, up));
            else HIP_CHECK(hipMemcpy2DAsync(dS[bi & 1], es * n, src, es * h.lds, es * n, (size_t)(b1 - b0), hipMemcpyHostToDevice, up));
        } else {
            const size_t fe = h.f_elem();
            char *dst = dA + (size_t)b0 * k * fe; const void *src = h.A_from((size_t)u0 + b0);
            if (h.lda == (size_t)k) HIP_CHECK(hipMemcpyAsync(dst, src, fe * (size_t)(b1 - b0) * k, hipMemcpyHostToDevice, up));
            else HIP_CHECK(hipMemcpy2DAsync(dst, fe * k, src, fe * h.lda, fe * k, (size_t)(b1 - b0), hipMemcpyHostToDevice, up));
        }
        const long long r0 = trp[b0], r1 = trp[b1], e0 = tep[b0], e1 = tep[b1];      // range-relative entries of the batch
        if (r1 > r0) HIP_CHECK(hipMemcpyAsync(dtri + r0, h.train_i + tr0 + r0, sizeof(int) * (size_t)(r1 - r0), hipMemcpyHostToDevice, up));
        if (e1 > e0) HIP_CHECK(hipMemcpyAsync(dtei + e0, h.test_i + te0 + e0, sizeof(int) * (size_t)(e1 - e0), hipMemcpyHostToDevice, up));
        if (dtev && e1 > e0) HIP_CHECK(hipMemcpyAsync(dtev + e0, h.test_v + te0 + e0, sizeof(T) * (size_t)(e1 - e0), hipMemcpyHostToDevice, up));
        HIP_CHECK(hipEventRecord(cx.up_ev[bi & 1], up));
    }
    // shard 0 sends the item factors first (the other shards are waiting for them); the others send their own rows first
    void first_uploads()
    {
        RM_TRACE_POINT("host entry: batches start");
        t_start = std::chrono::steady_clock::now();
        if (!shared || shard == 0) { items.run(dB, cx.device, up); stamp("items enqueued"); upload_users(0); }
        else { upload_users(0); items.run(dB, cx.device, up); HIP_CHECK(hipEventRecord(cx.up_ev[0], up)); }
        stamp("batch 0 rows enqueued");
    }
    // users [b0, b0 + mb) of the range as a call on the staged arrays: the request, rebased -- everything but the outputs (the request's
    // are the caller's host arrays: enqueue_batch and ExactPass::block point a call at device arrays of its own) and the tie noise's flags
    Call<T> batch_call(long long b0, int mb) const
    {
        Call<T> c(h);
        c.A = dA + (size_t)b0 * k * h.f_elem(); c.lda = k; c.B = dB; c.ldb = k; c.m = mb;
        if (h.scores) { c.S = cur_S; c.lds = (size_t)n; c.A = nullptr; c.B = nullptr; }
        c.train_p = dtrp + b0; c.train_i = dtri; c.nnz_train = nnz_tr;
        c.test_p = dtep ? dtep + b0 : nullptr; c.test_i = dtei; c.test_v = dtev; c.nnz_test = nnz_te;
        c.outputs() = Outputs<T>{};
        c.items_tag = tag; c.user0 = (long long)u0 + b0;
        return c;
    }
    // the device-to-host copies of the batch in flight on context `which`, enqueued behind the batch and once more when its tail
    // rewrote outputs
    void copy_out(int which)
    {
        const long long b0 = fl[which].b0; const int mb = fl[which].mb;
        Ctx &bc = *ctxs[which]; hipStream_t bs = streams[which];
        const Plan *plan = bc.ws.array<Plan>(WS_PLAN, 1);
        // (`range_noise`: run_call ran on this context with the noise on, so the context has its words)
        if (range_noise) HIP_CHECK(hipMemcpyAsync(&bc.noise_words->batch_flagged, &plan->n_noise_flagged, sizeof(int), hipMemcpyDeviceToHost, bs));
        if (lay.rec_w) HIP_CHECK(hipMemcpyAsync(hblocks[which], dblocks[which], sizeof(T) * lay.block_size((size_t)mb), hipMemcpyDeviceToHost, bs));
        if (h.topk_idx) {
            const long long e0 = tep[b0], e1 = tep[b0 + mb];          // this batch's test entries (range-relative)
            HIP_CHECK(hipMemcpyAsync(h.topk_idx + ((size_t)u0 + b0) * K, d_rank.topk_idx + (size_t)b0 * K, sizeof(int) * (size_t)mb * K, hipMemcpyDeviceToHost, bs));
            if (h.topk_score) HIP_CHECK(hipMemcpyAsync(h.topk_score + ((size_t)u0 + b0) * K, d_rank.topk_score + (size_t)b0 * K, sizeof(T) * (size_t)mb * K, hipMemcpyDeviceToHost, bs));
            HIP_CHECK(hipMemcpyAsync(h.status + u0 + b0, d_rank.status + b0, sizeof(int) * (size_t)mb, hipMemcpyDeviceToHost, bs));
            if (h.pos_rank && e1 > e0) HIP_CHECK(hipMemcpyAsync(h.pos_rank + te0 + e0, d_rank.pos_rank + e0, sizeof(long long) * (size_t)(e1 - e0), hipMemcpyDeviceToHost, bs));
        }
    }

    void finish(int which)                                            // wait for the batch in flight on context `which`, hand its outputs over
    {
        InFlight &f = fl[which];
        if (!f.on) return;
        f.on = false;
        if (f.tail) { const bool again = f.tail(); f.tail = nullptr; if (again) copy_out(which); }
        HIP_CHECK(hipStreamSynchronize(streams[which]));
        stamp("batch done");
        for (int i = 0; i < 10; i++)
            if (lay.want[i]) std::memcpy(h.out[i] + ((size_t)u0 + f.b0) * lay.width(i), hblocks[which] + lay.block_off(i, (size_t)f.mb), sizeof(T) * (size_t)f.mb * lay.width(i));
        stamp("outputs scattered");
        users_copied = std::max<long long>(users_copied, f.b0 + f.mb);
        if (range_noise) flagged_total += ctxs[which]->noise_words->batch_flagged;
        if (n_batches > 1) {                                          // more than one batch: add up the stage timings
            Ctx &c = *ctxs[which];
            float ms[4] = {0, 0, 0, 0};
            c.stage_ms(ms);
            for (int i = 0; i < 4; i++) cx.acc[i] += ms[i];
            c.ev_recorded = false; cx.ev_recorded = false;
        }
    }

    void enqueue_batch(int bi)
    {
        const long long b0 = cuts[bi];
        const int mb = (int)(cuts[bi + 1] - b0);
        const int which = two_ctx ? (bi & 1) : 0;
        InFlight &f = fl[which];
        finish(which);                                               // (the batch two back: its context and staging are free again)
        HIP_CHECK(hipStreamWaitEvent(streams[which], cx.up_ev[bi & 1], 0));
        cur_S = dS[bi & 1];
        Call<T> c = batch_call(b0, mb);
        f.b0 = b0; f.mb = mb;
        c.outputs() = d_rank.from_user((size_t)b0, lay.per, K);      // (the ranking outputs of rm_rank_* and of the lists, when asked for)
        lay.point_at(dblocks[which], (size_t)mb, c.out);
        if (range_noise) c.first_pass_flags = range_flag + b0;
        const bool snap_here = range_noise && bi == n_batches - 1;
        if (snap_here) {
            c.flag_snapshot = range_snap + b0; c.flag_count_host = &cx.noise_words->first_early; c.flags_event = cx.flags_ev;
        }
        // enqueued (one short plan read-back inside; with more than one batch the tie noise's last look at the batch is deferred to
        // finish(): the next batch is enqueued first)
        run_call<T>(c, streams[which], *ctxs[which], n_batches > 1 ? &f.tail : nullptr);
        f.on = true;
        stamp("batch enqueued");
        copy_out(which);
        // the next batch's rows travel while this batch's sweep runs (the copies below block the host, not the device)
        if (bi + 1 < n_batches && !g_interrupt) upload_users(bi + 1);
        stamp("next rows enqueued");
        if (snap_here && !g_interrupt) {
            exact_beside_last(b0, (two_ctx && bi > 0) ? ctxs[(bi - 1) & 1]->ev[EV_PREP_END] : (hipEvent_t)nullptr);
            stamp("exact pass beside the last batch enqueued");
        }
        if (!two_ctx) finish(which);
    }
    // (the batch before the last one first: its outputs are copied to the caller while the last batch is still on the device)
    void finish_all() { const int older = two_ctx ? ((n_batches - 2) & 1) : 0; finish(older); finish(older ^ 1); g_last_ctx = &cx; }

    // ---- fp32 tie noise over the whole range (see `range_noise` in plan_batches) ----
    // every user of the range (an exact pass over it writes into a metric block of its own, ExactPass::block)
    Call<T> range_call() const { Call<T> c = batch_call(0, m); c.csr_checked = true; return c; }      // (every batch has looked at its rows)
    // an exact pass's results leave the device packed: one record of `lay.rec_w` values per evaluated user (k_noise_gather)
    void gather_exact(Ctx &gc, const Call<T> &c, const int *row_user, int count, hipStream_t st, T *&hx, int *&hu)
    {
        GatherArgs<T> ga{};
        for (int i = 0; i < 10; i++) { ga.src[i] = c.out[i]; ga.width[i] = (int)lay.width(i); ga.off[i] = (int)lay.rec_off[i]; }
        ga.out_w = (int)lay.rec_w;
        T *dg = gc.ws.array<T>(WS_O_EXACT_PACKED, lay.rec_w * (size_t)count);
        hipLaunchKernelGGL(k_noise_gather<T>, dim3(cdiv(count, 256)), dim3(256), 0, st, count, row_user, ga, dg);
        hx = (T *)gc.pinned_get(sizeof(T) * lay.rec_w * (size_t)count + sizeof(int) * (size_t)count);
        hu = (int *)(hx + lay.rec_w * (size_t)count);
        HIP_CHECK(hipMemcpyAsync(hx, dg, sizeof(T) * lay.rec_w * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipMemcpyAsync(hu, row_user, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost, st));
    }
    void scatter_exact(const T *hx, const int *hu, int count)         // the flagged users' records -> the caller's arrays
    {
        for (int f = 0; f < count; f++)
            for (int i = 0; i < 10; i++)
                if (lay.want[i]) std::memcpy(h.out[i] + ((size_t)u0 + hu[f]) * lay.width(i), hx + (size_t)f * lay.rec_w + lay.rec_off[i], sizeof(T) * lay.width(i));
    }
    // the exact pass beside the last batch's sweep, on the NOISE_SLOT context and its stream: flags as they stand once the last batch
    // has scored its positives, noise rows for those users (from dense train rows built for them alone), the pipeline for them,
    // and the copy of their metric block to page-locked memory -- all of it enqueued behind `flags_ev`, none of it waited for here
    // except the count of the flagged users
    // It runs on the NOISE_SLOT context's high-priority streams (create_stream): at normal priority, kernels that reach the device after
    // a sweep which fills every compute unit only start when it drains -- the pass began when the last batch ended and cost its full
    // 0.9 ms (profiles/r5_host_entry.txt).
    void exact_beside_last(long long b0_last, hipEvent_t other)
    {
        if (!lay.rec_w) return;
        // (`other`: the batch before the last runs on the other context's stream: its positives -- the early flags -- are in place once its
        // own sweep has been launched, the event run() records as EV_PREP_END; what its k_finalize flags later is the late pass's)
        bes.open(other);
        // (the earlier batches' flags as they stand: a flag their k_finalize sets later is the sequential pass's, below)
        if (b0_last > 0) HIP_CHECK(hipMemcpyAsync(range_snap, range_flag, sizeof(int) * (size_t)b0_last, hipMemcpyDeviceToDevice, bes.ps));
        // (the wait in there: the last batch's positives are scored; its sweep has just been launched)
        const int n_early = bes.assign(m, range_snap, nullptr, -1, &cx.noise_words->range_early);
        const NoiseGeom<T> g(bes.pc->ws, n);
        if (n_early <= 0 || n_early > g.cap) return;                  // nobody, or more rows than the budget holds at once: the sequential pass
        Call<T> c = range_call();
        bes.block(c, lay);
        bes.step(c, g, 0, n_early, true);                             // dense rows of the flagged users alone, train items only
        gather_exact(*bes.pc, c, bes.row_user, n_early, bes.ps, bes_hx, bes_hu);
        bes_ran = true; bes_count = n_early;
    }
    // behind the last batch: the values of the pass beside it, and the exact pass over the users of the range that the first passes
    // flagged and that pass has not seen (all of them without it)
    void exact_late(bool wanted)
    {
        if (!(range_noise && wanted && lay.rec_w)) { bes.sync(); return; }
        if (bes_ran) {                                                // (its results left the device while the last batch was sweeping)
            HIP_CHECK(hipStreamSynchronize(bes.ps));
            scatter_exact(bes_hx, bes_hu, bes_count);
            stamp("exact pass (beside) scattered");
        }
        // into a metric block of its own, from which the host takes the flagged users' values
        Call<T> c = range_call();
        ExactPass<T> late_pass(cx, stream);
        late_pass.block(c, lay);
        // (every batch reports how many users its first pass flagged: when the pass beside the last batch has seen them all --
        // the usual case -- nothing is left to look for)
        const long long late = flagged_total - (bes_ran ? bes_count : 0);
        if (late <= 0) return;
        const int n_flagged = late_pass.sequential(c, range_flag, bes_ran ? (const int *)range_snap : (const int *)nullptr, -1, &cx.noise_words->sequential);
        stamp("exact pass enqueued");
        if (n_flagged <= 0) return;
        T *hx = nullptr; int *hu = nullptr;
        gather_exact(cx, c, late_pass.row_user, n_flagged, stream, hx, hu);
        HIP_CHECK(hipStreamSynchronize(stream));
        scatter_exact(hx, hu, n_flagged);
        stamp("exact pass scattered");
    }
    //  a call that stops between its first passes and the exact one -- interrupt, failure -- must not leave the first
    // pass's un-noised values of the flagged users in the caller's arrays looking like results: they become NaN
    void withdraw_flagged()
    {
        if (!range_noise || !lay.rec_w || users_copied <= 0) return;
        std::vector<int> hf((size_t)users_copied);
        if (hipMemcpy(hf.data(), range_flag, sizeof(int) * (size_t)users_copied, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return; }
        for (long long u = 0; u < users_copied; u++) {
            if (!hf[(size_t)u]) continue;
            for (int i = 0; i < 10; i++)
                if (lay.want[i]) std::fill_n(h.out[i] + ((size_t)u0 + (size_t)u) * lay.width(i), lay.width(i), std::numeric_limits<T>::quiet_NaN());
        }
    }
    void drain()                                                      // a failure: nothing may still write into staging that goes away
    {
        for (int i = 0; i < 2; i++) (void)hipStreamSynchronize(streams[i]);
        (void)hipStreamSynchronize(up);
        bes.sync();
        withdraw_flagged();
    }
};

template <class T>
void run_host_range(const Request<T> &h, int u0, int u1, Ctx &cx, hipStream_t stream, SharedItems *shared, int shard, unsigned long long tag)
{
    HostRange<T> r(h, u0, u1, cx, stream, shared, shard, tag);
    if (!r.stage_inputs()) return;
    r.plan_batches();
    r.first_uploads();
    try {
        for (int bi = 0; bi < r.n_batches && !g_interrupt; bi++) r.enqueue_batch(bi);      // reference :488-489: the remaining users are skipped
        r.finish_all();
        // (ONE look at the flag decides both: whether the exact passes run, and whether the flagged users' values are withdrawn -- an
        // interrupt that arrives while the passes finish must not turn their finished, correct values into NaN)
        const bool interrupted = g_interrupt;
        r.exact_late(!interrupted);
        if (interrupted) r.withdraw_flagged();
    } catch (...) {
        r.drain();
        throw;
    }
    HIP_CHECK(hipStreamSynchronize(r.up));                            // `rb` and the caller's arrays go out of use (also after an interrupt)
    if (g_sw.host_trace) print_host_trace(r.n_batches, r.stamps);
}

// ---- what is wrong with a request: decided once per entry, on the host, before any device is asked for ---------------------------------
// (m == 0 is not an error: the reference's loop over users, src/recometrics.hpp:428-437, simply does not run; the entries return RM_OK
// before they get here.  `test_i` may be null when there is no test entry at all -- every user is then NaN, as in the reference --
// which is what a binding hands over for an empty index array.)
// `host`: the host form also looks at the index pointers themselves -- they say how much of the caller's index arrays is read at all
// (2 (m + 1) integers, before anything is sized or copied by them), and the lengths of those arrays are read from them -- but only once
// the arrays it reads are known not to be null.  The indices are validated on the device (run()).
// Codes, texts and WHICH message a caller gets when several apply are the entries' behaviour (tests/golden/api/entry_errors.json), the
// differences between the entries included.  Where the order differs for no reason it is kept and marked (*).
template <class T>
void check_request(const Request<T> &r, bool host)
{
    const auto fail = [](const std::string &msg) { throw RmError{RM_ERR_INVALID, msg}; };
    const char *null_in = "null input pointer", *mnk = "m, n, k must be positive", *mn = "m must not be negative and n must be positive";
    const std::string of_n = " with " + std::to_string(r.n) + " items)";
    const auto ld_covers_k = [&] { if (r.lda < (size_t)r.k || r.ldb < (size_t)r.k) fail("leading dimension smaller than k"); };
    const auto lds_covers_n = [&] {
        if (r.lds < (size_t)r.n) fail("leading dimension of the score matrix smaller than n (got " + std::to_string(r.lds) + of_n);
    };
    const auto K_in_1_n = [&](const char *name) {
        if (r.K < 1 || r.K > r.n) fail(std::string(name) + " must lie in [1, n] (got " + std::to_string(r.K) + of_n);
    };
    // the length of the test index array (read only behind the null check of `test_p`; the host form has looked at m by then)
    const auto nnz_test = [&] { return host ? (long long)r.test_p[r.m] : r.nnz_test; };
    // (deviation D8: the reference's walk would use gain 0 for a null Xtest_csr, :620, but its normalisation dereferences
    // the pointer, :870-874 -- a crash there, an error here)
    const auto ndcg_has_values = [&] { if (r.out[5] && !r.test_v) fail("NDCG requested without test values"); };
    // host form (a null array: lists have no test matrix and need no exclusion matrix)
    const auto index_pointers = [&] {
        for (const int *p : {r.train_p, r.test_p}) {
            if (!p) continue;
            int bad = p[0] < 0;
            for (int u = 0; u < r.m; u++) bad |= p[u + 1] < p[u];
            if (bad) {
                int u = 0;
                while (u < r.m && !(p[u] < 0 || p[u + 1] < p[u])) u++;
                fail(std::string("CSR index pointers of row ") + std::to_string(u) + " are negative or decreasing ("
                     + (p == r.train_p ? "X_train" : "X_test") + ")");
            }
        }
        if (r.train_p && r.train_p[r.m] > 0 && !r.train_i) fail("null train indices");
    };
    if (r.reco) {                                                    // lists, from factors or from scores
        if (r.m < 0 || r.n <= 0 || (!r.scores && r.k <= 0)) fail(r.scores ? mn : mnk);
        if (r.scores ? !r.S : (!r.A || !r.B)) fail(null_in);
        if (!r.topk_idx || !r.status) fail("null output pointer");
        if (r.scores) { lds_covers_n(); K_in_1_n("k_top"); }
        else { K_in_1_n("k_top"); ld_covers_k(); }                   // (*) the list length in front of the leading dimensions
        // (device form: the two entries used to ask these two in opposite orders; nnz < 0 and nnz > 0 exclude each other, so one order serves both)
        if (host) index_pointers();
        else if (r.nnz_train < 0) fail("negative length of the index array");
        else if (r.train_p && r.nnz_train > 0 && !r.train_i) fail(null_in);
        return;
    }
    if (r.scores) {                                                  // metrics from scores
        if (r.m < 0 || r.n <= 0) fail(mn);
        if (!r.S || !r.train_p || !r.test_p || (!r.test_i && nnz_test() > 0)) fail(null_in);
        lds_covers_n(); K_in_1_n("k_metrics"); ndcg_has_values();
        if (host) index_pointers();
        else if (r.nnz_train < 0 || r.nnz_test < 0) fail("negative length of an index array");
        else if (r.nnz_train > 0 && !r.train_i) fail("null train indices");
        return;
    }
    // metrics from factors, rm_rank_*.  (*) The host form names a negative m in front of a null pointer, the device form behind it; and
    // the device form leaves the lengths and a null train index array to the device's own checks of the CSR arrays.
    if (host && r.m < 0) fail(mnk);
    if (!r.A || !r.B || !r.train_p || !r.test_p || (!r.test_i && nnz_test() > 0)) fail(null_in);
    if (r.m <= 0 || r.n <= 0 || r.k <= 0) fail(mnk);
    if (r.K <= 0) fail("k_metrics must be positive");
    ld_covers_k();
    if (host) index_pointers();
    ndcg_has_values();
}

// a host-pointer request that has passed check_request: one device (the calling thread's current one), or the devices of rm_set_devices with
// contiguous user ranges [m g / G, m (g + 1) / G), one host thread + stream + workspace per shard, no exchange between the shards
template <class T>
void run_host_once(const Request<T> &h)
{
    std::vector<int> devs;
    { std::lock_guard<std::mutex> lk(g_dev_mu); devs = g_devices; }
    const unsigned long long tag = g_call_counter.fetch_add(1);
    SignalGuard guard;
    if (devs.size() <= 1) {
        int prev = -1;
        if (devs.size() == 1) { HIP_CHECK(hipGetDevice(&prev)); HIP_CHECK(hipSetDevice(devs[0])); }
        try { run_host_range<T>(h, 0, h.m, context(0), nullptr, nullptr, 0, tag); }
        catch (...) { if (prev >= 0) (void)hipSetDevice(prev); throw; }
        if (prev >= 0) HIP_CHECK(hipSetDevice(prev));
        guard.check();
        return;
    }
    const int G = (int)devs.size();
    SharedItems shared;
    shared.copies_pending = G - 1;
    std::vector<RmError> errs((size_t)G, RmError{RM_OK, ""});
    std::vector<std::thread> workers;
    std::vector<char> reached((size_t)G, 0);                          // shard g got as far as run_host_range (whose guard then owns the hand-shake)
    Ctx *first = nullptr;
    std::mutex first_mu;
    for (int g = 0; g < G; g++) {
        workers.emplace_back([&, g] {
            try {
                HIP_CHECK(hipSetDevice(devs[g]));
                Ctx &cx = context(g);
                if (g == 0) { std::lock_guard<std::mutex> lk(first_mu); first = &cx; }
                if (!cx.own_stream) HIP_CHECK(hipStreamCreateWithFlags(&cx.own_stream, hipStreamNonBlocking));
                const int u0 = (int)((long long)h.m * g / G), u1 = (int)((long long)h.m * (g + 1) / G);
                reached[g] = 1;
                run_host_range<T>(h, u0, u1, cx, cx.own_stream, &shared, g, tag);
            } catch (const RmError &e) { errs[g] = e; }
            catch (const std::bad_alloc &) { errs[g] = RmError{RM_ERR_NOMEM, "host allocation failed"}; }
            catch (const std::exception &e) { errs[g] = RmError{RM_ERR_HIP, e.what()}; }
            // (a shard that failed before it reached run_host_range's guard -- hipSetDevice, stream creation -- has to do the
            // guard's job here: shard 0 publishes the failure, the others give up their copy)
            if (errs[g].code != RM_OK) {
                std::lock_guard<std::mutex> sl(shared.mu);
                if (g == 0) { if (!shared.ready) { shared.ready = true; shared.failed = true; } }
                else if (!reached[g]) shared.copies_pending--;
                shared.cv.notify_all();
            }
        });
    }
    for (auto &w : workers) w.join();
    g_last_ctx = first;
    for (int g = 0; g < G; g++) if (errs[g].code != RM_OK && errs[g].code != RM_INTERNAL_UNSORTED) throw RmError{errs[g].code, "device " + std::to_string(devs[g]) + ": " + errs[g].msg};
    for (int g = 0; g < G; g++) if (errs[g].code == RM_INTERNAL_UNSORTED) throw errs[g];
    guard.check();
}

// The reference's callers hand over CSR rows with sorted column indices (recometrics/__init__.py:35-41 sorts them with SciPy, one
// thread walking every entry: 26-33 ms at BASELINE C2); here the rows are uploaded as they come and validated on the device (run():
// k_check_csr_*, ~40 us).  Only when some row turns out unsorted is a copy of the index / value arrays sorted on the host
// (csrc/rm_csr.cpp, multi-threaded, stable like SciPy's) and the call run again on the copy -- the caller's arrays are const.
// Recommendation lists have no test matrix: a row of zeros stands for its index pointers in the host-side bookkeeping of the batches
// (nothing of it reaches the device), and for the exclusion matrix's when there is none.
template <class T>
void run_host(Request<T> h, int nthreads)
{
    std::vector<int> zeros;
    if (h.reco) {
        zeros.assign((size_t)h.m + 1, 0);
        h.test_p = zeros.data();
        if (!h.train_p) h.train_p = zeros.data();
    }
    h.nnz_train = h.train_p[h.m]; h.nnz_test = h.test_p[h.m];
    try { run_host_once<T>(h); return; }
    catch (const RmError &e) { if (e.code != RM_INTERNAL_UNSORTED) throw; }
    if (h.topk_idx && !h.reco) throw RmError{RM_ERR_INVALID, "rm_rank_*: the CSR rows must be sorted (pos_rank is indexed by the caller's entry order)"};
    std::vector<int> tri(h.train_i, h.train_i + h.nnz_train), tei(h.test_i, h.test_i + h.nnz_test);
    std::vector<T> tev;
    if (h.test_v) tev.assign(h.test_v, h.test_v + h.nnz_test);
    int rc = rm_csr_sort_rows(h.train_p, tri.data(), nullptr, 0, h.m, nthreads);
    if (rc == RM_OK) rc = rm_csr_sort_rows(h.test_p, tei.data(), h.test_v ? (void *)tev.data() : nullptr, h.test_v ? (int32_t)sizeof(T) : 0, h.m, nthreads);
    if (rc != RM_OK) throw RmError{rc, "sorting a copy of the CSR rows failed"};
    h.train_i = tri.data(); h.test_i = tei.data(); h.test_v = h.test_v ? tev.data() : nullptr;
    try { run_host_once<T>(h); }
    catch (const RmError &e) { if (e.code != RM_INTERNAL_UNSORTED) throw; throw RmError{RM_ERR_INVALID, "CSR rows are not sorted"}; }
}

// device-pointer entry: the same fall-back through the host (the arrays are const device memory of the caller's: the sorted copies live in
// the context's workspace)
// (lists without an exclusion matrix: the index pointers become a row of zeros)
template <class T>
void run_dev(const Request<T> &r, hipStream_t stream)
{
    Call<T> c(r);
    Ctx &cx = context(0);
    std::lock_guard<std::mutex> lk(cx.mu);
    cx.acc[0] = cx.acc[1] = cx.acc[2] = cx.acc[3] = 0;
    if (r.reco && !r.train_p) {
        int *z = cx.ws.array<int>(WS_RECO_ZERO_P, (size_t)r.m + 1);
        if (cx.ev_valid) HIP_CHECK(hipStreamWaitEvent(stream, cx.done, 0));          // (an earlier call on another stream may still read it)
        HIP_CHECK(hipMemsetAsync(z, 0, sizeof(int) * ((size_t)r.m + 1), stream));
        c.train_p = z; c.train_i = z; c.nnz_train = 0;
    }
    try { run_call<T>(c, stream, cx); return; }
    catch (const RmError &e) { if (e.code != RM_INTERNAL_UNSORTED) throw; }
    const size_t m1 = (size_t)c.m + 1, nnz_tr = (size_t)std::max<long long>(c.nnz_train, 0), nnz_te = (size_t)std::max<long long>(c.nnz_test, 0);
    std::vector<int> trp(m1), tep(m1), tri(std::max<size_t>(nnz_tr, 1)), tei(std::max<size_t>(nnz_te, 1));
    std::vector<T> tev(c.test_v ? std::max<size_t>(nnz_te, 1) : 0);
    HIP_CHECK(hipMemcpyAsync(trp.data(), c.train_p, sizeof(int) * m1, hipMemcpyDeviceToHost, stream));
    if (c.test_p) HIP_CHECK(hipMemcpyAsync(tep.data(), c.test_p, sizeof(int) * m1, hipMemcpyDeviceToHost, stream));      // (none: recommendation lists -- `tep` stays zero)
    if (nnz_tr) HIP_CHECK(hipMemcpyAsync(tri.data(), c.train_i, sizeof(int) * nnz_tr, hipMemcpyDeviceToHost, stream));
    if (nnz_te) HIP_CHECK(hipMemcpyAsync(tei.data(), c.test_i, sizeof(int) * nnz_te, hipMemcpyDeviceToHost, stream));
    if (c.test_v && nnz_te) HIP_CHECK(hipMemcpyAsync(tev.data(), c.test_v, sizeof(T) * nnz_te, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    int rc = rm_csr_sort_rows(trp.data(), tri.data(), nullptr, 0, c.m, 0);
    if (rc == RM_OK) rc = rm_csr_sort_rows(tep.data(), tei.data(), c.test_v ? (void *)tev.data() : nullptr, c.test_v ? (int32_t)sizeof(T) : 0, c.m, 0);
    if (rc != RM_OK) throw RmError{rc, "sorting a copy of the CSR rows failed"};
    int *dtri = cx.ws.array<int>(WS_SORTED_TRI, std::max<size_t>(nnz_tr, 1));
    int *dtei = cx.ws.array<int>(WS_SORTED_TEI, std::max<size_t>(nnz_te, 1));
    T *dtev = c.test_v ? cx.ws.array<T>(WS_SORTED_TEV, std::max<size_t>(nnz_te, 1)) : nullptr;
    if (nnz_tr) HIP_CHECK(hipMemcpyAsync(dtri, tri.data(), sizeof(int) * nnz_tr, hipMemcpyHostToDevice, stream));
    if (nnz_te) HIP_CHECK(hipMemcpyAsync(dtei, tei.data(), sizeof(int) * nnz_te, hipMemcpyHostToDevice, stream));
    if (dtev && nnz_te) HIP_CHECK(hipMemcpyAsync(dtev, tev.data(), sizeof(T) * nnz_te, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));                         // (the vectors go out of scope below)
    c.train_i = dtri; c.test_i = dtei; c.test_v = dtev;
    try { run_call<T>(c, stream, cx); }
    catch (const RmError &e) { if (e.code != RM_INTERNAL_UNSORTED) throw; throw RmError{RM_ERR_INVALID, "CSR rows are not sorted"}; }
}

template <class T>
void debug_scores(const T *A, size_t lda, const T *B, size_t ldb, int m, int n, int k, T *out)
{
    typedef Prec<T> P;
    constexpr int GU = P::GU;
    if (!A || !B || !out || m <= 0 || n <= 0 || k <= 0) throw RmError{RM_ERR_INVALID, "bad argument"};
    const int NG = P::supported_ng(k);
    if (NG < 0) throw RmError{RM_ERR_UNSUPPORTED, P::limit()};
    Ctx &cx = context(0);
    std::lock_guard<std::mutex> lk(cx.mu);
    Workspace &ws = cx.ws;
    cx.packed.invalidate();                                  // the packed item image is overwritten below
    cx.split.invalidate();                                   // ... and so are the slot tables
    hipStream_t stream = nullptr;
    T *dA = ws.array<T>(WS_IN_A, (size_t)m * k);
    T *dB = ws.array<T>(WS_IN_B, (size_t)n * k);
    HIP_CHECK(hipMemcpy2DAsync(dA, sizeof(T) * k, A, sizeof(T) * lda, sizeof(T) * k, m, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpy2DAsync(dB, sizeof(T) * k, B, sizeof(T) * ldb, sizeof(T) * k, n, hipMemcpyHostToDevice, stream));
    const int n_groups = (m + GU - 1) / GU, n_ublocks = (n_groups + GROUPS_PER_BLOCK - 1) / GROUPS_PER_BLOCK;
    const int tiles_total = (n + TILE_ITEMS - 1) / TILE_ITEMS;
    int *slot_user = ws.array<int>(WS_SLOT_USER, (size_t)m);
    int *zeros = ws.array<int>(WS_DBG_ZEROS, (size_t)(m + 1 + n_groups));
    long long *grow = ws.array<long long>(WS_GROW, (size_t)n_groups);
    HIP_CHECK(hipMemsetAsync(zeros, 0, sizeof(int) * (size_t)(m + 1 + n_groups), stream));
    HIP_CHECK(hipMemsetAsync(grow, 0, sizeof(long long) * (size_t)n_groups, stream));
    hipLaunchKernelGGL(k_iota<int>, dim3(cdiv(m, 256)), dim3(256), 0, stream, slot_user, m);
    const long long bp_units = P::items_units(tiles_total, NG), ap_units = P::users_units(n_groups, NG);
    typename P::PackT *Bp = (typename P::PackT *)ws.get(WS_BP, 16 * (size_t)bp_units);
    typename P::PackT *Ap = (typename P::PackT *)ws.get(WS_AP, 16 * (size_t)ap_units);
    pack_operands(dA, (size_t)k, dB, (size_t)k, n, k, NG, TILE_ITEMS, slot_user, m, Ap, ap_units, Bp, bp_units, stream);
    T *dump = ws.array<T>(WS_DBG_DUMP, (size_t)m * n);
    const int K = 1;
    typename P::ListT *glists = ws.array<typename P::ListT>(WS_GLISTS, (size_t)n_ublocks * 8 * GU * (2 * K + 32));
    typename P::Args sa{};
    sa.n = n; sa.K = K; sa.ngt = NG; sa.n_slots = m; sa.n_groups = n_groups; sa.n_ublocks = n_ublocks; sa.n_splits = 1; sa.part_splits = 1;
    sa.tiles_total = tiles_total; sa.jmax = 0; sa.check_nan = 1; sa.Ap = (decltype(sa.Ap))Ap; sa.Bp = (decltype(sa.Bp))Bp;
    sa.slot_user = slot_user; sa.slot_chunk = zeros; sa.train_p = zeros; sa.train_i = zeros; sa.gj = zeros + m + 1; sa.grow = grow;
    sa.glists = glists; sa.dump = dump;
    sa.sync_off = (int)P::lds_b(NG);
    dispatch_sweep(false, true, false, 2, NG, dim3(n_ublocks), P::lds_b(NG) + SYNC_BYTES, stream, sa);
    HIP_CHECK(hipMemcpyAsync(out, dump, sizeof(T) * (size_t)m * n, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// ---- the entries: a request from the C arguments of its family, checked, run ------------------------------------------------------------
// The four families are two score sources -- factors, or the caller's score matrix -- times two kinds of request, and the host and the
// device form of a family state the same request: the device form adds the lengths of the index arrays (the host form reads them from the
// index pointers) and a stream, the host form the threads of the fall-back sort.
template <class T> Request<T> from_factors(const T *A, size_t lda, const T *B, size_t ldb, int k)
{
    Request<T> r;
    r.A = A; r.lda = lda; r.B = B; r.ldb = ldb; r.k = k;
    return r;
}
// 16-bit factors (recometrics_hip_half_factors.h): bit patterns, lda / ldb in 2-byte elements; the request is an fp32 request otherwise
inline Request<float> from_factors_half(const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int k, ScoreType type)
{
    Request<float> r;
    r.A = A; r.lda = lda; r.B = B; r.ldb = ldb; r.k = k; r.f_type = type;
    return r;
}
template <class T> Request<T> from_scores(const T *S, size_t lds)
{
    Request<T> r;
    r.S = S; r.lds = lds; r.scores = true;
    return r;
}
// 16-bit scores (recometrics_hip_half.h): bit patterns, lds in 2-byte elements; the request is an fp32 request otherwise
inline Request<float> from_scores_half(const uint16_t *S, size_t lds, ScoreType type)
{
    Request<float> r;
    r.S = S; r.s_type = type; r.lds = lds; r.scores = true;
    return r;
}
template <class T>
Request<T> metrics_request(Request<T> r, int m, int n, const int *train_p, const int *train_i, long long nnz_train,
                           const int *test_p, const int *test_i, const T *test_v, long long nnz_test,
                           int K, int cumulative, int noise, const std::array<T *, 10> &out,
                           int cold, int min_items_pool, int min_pos_test, unsigned long long seed)
{
    r.m = m; r.n = n;
    r.train_p = train_p; r.train_i = train_i; r.nnz_train = nnz_train;
    r.test_p = test_p; r.test_i = test_i; r.test_v = test_v; r.nnz_test = nnz_test;
    r.K = K; r.cumulative = cumulative != 0; r.noise = noise != 0;
    std::copy(out.begin(), out.end(), r.out);
    r.cold = cold != 0; r.min_items_pool = min_items_pool; r.min_pos_test = min_pos_test; r.seed = seed;
    return r;
}
// Recommendation lists (rm_recommend_*, rm_recommend_scores_*): the metric call's pipeline in its `reco` mode (k_classify without a test
// matrix, the sweep without positives, k_finalize_reco); every user is eligible.  `xp == NULL`: nothing is excluded.  From the caller's
// scores, up to ROW_TOPK_MAX_K items per list the row kernel of rm_rowtopk.hpp selects them while it reads the row; beyond (or under
// RM_DEBUG_NO_ROW_TOPK) k_score_rows -> k_select_topk -> k_finalize_reco.
template <class T>
Request<T> lists_request(Request<T> r, int m, int n, const int *xp, const int *xi, long long nnz, int K, int *idx, T *score, int *status)
{
    r.m = m; r.n = n;
    r.train_p = xp; r.train_i = xp ? xi : nullptr; r.nnz_train = nnz;
    r.K = K; r.cold = true; r.min_items_pool = 1; r.min_pos_test = 0;
    r.topk_idx = idx; r.topk_score = score; r.status = status; r.reco = true;
    return r;
}

template <class T> void host_entry(const Request<T> &r, int nthreads)
{
    if (r.m == 0) return;                                            // reference :428-437: no user, nothing written
    check_request(r, true);
    run_host<T>(r, nthreads > 0 ? nthreads : 0);                     // (host threads of the fall-back sort of unsorted CSR rows: 0 = all)
}
template <class T> void dev_entry(const Request<T> &r, void *stream)
{
    if (r.m == 0) return;
    check_request(r, false);
    run_dev<T>(r, (hipStream_t)stream);
}
// rm_rank_*: the factor metrics' host request with the ranking outputs, its AP / ROC-AUC / PR-AUC going to scratch arrays
template <class T> void rank_entry(Request<T> r, int *topk_idx, T *topk_score, long long *pos_rank, int *status)
{
    if (!topk_idx || !topk_score || !pos_rank || !status) throw RmError{RM_ERR_INVALID, "null output pointer"};     // (*) even with m == 0
    std::vector<T> ap((size_t)std::max(r.m, 1)), roc((size_t)std::max(r.m, 1)), pr((size_t)std::max(r.m, 1));
    r.out[3] = ap.data(); r.out[8] = roc.data(); r.out[9] = pr.data();
    r.topk_idx = topk_idx; r.topk_score = topk_score; r.pos_rank = pos_rank; r.status = status;
    host_entry<T>(r, 0);
}

} // namespace

// =====================================================================================================================
// C-ABI
// =====================================================================================================================
#define RM_HOST_ENTRY(SUFFIX, T)                                                                                        \
extern "C" int rm_calc_metrics_##SUFFIX(                                                                                \
    const T *A, size_t lda, const T *B, size_t ldb, int32_t m, int32_t n, int32_t k,                                    \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,                                                           \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const T *Xtest_csr,                                         \
    int32_t k_metrics, int cumulative, int break_ties_with_noise,                                                       \
    T *p_at_k, T *tp_at_k, T *r_at_k, T *ap_at_k, T *tap_at_k, T *ndcg_at_k, T *hit_at_k, T *rr_at_k,                   \
    T *roc_auc, T *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,                       \
    int32_t nthreads, uint64_t seed)                                                                                    \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<T>(metrics_request<T>(from_factors<T>(A, lda, B, ldb, k), m, n, Xtrain_csr_p, Xtrain_csr_i, 0,       \
                                         Xtest_csr_p, Xtest_csr_i, Xtest_csr, 0, k_metrics, cumulative,                 \
                                         break_ties_with_noise,                                                         \
                                         {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,     \
                                          roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, seed),   \
                      nthreads);                                                                                        \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_calc_metrics_dev_##SUFFIX(                                                                            \
    const T *A, size_t lda, const T *B, size_t ldb, int32_t m, int32_t n, int32_t k,                                    \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,                                        \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const T *Xtest_csr, int64_t nnz_test,                       \
    int32_t k_metrics, int cumulative, int break_ties_with_noise,                                                       \
    T *p_at_k, T *tp_at_k, T *r_at_k, T *ap_at_k, T *tap_at_k, T *ndcg_at_k, T *hit_at_k, T *rr_at_k,                   \
    T *roc_auc, T *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,                       \
    uint64_t seed, void *stream)                                                                                        \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<T>(metrics_request<T>(from_factors<T>(A, lda, B, ldb, k), m, n, Xtrain_csr_p, Xtrain_csr_i, nnz_train,\
                                        Xtest_csr_p, Xtest_csr_i, Xtest_csr, nnz_test, k_metrics, cumulative,           \
                                        break_ties_with_noise,                                                          \
                                        {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,      \
                                         roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, seed),    \
                     stream);                                                                                           \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_rank_##SUFFIX(                                                                                        \
    const T *A, size_t lda, const T *B, size_t ldb, int32_t m, int32_t n, int32_t k,                                    \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i,   \
    int32_t k_metrics, int break_ties_with_noise, int consider_cold_start, int32_t min_items_pool,                      \
    int32_t min_pos_test, uint64_t seed, int32_t *topk_idx, T *topk_score, int64_t *pos_rank, int32_t *status)          \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        rank_entry<T>(metrics_request<T>(from_factors<T>(A, lda, B, ldb, k), m, n, Xtrain_csr_p, Xtrain_csr_i, 0,       \
                                         Xtest_csr_p, Xtest_csr_i, nullptr, 0, k_metrics, 0, break_ties_with_noise, {}, \
                                         consider_cold_start, min_items_pool, min_pos_test, seed),                      \
                      topk_idx, topk_score, (long long *)pos_rank, status);                                             \
    });                                                                                                                 \
}

RM_HOST_ENTRY(f32, float)
RM_HOST_ENTRY(f64, double)

// metrics from the caller's score matrix: the host entry through HostRange (rows of S batch by batch), the device entry through run_dev
#define RM_SCORES_ENTRY(SUFFIX, T)                                                                                      \
extern "C" int rm_calc_metrics_scores_##SUFFIX(                                                                         \
    const T *S, size_t lds, int32_t m, int32_t n,                                                                       \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,                                                           \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const T *Xtest_csr,                                         \
    int32_t k_metrics, int cumulative,                                                                                  \
    T *p_at_k, T *tp_at_k, T *r_at_k, T *ap_at_k, T *tap_at_k, T *ndcg_at_k, T *hit_at_k, T *rr_at_k,                   \
    T *roc_auc, T *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads)     \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<T>(metrics_request<T>(from_scores<T>(S, lds), m, n, Xtrain_csr_p, Xtrain_csr_i, 0,                   \
                                         Xtest_csr_p, Xtest_csr_i, Xtest_csr, 0, k_metrics, cumulative, 0,              \
                                         {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,     \
                                          roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, 0),      \
                      nthreads);                                                                                        \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_calc_metrics_scores_dev_##SUFFIX(                                                                     \
    const T *S, size_t lds, int32_t m, int32_t n,                                                                       \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,                                        \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const T *Xtest_csr, int64_t nnz_test,                       \
    int32_t k_metrics, int cumulative,                                                                                  \
    T *p_at_k, T *tp_at_k, T *r_at_k, T *ap_at_k, T *tap_at_k, T *ndcg_at_k, T *hit_at_k, T *rr_at_k,                   \
    T *roc_auc, T *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream)         \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<T>(metrics_request<T>(from_scores<T>(S, lds), m, n, Xtrain_csr_p, Xtrain_csr_i, nnz_train,            \
                                        Xtest_csr_p, Xtest_csr_i, Xtest_csr, nnz_test, k_metrics, cumulative, 0,        \
                                        {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,      \
                                         roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, 0),       \
                     stream);                                                                                           \
    });                                                                                                                 \
}

RM_SCORES_ENTRY(f32, float)
RM_SCORES_ENTRY(f64, double)

#define RM_RECOMMEND_ENTRY(SUFFIX, T)                                                                                   \
extern "C" int rm_recommend_##SUFFIX(                                                                                   \
    const T *A, size_t lda, const T *B, size_t ldb, int32_t m, int32_t n, int32_t k,                                    \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,                                              \
    int32_t *idx, T *score, int32_t *status, int32_t nthreads)                                                          \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<T>(lists_request<T>(from_factors<T>(A, lda, B, ldb, k), m, n, Xexcl_csr_p, Xexcl_csr_i, 0, k_top,    \
                                       idx, score, status), nthreads);                                                  \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_dev_##SUFFIX(                                                                               \
    const T *A, size_t lda, const T *B, size_t ldb, int32_t m, int32_t n, int32_t k,                                    \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,                            \
    int32_t *idx, T *score, int32_t *status, void *stream)                                                              \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<T>(lists_request<T>(from_factors<T>(A, lda, B, ldb, k), m, n, Xexcl_csr_p, Xexcl_csr_i, nnz_excl,     \
                                      k_top, idx, score, status), stream);                                              \
    });                                                                                                                 \
}

RM_RECOMMEND_ENTRY(f32, float)
RM_RECOMMEND_ENTRY(f64, double)

#define RM_RECOMMEND_SCORES_ENTRY(SUFFIX, T)                                                                            \
extern "C" int rm_recommend_scores_##SUFFIX(                                                                            \
    const T *S, size_t lds, int32_t m, int32_t n,                                                                       \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,                                              \
    int32_t *idx, T *score, int32_t *status, int32_t nthreads)                                                          \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<T>(lists_request<T>(from_scores<T>(S, lds), m, n, Xexcl_csr_p, Xexcl_csr_i, 0, k_top,                \
                                       idx, score, status), nthreads);                                                  \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_scores_dev_##SUFFIX(                                                                        \
    const T *S, size_t lds, int32_t m, int32_t n,                                                                       \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,                            \
    int32_t *idx, T *score, int32_t *status, void *stream)                                                              \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<T>(lists_request<T>(from_scores<T>(S, lds), m, n, Xexcl_csr_p, Xexcl_csr_i, nnz_excl, k_top,          \
                                      idx, score, status), stream);                                                     \
    });                                                                                                                 \
}

RM_RECOMMEND_SCORES_ENTRY(f32, float)
RM_RECOMMEND_SCORES_ENTRY(f64, double)

// ---- 16-bit score matrices (include/recometrics_hip_half.h): the four from-scores entries of fp32 with S in IEEE binary16 / bfloat16 ----
#define RM_HALF_ENTRY(SUFFIX, TYPE)                                                                                     \
extern "C" int rm_calc_metrics_scores_##SUFFIX(                                                                         \
    const uint16_t *S, size_t lds, int32_t m, int32_t n,                                                                \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,                                                           \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,                                     \
    int32_t k_metrics, int cumulative,                                                                                  \
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k,   \
    float *rr_at_k, float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool,                     \
    int32_t min_pos_test, int32_t nthreads)                                                                             \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<float>(metrics_request<float>(from_scores_half(S, lds, TYPE), m, n, Xtrain_csr_p, Xtrain_csr_i, 0,   \
                                         Xtest_csr_p, Xtest_csr_i, Xtest_csr, 0, k_metrics, cumulative, 0,              \
                                         {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,     \
                                          roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, 0),      \
                      nthreads);                                                                                        \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_calc_metrics_scores_dev_##SUFFIX(                                                                     \
    const uint16_t *S, size_t lds, int32_t m, int32_t n,                                                                \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,                                        \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,                   \
    int32_t k_metrics, int cumulative,                                                                                  \
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k,   \
    float *rr_at_k, float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool,                     \
    int32_t min_pos_test, void *stream)                                                                                 \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<float>(metrics_request<float>(from_scores_half(S, lds, TYPE), m, n, Xtrain_csr_p, Xtrain_csr_i,       \
                                        nnz_train, Xtest_csr_p, Xtest_csr_i, Xtest_csr, nnz_test, k_metrics,            \
                                        cumulative, 0,                                                                  \
                                        {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,      \
                                         roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, 0),       \
                     stream);                                                                                           \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_scores_##SUFFIX(                                                                            \
    const uint16_t *S, size_t lds, int32_t m, int32_t n,                                                                \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,                                              \
    int32_t *idx, float *score, int32_t *status, int32_t nthreads)                                                      \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<float>(lists_request<float>(from_scores_half(S, lds, TYPE), m, n, Xexcl_csr_p, Xexcl_csr_i, 0,       \
                                               k_top, idx, score, status), nthreads);                                   \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_scores_dev_##SUFFIX(                                                                        \
    const uint16_t *S, size_t lds, int32_t m, int32_t n,                                                                \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,                            \
    int32_t *idx, float *score, int32_t *status, void *stream)                                                          \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<float>(lists_request<float>(from_scores_half(S, lds, TYPE), m, n, Xexcl_csr_p, Xexcl_csr_i,           \
                                              nnz_excl, k_top, idx, score, status), stream);                            \
    });                                                                                                                 \
}

RM_HALF_ENTRY(f16, SCORE_F16)
RM_HALF_ENTRY(bf16, SCORE_BF16)

// ---- 16-bit factor matrices (include/recometrics_hip_half_factors.h): the four factor entries of fp32 with A, B in IEEE binary16 / bfloat16 ----
#define RM_HALF_FACTOR_ENTRY(SUFFIX, TYPE)                                                                              \
extern "C" int rm_calc_metrics_##SUFFIX(                                                                                \
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,                      \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,                                                           \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,                                     \
    int32_t k_metrics, int cumulative, int break_ties_with_noise,                                                       \
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k,   \
    float *rr_at_k, float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool,                     \
    int32_t min_pos_test, int32_t nthreads, uint64_t seed)                                                              \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<float>(metrics_request<float>(from_factors_half(A, lda, B, ldb, k, TYPE), m, n, Xtrain_csr_p,        \
                                         Xtrain_csr_i, 0, Xtest_csr_p, Xtest_csr_i, Xtest_csr, 0, k_metrics,            \
                                         cumulative, break_ties_with_noise,                                             \
                                         {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,     \
                                          roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, seed),   \
                      nthreads);                                                                                        \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_calc_metrics_dev_##SUFFIX(                                                                            \
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,                      \
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,                                        \
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,                   \
    int32_t k_metrics, int cumulative, int break_ties_with_noise,                                                       \
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k,   \
    float *rr_at_k, float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool,                     \
    int32_t min_pos_test, uint64_t seed, void *stream)                                                                  \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<float>(metrics_request<float>(from_factors_half(A, lda, B, ldb, k, TYPE), m, n, Xtrain_csr_p,         \
                                        Xtrain_csr_i, nnz_train, Xtest_csr_p, Xtest_csr_i, Xtest_csr, nnz_test,         \
                                        k_metrics, cumulative, break_ties_with_noise,                                   \
                                        {p_at_k, tp_at_k, r_at_k, ap_at_k, tap_at_k, ndcg_at_k, hit_at_k, rr_at_k,      \
                                         roc_auc, pr_auc}, consider_cold_start, min_items_pool, min_pos_test, seed),    \
                     stream);                                                                                           \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_##SUFFIX(                                                                                   \
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,                      \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,                                              \
    int32_t *idx, float *score, int32_t *status, int32_t nthreads)                                                      \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        host_entry<float>(lists_request<float>(from_factors_half(A, lda, B, ldb, k, TYPE), m, n, Xexcl_csr_p,           \
                                               Xexcl_csr_i, 0, k_top, idx, score, status), nthreads);                   \
    });                                                                                                                 \
}                                                                                                                       \
extern "C" int rm_recommend_dev_##SUFFIX(                                                                               \
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,                      \
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,                            \
    int32_t *idx, float *score, int32_t *status, void *stream)                                                          \
{                                                                                                                       \
    return guarded([&] {                                                                                                \
        dev_entry<float>(lists_request<float>(from_factors_half(A, lda, B, ldb, k, TYPE), m, n, Xexcl_csr_p,            \
                                              Xexcl_csr_i, nnz_excl, k_top, idx, score, status), stream);               \
    });                                                                                                                 \
}

RM_HALF_FACTOR_ENTRY(f16, SCORE_F16)
RM_HALF_FACTOR_ENTRY(bf16, SCORE_BF16)

extern "C" int rm_debug_scores_f32(const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k, float *out)
{
    return guarded([&] { debug_scores<float>(A, lda, B, ldb, m, n, k, out); });
}

extern "C" int rm_debug_scores_f64(const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k, double *out)
{
    return guarded([&] { debug_scores<double>(A, lda, B, ldb, m, n, k, out); });
}

extern "C" int rm_has_openmp(void) { return 1; }

extern "C" const char *rm_last_error(void) { return g_err.c_str(); }

extern "C" int rm_device_count(void)
{
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) return 0;
    return c;
}

extern "C" int rm_set_device(int device)
{
    return guarded([&] { HIP_CHECK(hipSetDevice(device)); });
}

extern "C" int rm_set_devices(const int32_t *devices, int32_t n)
{
    return guarded([&] {
        if (n < 0 || (n > 0 && !devices)) throw RmError{RM_ERR_INVALID, "bad device list"};
        int count = 0;
        HIP_CHECK(hipGetDeviceCount(&count));
        std::vector<int> v;
        for (int i = 0; i < n; i++) {
            if (devices[i] < 0 || devices[i] >= count) throw RmError{RM_ERR_INVALID, "device " + std::to_string(devices[i]) + " does not exist (" + std::to_string(count) + " visible)"};
            v.push_back(devices[i]);
        }
        std::lock_guard<std::mutex> lk(g_dev_mu);
        g_devices = v;
    });
}

extern "C" int rm_get_devices(int32_t *devices, int32_t cap)
{
    std::lock_guard<std::mutex> lk(g_dev_mu);
    for (int i = 0; i < (int)g_devices.size() && i < cap; i++) devices[i] = g_devices[i];
    return (int)g_devices.size();
}

extern "C" void rm_request_interrupt(void) { g_interrupt = 1; }

extern "C" void rm_debug_reload_switches(void) { g_sw.load(); }

// test hooks over the table of sweep variants (rm_launch.hpp): host only, no device is touched
template <class Args> int debug_sweep_variants(int *out, int cap)
{
    int n = 0;
    for (int u = 0;; u++) {
        const SweepRows<Args> r = sweep_rows<Args>(u);
        if (!r.row) return n;
        for (int i = 0; i < r.n; i++, n++)
            if (out && n < cap) std::memcpy(out + 6 * n, &r.row[i].key, sizeof(SweepKey));
    }
}
template <class Args> int debug_find_sweep(int ng, int ngt, int auc, int dump, int lmode, int nsub, int spec, int *out6)
{
    SweepKey key;
    if (!sweep_key<Args>(ng, ngt, auc != 0, dump != 0, lmode, nsub, spec, key) || !find_sweep<Args>(key)) return -1;
    if (out6) std::memcpy(out6, &key, sizeof key);
    return 0;
}
extern "C" int rm_debug_sweep_variants(int elem_bytes, int *out, int cap)
{
    return elem_bytes == 4 ? debug_sweep_variants<SweepArgs>(out, cap) : elem_bytes == 8 ? debug_sweep_variants<Sweep64Args>(out, cap) : -1;
}
extern "C" int rm_debug_find_sweep(int elem_bytes, int ng, int ngt, int auc, int dump, int lmode, int nsub, int spec, int *out6)
{
    return elem_bytes == 4   ? debug_find_sweep<SweepArgs>(ng, ngt, auc, dump, lmode, nsub, spec, out6)
           : elem_bytes == 8 ? debug_find_sweep<Sweep64Args>(ng, ngt, auc, dump, lmode, nsub, spec, out6) : -1;
}
extern "C" int rm_debug_supported_ng(int elem_bytes, int k)
{
    return elem_bytes == 4 ? Prec<float>::supported_ng(k) : elem_bytes == 8 ? Prec<double>::supported_ng(k) : -1;
}
// the launch ledger of dispatch_sweep
template <class Args> int debug_sweep_launched(int *counts, int cap)
{
    const int n = debug_sweep_variants<Args>(nullptr, 0);
    for (int i = 0; counts && i < n && i < cap; i++) counts[i] = i < LEDGER_ROWS ? sweep_ledger<Args>()[i].load(std::memory_order_relaxed) : 0;
    return n;
}
extern "C" int rm_debug_sweep_launched(int elem_bytes, int *counts, int cap)
{
    return elem_bytes == 4 ? debug_sweep_launched<SweepArgs>(counts, cap) : elem_bytes == 8 ? debug_sweep_launched<Sweep64Args>(counts, cap) : -1;
}
extern "C" void rm_debug_sweep_launched_reset(void)
{
    for (auto &prec : g_sweep_launched) for (auto &c : prec) c.store(0, std::memory_order_relaxed);
}

// Test hook of the warm bounds (tests only; stated in _binding.TEST_HOOKS, not part of the header's API): the item ids of the lists the
// current device's context keeps for its next pass on the kept split are overwritten with ids[m][K] (host) -- the scores stay --, so
// that a test can hand k_hint_bounds advice no pass would leave.  RM_ERR_INVALID when the context keeps no lists of that shape.
template <class T> __global__ void k_set_list_ids(long long count, Entry<T> *lists, const int *ids)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) lists[i].idx = ids[i];
}
extern "C" int rm_debug_set_list_ids(const int32_t *ids, int32_t m, int32_t K)
{
    return guarded([&] {
        Ctx &cx = context(0);
        std::lock_guard<std::mutex> lk(cx.mu);
        const SplitCache &kept = cx.split;
        const Workspace::Buf buf = cx.ws.peek(WS_MERGED);
        const long long count = (long long)m * K;
        if (!ids || m <= 0 || K <= 0 || !kept.valid || !kept.lists.current(cx.ws) || kept.key.m != m || kept.key.K != K ||
            (size_t)count * (kept.key.elem == 4 ? sizeof(Entry<float>) : sizeof(Entry<double>)) > buf.bytes)
            throw RmError{RM_ERR_INVALID, "rm_debug_set_list_ids: the context keeps no lists of " + std::to_string(m) + " x " + std::to_string(K) + " entries"};
        HIP_CHECK(hipDeviceSynchronize());
        int *dev = nullptr;
        HIP_CHECK(hipMalloc((void **)&dev, sizeof(int) * (size_t)count));
        hipError_t e = hipMemcpy(dev, ids, sizeof(int) * (size_t)count, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            if (kept.key.elem == 4) hipLaunchKernelGGL(k_set_list_ids<float>, dim3(cdiv(count, 256)), dim3(256), 0, nullptr, count, (Entry<float> *)buf.ptr, (const int *)dev);
            else hipLaunchKernelGGL(k_set_list_ids<double>, dim3(cdiv(count, 256)), dim3(256), 0, nullptr, count, (Entry<double> *)buf.ptr, (const int *)dev);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipDeviceSynchronize();
        (void)hipFree(dev);
        HIP_CHECK(e);
    });
}

extern "C" int rm_get_timings(double *out, int n)
{
    Ctx *cx = g_last_ctx;
    if (!out || n <= 0 || !cx || !cx->ev_valid) return 0;
    float ms[4] = {0, 0, 0, 0};
    if (cx->ev_recorded) {
        if (hipEventSynchronize(cx->ev[EV_END]) != hipSuccess) return 0;
        cx->stage_ms(ms);
    }
    for (int i = 0; i < 4; i++) cx->timings[i] = cx->acc[i] + ms[i];
    const int cnt = n < Ctx::TM_COUNT ? n : Ctx::TM_COUNT;
    for (int i = 0; i < cnt && i < Ctx::TM_TIMED_SLOTS; i++) out[i] = cx->timings[i];
    if (cnt > Ctx::TM_TIMED_SLOTS) out[Ctx::TM_TIMED_SLOTS] = cx->timed_slots;
    if (cnt > Ctx::TM_TOTAL_SLOTS) out[Ctx::TM_TOTAL_SLOTS] = cx->total_slots;
    if (cnt > Ctx::TM_SPLIT_REUSED) out[Ctx::TM_SPLIT_REUSED] = cx->split_reused;
    if (cnt > Ctx::TM_HINTED) out[Ctx::TM_HINTED] = (cx->hints_ran && cx->ev_recorded && cx->hint_counts) ? cx->hint_counts[0] : 0;      // (EV_END is behind the counts' copy)
    return cnt;
}

extern "C" int rm_release_workspace(void)
{
    return guarded([&] {
        int dev = 0;
        HIP_CHECK(hipGetDevice(&dev));
        // (contexts are never destroyed, so the pointers stay valid; a context's mutex is NOT taken under g_ctx_mu: a running
        // call holds its context and may ask for a peer context, which takes g_ctx_mu -- the other order would deadlock)
        std::vector<Ctx *> mine;
        {
            std::lock_guard<std::mutex> lk(g_ctx_mu);
            for (auto &kv : g_ctx) if (kv.first.first == dev) mine.push_back(kv.second.get());
        }
        for (Ctx *c : mine) {
            std::lock_guard<std::mutex> cl(c->mu);
            c->ws.release();                  // (what the context remembers of the buffers' contents goes with their stamps)
        }
    });
}

// Test hooks of RM_DEBUG_WS_GUARD (Workspace).  The contexts of the current device, by slot; their mutexes are taken one by one
// (rm_release_workspace says why).
static std::vector<Ctx *> contexts_of_current_device()
{
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::vector<Ctx *> mine;
    std::lock_guard<std::mutex> lk(g_ctx_mu);
    for (auto &kv : g_ctx) if (kv.first.first == dev) mine.push_back(kv.second.get());
    return mine;
}
// Compares both zones of every live guarded buffer of the current device with WS_RED (of a tail longer than WS_CHECK_MAX its first
// WS_CHECK_MAX bytes) and returns the number of damaged zones, -1 on a HIP error (rm_last_error).  `msg` (cap bytes, may be NULL)
// receives "checked <buffers> buffers, <damaged> damaged zones" and a line per damaged zone:
//     damaged: buffer=<name> slot=<context slot> side=<head|tail> first=<offset> last=<offset> requested=<bytes> zone=<bytes>
// first / last: the first and the last damaged byte, counted from the payload's start (head: -256 .. -1) or from its end (tail: 0 ..).
extern "C" int rm_debug_ws_check(char *msg, int cap)
{
    int damaged = 0;
    const int rc = guarded([&] {
        HIP_CHECK(hipDeviceSynchronize());
        int checked = 0;
        std::string lines;
        std::vector<unsigned char> host;
        for (Ctx *c : contexts_of_current_device()) {
            std::lock_guard<std::mutex> cl(c->mu);
            for (int id = 0; id < WS_COUNT; id++) {
                const Workspace::Buf &b = c->ws.peek((WsBuf)id);
                if (!b.ptr || !b.guard) continue;
                checked++;
                if (b.lost_first >= 0) {              // (found when a larger request took that part of the tail zone over: Workspace::guard_grow)
                    damaged++;
                    lines += std::string("damaged: buffer=") + WS_NAMES[id] + " slot=" + std::to_string(c->slot) + " side=tail first=" + std::to_string(b.lost_first) +
                             " last=" + std::to_string(b.lost_last) + " requested=" + std::to_string(b.lost_req) + " zone=" + std::to_string(b.real - WS_ZONE - b.lost_req) + "\n";
                }
                for (int tail = 0; tail < 2; tail++) {
                    const size_t zone = tail ? b.tail_bytes() : WS_ZONE, len = std::min(zone, WS_CHECK_MAX);
                    const size_t at = tail ? WS_ZONE + b.req : 0;            // the zone's offset in the allocation
                    host.resize(len);
                    HIP_CHECK(hipMemcpy(host.data(), (const char *)b.base() + at, len, hipMemcpyDeviceToHost));
                    long long first = -1, last = -1;
                    for (size_t i = 0; i < len; i++)
                        if (host[i] != ws_pattern_byte(WS_RED, at + i)) { if (first < 0) first = (long long)i; last = (long long)i; }
                    if (first < 0) continue;
                    damaged++;
                    const long long origin = tail ? 0 : -(long long)WS_ZONE;
                    lines += std::string("damaged: buffer=") + WS_NAMES[id] + " slot=" + std::to_string(c->slot) + " side=" + (tail ? "tail" : "head") +
                             " first=" + std::to_string(origin + first) + " last=" + std::to_string(origin + last) +
                             " requested=" + std::to_string(b.req) + " zone=" + std::to_string(zone) + "\n";
                }
            }
        }
        const std::string text = "checked " + std::to_string(checked) + " buffers, " + std::to_string(damaged) + " damaged zones\n" + lines;
        if (msg && cap > 0) { const size_t n = std::min(text.size(), (size_t)cap - 1); std::memcpy(msg, text.data(), n); msg[n] = 0; }
    });
    return rc ? -1 : damaged;
}
// The positive control of that check: one byte of a zone of the live guarded buffer `buffer_id` (its place in RM_WS_BUFFERS; the
// first context of the current device that has one) is overwritten with the complement of its pattern byte.  tail = 0: the head
// zone; offset >= 0 counts from the zone's first byte, offset < 0 from behind its last one (-1: the last byte).  Only memory that
// Workspace::get allocated as a zone is touched.  RM_ERR_INVALID when there is no such buffer or the offset lies outside the zone.
extern "C" int rm_debug_ws_poke(int buffer_id, int tail, int offset)
{
    return guarded([&] {
        if (buffer_id < 0 || buffer_id >= WS_COUNT) throw RmError{RM_ERR_INVALID, "rm_debug_ws_poke: no buffer " + std::to_string(buffer_id)};
        HIP_CHECK(hipDeviceSynchronize());
        for (Ctx *c : contexts_of_current_device()) {
            std::lock_guard<std::mutex> cl(c->mu);
            const Workspace::Buf &b = c->ws.peek((WsBuf)buffer_id);
            if (!b.ptr || !b.guard) continue;
            const long long zone = (long long)(tail ? b.tail_bytes() : WS_ZONE), i = offset < 0 ? zone + offset : offset;
            if (i < 0 || i >= zone) throw RmError{RM_ERR_INVALID, std::string("rm_debug_ws_poke: ") + WS_NAMES[buffer_id] + ": offset " + std::to_string(offset) + " is outside the zone of " + std::to_string(zone) + " B"};
            const size_t at = (tail ? WS_ZONE + b.req : 0) + (size_t)i;
            HIP_CHECK(hipMemset((char *)b.base() + at, ws_pattern_byte(WS_RED, at) ^ 0xFF, 1));
            HIP_CHECK(hipDeviceSynchronize());
            return;
        }
        throw RmError{RM_ERR_INVALID, std::string("rm_debug_ws_poke: no live guarded buffer ") + WS_NAMES[buffer_id]};
    });
}
