/* recometrics_hip.h -- C-ABI of librecometrics_hip.so: the MI355X (gfx950) drop-in for the hot path of
 * david-cortes/recometrics.
 *
 * Boundary replaced (reference files, relative to the reference repository root):
 *   src/recometrics_signatures.hpp:46       bool get_has_openmp()
 *   src/recometrics_signatures.hpp:48-72    void calc_metrics_double(...30 parameters...)
 *   src/recometrics_signatures.hpp:74-98    void calc_metrics_float(...30 parameters...)
 * which recometrics/wrapper.pyx:282-304,381-403 (Cython) calls today and which src/Rwrapper.cpp:250-274 (Rcpp)
 * reaches through the template src/recometrics.hpp:359.  The entry points below keep the reference's PARAMETER
 * ORDER and meaning one-for-one; the differences are the ones a C-ABI needs: `bool` -> `int`, C linkage, and an
 * `int` status return (0 = ok) instead of C++ exceptions (std::bad_alloc / std::runtime_error in the reference,
 * src/recometrics.hpp:395-397,:171).  rm_last_error() returns the message for the calling thread.
 *
 * Ownership (same as the reference, src/recometrics.hpp:193-358): the caller owns every buffer; outputs are
 * pre-allocated by the binding ([m] or row-major [m x k_metrics] when `cumulative`); a NULL output pointer means
 * "metric not requested"; inputs are never modified; users that cannot be evaluated get NaN in every requested
 * output, so outputs need no initialisation.  CSR is 0-based int32.  The reference's callers sort the column indices of every row
 * first (recometrics/__init__.py:35-41, R/recometrics.R) and nobody checks them; here the arrays are VALIDATED on the device
 * before anything indexes by them: index pointers that are negative, decreasing or beyond the index array, and column indices
 * outside [0, n), are RM_ERR_INVALID with a message that names the row (on the CPU: a segfault); rows that are merely unsorted
 * are sorted by the library -- a copy, the caller's arrays are const -- and give the outputs of the sorted matrix (rm_rank_*
 * excepted: its pos_rank is indexed by the caller's entry order, unsorted rows are RM_ERR_INVALID there).  An item listed twice
 * in a row is tolerated as the reference tolerates it.
 * On a status other than RM_OK the contents of the output arrays are undefined, with one exception: RM_ERR_INTERRUPTED (below).
 * `nthreads` is accepted for signature compatibility (the device path has no host thread pool).  `seed` is USED:
 * with `break_ties_with_noise` the reference's tie-breaking noise -- std::mt19937(seed + user) through libstdc++'s
 * uniform_real_distribution, reference :528-534 -- is reproduced bit for bit (rm_noise.hpp; DESIGN.md, "tie noise"),
 * so pass the same seed the reference would get.
 * m == 0 returns RM_OK and writes nothing (the reference's loop over users does not run).  Xtest_csr_i may be NULL
 * when Xtest_csr_p[m] == 0.  Deviation: NDCG requested with Xtest_csr == NULL is RM_ERR_INVALID (the reference
 * dereferences the null pointer in its normalisation, :870-874).
 *
 * No torch / HIP types appear in any signature: pointers, sizes and scalars only.
 */
#ifndef RECOMETRICS_HIP_H
#define RECOMETRICS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes */
#define RM_OK 0
#define RM_ERR_INVALID 1     /* bad argument (null pointer, negative size, n or k == 0, k_metrics > n ...) */
#define RM_ERR_HIP 2         /* HIP runtime failure (message has the hipError string) */
#define RM_ERR_NOMEM 3       /* device or host allocation failed (the reference throws std::bad_alloc) */
#define RM_ERR_UNSUPPORTED 4 /* shape outside what the kernels are built for (message says which) */
#define RM_ERR_INTERRUPTED 5 /* SIGINT (or rm_request_interrupt) during a host-pointer call: "Error: procedure was interrupted."
                              * -- the std::runtime_error of src/recometrics.hpp:171.  Users of finished batches have their
                              * results; the rest of the output arrays is untouched, as in the reference (:488-489).  With
                              * break_ties_with_noise in fp32, users of finished batches whose exact (noise) evaluation had not
                              * run yet are set to NaN rather than left with their un-noised first-pass values */

/* replaces calc_metrics_float  (src/recometrics_signatures.hpp:74-98).  ALL pointers are HOST pointers. */
int rm_calc_metrics_f32(
    const float *A, size_t lda, const float *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    int32_t nthreads, uint64_t seed);

/* replaces calc_metrics_double (src/recometrics_signatures.hpp:48-72).  ALL pointers are HOST pointers. */
int rm_calc_metrics_f64(
    const double *A, size_t lda, const double *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k,
    double *ndcg_at_k, double *hit_at_k, double *rr_at_k, double *roc_auc, double *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    int32_t nthreads, uint64_t seed);

/* Same contracts with every pointer a DEVICE pointer on the current device (inputs already resident in HBM,
 * outputs written to HBM); `stream` is a hipStream_t passed as void* (NULL = default stream).  Asynchronous
 * apart from one small plan read-back; the caller synchronises the stream before reading the outputs.
 * `nnz_train` / `nnz_test` are the lengths of the index arrays (the host variants read them from indptr[m]). */
int rm_calc_metrics_dev_f32(
    const float *A, size_t lda, const float *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    uint64_t seed, void *stream);

int rm_calc_metrics_dev_f64(
    const double *A, size_t lda, const double *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k,
    double *ndcg_at_k, double *hit_at_k, double *rr_at_k, double *roc_auc, double *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    uint64_t seed, void *stream);

/* Metrics from the CALLER'S score matrix (no counterpart in the reference, whose scores are always dot products of two factor matrices): any model that has its
 * scores as a [users x items] array -- a two-tower model with a non-linear head, an item-kNN, a re-ranker, popularity with
 * business rules -- is evaluated by the same ten metrics.  The score of item i for user u is S[u * lds + i], exactly as given:
 * row-major, lds >= n, otherwise arbitrary (rows need not be 16-byte aligned); S is never modified.
 * Everything else is rm_calc_metrics_* with break_ties_with_noise = 0: eligibility (consider_cold_start, min_items_pool,
 * min_pos_test), candidates = the items outside the user's train row, the validity rules, the top-K walk, the NaN overrides,
 * ROC / PR-AUC, NDCG and `cumulative` layout, the ten outputs in the same order (NULL = not requested).  Equal scores are ordered
 * by item id (+0 == -0); there is no tie noise and no `seed`.  For factors whose k-ordered fma chain yields S, all ten outputs
 * are the same bits as rm_calc_metrics_* writes.
 * A score at a TRAIN item is never looked at: NaN or +-Inf there changes nothing.  A NaN among a user's candidates makes that user
 * NaN in every output; +-Inf among the candidates is treated as the factor call treats it (an infinite best score, or an infinite
 * score at the other end of what the request ranks -- the K-th place, the worst candidate with ROC-AUC or K >= candidates -- makes
 * the user NaN).
 * CSR arrays: validated as for the factor call (bad index pointers / indices: RM_ERR_INVALID naming the row; unsorted rows are
 * sorted in a copy).  m == 0 returns RM_OK and writes nothing.  RM_ERR_INVALID, decided on the host before any device work:
 * lds < n, n <= 0, k_metrics outside [1, n], S == NULL, NDCG requested with Xtest_csr == NULL.
 * rm_calc_metrics_scores_f32/f64: HOST pointers, through the machinery of the host-pointer metric call -- user batches sized so
 * that a batch's rows (two upload buffers and the masked copy) fit the device, rm_set_devices shards, SIGINT -> RM_ERR_INTERRUPTED
 * with the finished batches kept, `nthreads` for the fall-back sort; results depend neither on the device list nor on the
 * batch size.  rm_calc_metrics_scores_dev_f32/f64: DEVICE pointers on the current device, asynchronous on `stream` like
 * rm_calc_metrics_dev_*; one masked score row (budgeted as n rounded up to a multiple of 192 items, x the score's size) per user is kept in
 * device memory, and when the rows of m users do not fit a third of what is free the call answers RM_ERR_NOMEM with the bytes per row
 * and the largest m that fits in the message, as the k_metrics > 256 factor call does.  rm_get_timings covers all four; out[1]
 * then brackets the kernel that copies and masks the score rows (there is no sweep), out[6] is its blocks = evaluated users. */
int rm_calc_metrics_scores_f32(
    const float *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_scores_f64(
    const double *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k,
    double *ndcg_at_k, double *hit_at_k, double *rr_at_k, double *roc_auc, double *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_scores_dev_f32(
    const float *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_calc_metrics_scores_dev_f64(
    const double *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k,
    double *ndcg_at_k, double *hit_at_k, double *rr_at_k, double *roc_auc, double *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);

/* Ranking introspection (host pointers): the ordered top-K item ids / scores per user ([m x k_metrics], -1 / NaN
 * padded), the 1-based position of every test item in the user's FULL candidate ranking ([nnz_test], 0 when the
 * item is masked by the train row or the user is skipped) and status[m] (0 = ranked, 1 = user skipped).  These are
 * the quantities the parity contract pins bit-exactly (top-K index sets, hit counts, positive ranks). */
int rm_rank_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i,
    int32_t k_metrics, int break_ties_with_noise, int consider_cold_start,
    int32_t min_items_pool, int32_t min_pos_test, uint64_t seed,
    int32_t *topk_idx, float *topk_score, int64_t *pos_rank, int32_t *status);

int rm_rank_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i,
    int32_t k_metrics, int break_ties_with_noise, int consider_cold_start,
    int32_t min_items_pool, int32_t min_pos_test, uint64_t seed,
    int32_t *topk_idx, double *topk_score, int64_t *pos_rank, int32_t *status);

/* Top-K recommendation lists for EVERY user (no counterpart in the reference: the lists its metrics are computed from).
 * For each user u in [0, m): candidates = the items of [0, n) not listed in row u of the exclusion matrix (CSR, validated like
 * Xtrain_csr_*: unsorted rows are sorted in a copy, duplicates tolerated; Xexcl_csr_p == NULL excludes nothing and Xexcl_csr_i
 * is then ignored); score = the k-ordered fma chain from +0 of the metric call (bit-identical to rm_debug_scores_*); order =
 * score descending, then item id ascending (+0 and -0 are equal scores); no tie noise.
 * Outputs, row-major: idx[m x k_top] item ids, score[m x k_top] (may be NULL: ids only), status[m]:
 *   0  the first min(k_top, C) places of the row hold the list (C = number of candidates), the others -1 / NaN;
 *   1  the row excludes the whole catalogue: -1 / NaN everywhere;
 *   2  some candidate score is NaN or +-Inf: -1 / NaN everywhere.
 * 1 <= k_top <= n; m == 0 returns RM_OK and writes nothing.  For every user rm_rank_* (noise off) ranks, list and scores are
 * the same bits.  rm_recommend_f32/f64: HOST pointers, through the machinery of the host-pointer metric call (user batches,
 * rm_set_devices shards, SIGINT -> RM_ERR_INTERRUPTED with the finished batches kept, `nthreads` for the fall-back sort);
 * results depend neither on the device list nor on the batch size.  rm_recommend_dev_f32/f64: DEVICE pointers on the current
 * device, asynchronous on `stream` like rm_calc_metrics_dev_*; `nnz_excl` is the length of Xexcl_csr_i; k_top > 256 may answer
 * RM_ERR_NOMEM as the metric call does (one score row per user).  rm_get_timings covers both. */
int rm_recommend_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, int32_t nthreads);
int rm_recommend_dev_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_dev_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, void *stream);

/* The same lists from the CALLER'S score matrix: rm_recommend_* with the scores of rm_calc_metrics_scores_*.
 * Score of item i for user u = S[u * lds + i] as given (lds >= n, rows at any alignment; S is never modified).  Candidates = the
 * items outside row u of the exclusion matrix (validated as everywhere else: unsorted rows are sorted in a copy, bad index pointers /
 * indices are RM_ERR_INVALID naming the row; Xexcl_csr_p == NULL excludes nothing).  Order = score descending, then item id
 * ascending; -0 and +0 are equal scores and come out as +0; no tie noise.  idx / score (may be NULL) / status as rm_recommend_*:
 *   0  the first min(k_top, C) places hold the list, the rest -1 / NaN;   1  the row excludes the whole catalogue;
 *   2  some CANDIDATE score is NaN or +-Inf: -1 / NaN everywhere.  A score at an excluded item is never looked at.
 * RM_ERR_INVALID, decided on the host before any device work: S == NULL, lds < n, n <= 0, m < 0, k_top outside [1, n], idx or
 * status NULL, nnz_excl < 0.  m == 0 returns RM_OK and writes nothing.  Where S is the library's own k-ordered fma chain of some
 * A, B (rm_debug_scores_*), ids, scores and status are the bits rm_recommend_* writes.
 * rm_recommend_scores_f32/f64: HOST pointers, through the machinery of rm_calc_metrics_scores_* (user batches with two upload
 * buffers, rm_set_devices shards, SIGINT -> RM_ERR_INTERRUPTED with the finished batches kept, `nthreads` for the fall-back sort);
 * results depend neither on the device list nor on the batch size.  rm_recommend_scores_dev_f32/f64: DEVICE pointers on the
 * current device, asynchronous on `stream` like rm_recommend_dev_*.  Up to k_top = 1024 one kernel reads each row once and
 * selects the list on the way: NO score row is kept per user (the workspace is O(m) words plus the plan), so the call does not
 * answer RM_ERR_NOMEM for an m at which rm_calc_metrics_scores_dev_* does.  Beyond 1024 the masked rows are stored as there and the
 * call may answer RM_ERR_NOMEM with that call's message.  rm_get_timings covers all four: out[1] brackets the row kernel, out[6]
 * is its blocks. */
int rm_recommend_scores_f32(
    const float *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_scores_f64(
    const double *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, int32_t nthreads);
int rm_recommend_scores_dev_f32(
    const float *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_scores_dev_f64(
    const double *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, void *stream);

/* Dense score matrix out[m x n] (host) computed by the sweep's own MFMA contraction -- test hook that pins the
 * "bit-identical to the k-ordered fma chain" claim (reference src/recometrics.hpp:99-112). */
int rm_debug_scores_f32(const float *A, size_t lda, const float *B, size_t ldb,
                        int32_t m, int32_t n, int32_t k, float *out);
int rm_debug_scores_f64(const double *A, size_t lda, const double *B, size_t ldb,
                        int32_t m, int32_t n, int32_t k, double *out);

/* replaces get_has_openmp (src/recometrics_signatures.hpp:46): host threads are irrelevant here; always 1 so that
 * the reference's "built without multi-threading" warning (recometrics/__init__.py:524-529) never fires. */
int rm_has_openmp(void);

const char *rm_last_error(void);       /* message of the last failing call on this thread ("" if none) */
int rm_device_count(void);             /* visible HIP devices (0 when there is no GPU / driver) */
int rm_set_device(int device);         /* device used by subsequent calls on this thread */

/* Devices of the HOST-pointer calls (rm_calc_metrics_f32/f64, rm_rank_*) of this process: with n > 1 a call shards its users
 * inside the library -- contiguous ranges [m g / n, m (g + 1) / n), one host thread + stream + workspace per entry, the item
 * factors uploaded once and copied device-to-device, every shard's results written straight into the caller's arrays; no
 * exchange between shards (reference: the OpenMP loop over users, src/recometrics.hpp:428-437).  The same device may be
 * listed more than once.  n = 0 restores "the calling thread's current device".  Results do not depend on the list. */
int rm_set_devices(const int32_t *devices, int32_t n);
int rm_get_devices(int32_t *devices, int32_t cap);      /* returns the length of the list */

/* Asks the host-pointer calls in flight to stop at their next batch boundary (what SIGINT does during such a call,
 * src/recometrics.hpp:114-174); they return RM_ERR_INTERRUPTED. */
void rm_request_interrupt(void);

/* Test hook: the RM_DEBUG_* / RM_*_MB switches (tests and A/B timing; they choose among code paths with
 * identical results) are read from the environment once, when the library is loaded; this reads them again.  Not for use
 * while a call is running. */
void rm_debug_reload_switches(void);

/* Test hooks over the table of sweep-kernel instantiations; none of them touches a device.  elem_bytes = 4 /
 * 8 picks the precision (anything else returns -1).  A variant is six ints, the kernel's template arguments: ng (factor groups of
 * 8; 0 = the kernel that takes the count at run time), auc, dump, list mode (0 LDS, 1 HBM replace-the-minimum, 2 HBM append), item
 * sub-tiles per step (fp64: always 2), spec.
 *   rm_debug_sweep_variants  writes the first `cap` rows of the table to out[6 * cap] (out may be NULL) and returns the row count
 *   rm_debug_find_sweep      the variant that serves a request of the pipeline (ngt = the group count the operands were packed
 *                            for): 0 and the key in out6, or -1 where there is no kernel for it
 *   rm_debug_supported_ng    the factor-group count a call with k factors runs as */
int rm_debug_sweep_variants(int elem_bytes, int *out, int cap);
int rm_debug_find_sweep(int elem_bytes, int ng, int ngt, int auc, int dump, int lmode, int nsub, int spec, int *out6);
int rm_debug_supported_ng(int elem_bytes, int k);

/* Test hooks: the launch ledger.  Every successful launch of a sweep kernel is counted against its row of the table (one counter
 * per row and precision, safe across the host threads of one call; host only).
 *   rm_debug_sweep_launched        returns the row count and writes to counts[i], i < cap, the launches of row i -- in the order of
 *                                  rm_debug_sweep_variants -- since the last reset (counts may be NULL); -1 for an unknown precision
 *   rm_debug_sweep_launched_reset  zeroes the counters of both precisions */
int rm_debug_sweep_launched(int elem_bytes, int *counts, int cap);
void rm_debug_sweep_launched_reset(void);

/* Timings of the most recent successful call on this thread, milliseconds measured with HIP events on the call's
 * stream: out[0] plan+pack+positives, out[1] sweep kernel, out[2] finalize, out[3] whole device section;
 * out[4] = launches of the sweep kernel, out[5] = item splits, out[6] = sweep blocks, out[7] = dynamic LDS bytes,
 * out[8] = user lanes (slots) of the launch that out[1] brackets -- when the blocks of streamed users run beside the main
 * launch on a second stream, out[1] times the main launch only --, out[9] = user lanes of the whole call,
 * out[10] = 1 when the call ran on what the context kept of the previous call's train / test split (same arrays, same contents:
 * DESIGN.md section 1), 0 when it planned and validated the split itself, -1 for the calls that never reuse one,
 * out[11] = users whose top-K bound that call seeded from the lists the call before it left on the kept split (k_hint_bounds,
 * DESIGN.md section 2; 0 where there were none, or RM_DEBUG_NO_WARM_BOUNDS is set).
 * Forces a synchronisation of that stream.  Returns the number of values written (at most 12).
 * (Beside this API the library exports one hook for the tests of those bounds, not declared here: rm_debug_set_list_ids, stated in
 * recometrics_amd/_binding.py TEST_HOOKS and csrc/rm_lib.hip.) */
int rm_get_timings(double *out, int n);

/* Releases the cached device workspace of the current device. */
int rm_release_workspace(void);

/* Test hooks of RM_DEBUG_WS_GUARD: while that switch is set, every workspace buffer the library allocates lies
 * between two red zones of a fixed pattern -- the tail zone starts at the byte count of the largest request the allocation has served --
 * and its payload is poisoned.
 *   rm_debug_ws_check  synchronises the current device and compares the zones of every live guarded buffer of its contexts with the
 *                      pattern (of a tail zone longer than 1 MiB the first 1 MiB).  Returns the number of damaged zones, -1 on an
 *                      error (rm_last_error).  msg (cap bytes, may be NULL) receives "checked <buffers> buffers, <zones> damaged
 *                      zones" and then one line per damaged zone: "damaged: buffer=<name> slot=<context slot> side=<head|tail>
 *                      first=<offset> last=<offset> requested=<bytes> zone=<bytes>", the offsets of the first and the last damaged
 *                      byte counted from the payload's start (head: -256 .. -1) or from its end (tail: 0 ..)
 *   rm_debug_ws_poke   the positive control: overwrites ONE byte of a zone of the live guarded buffer `buffer_id` (its place in the
 *                      list RM_WS_BUFFERS of csrc/rm_lib.hip): tail = 0 the head zone, else the tail zone; offset >= 0 from the zone's
 *                      first byte, < 0 from behind its last one.  It touches only memory allocated as a zone.  RM_ERR_INVALID when
 *                      no such buffer is live or the offset lies outside the zone */
int rm_debug_ws_check(char *msg, int cap);
int rm_debug_ws_poke(int buffer_id, int tail, int offset);

/* ---- train / test splitting (host only; "next" row N3) ------------------------------------------------------------
 * Replaces split_data_selected_users_{float,double}, split_data_separate_users_* and split_data_joined_users_*
 * (src/recometrics_signatures.hpp:100-220), which hand their results back in std::vector& parameters; a C-ABI returns an
 * opaque result instead.  mode 0 = every row is split ("all"), 1 = separated (test users drawn at random; outputs
 * rem / train / test / users_test), 2 = joined (train = [train of the test users ; remaining users]).  `n_users_test`,
 * `consider_cold_start`, `min_items_pool`, `min_pos_test` are ignored in mode 0.  Results are bit-identical to the
 * reference's for the same seed (both consume std::mt19937 through std::shuffle in the same order).
 * Arrays of a result, `which`: 0-2 train (indptr, indices, values), 3-5 test, 6-8 rem, 9 users_test. */
int rm_split_f32(const int32_t *X_csr_p, const int32_t *X_csr_i, const float *X_csr, int32_t m, int32_t n, int mode,
                 int32_t n_users_test, double test_fraction, int consider_cold_start, int32_t min_items_pool,
                 int32_t min_pos_test, uint64_t seed, void **result);
int rm_split_f64(const int32_t *X_csr_p, const int32_t *X_csr_i, const double *X_csr, int32_t m, int32_t n, int mode,
                 int32_t n_users_test, double test_fraction, int consider_cold_start, int32_t min_items_pool,
                 int32_t min_pos_test, uint64_t seed, void **result);
int64_t rm_split_size(const void *result, int which);           /* number of elements of array `which` (-1 = bad argument) */
int rm_split_copy(const void *result, int which, void *dst);    /* copies array `which` into dst (caller-sized) */
void rm_split_free(void *result);
const char *rm_split_last_error(void);

/* ---- CSR normalisation in front of the metric call (host only) --------------------------------------------------------
 * Replaces the `X.sort_indices()` of the reference's Python caller (recometrics/__init__.py:35-41 `_as_csr`, applied to X_train
 * and X_test at :553-562; the R caller's `sort_sparse_indices`, R/recometrics.R): SciPy's single-threaded pass over every
 * stored entry becomes a pass over row ranges on `nthreads` host threads (<= 0: all).
 * rm_csr_rows_sorted: 1 = the column indices of every row ascend (equal neighbours allowed, as SciPy's has_sorted_indices),
 *   0 = some row does not, -1 = bad argument.  rm_csr_sort_rows: sorts every row's (index, value) pairs by index, in place,
 *   stable; `values` are `value_bytes` (0 = no values, 4, 8) wide. */
int rm_csr_rows_sorted(const int32_t *indptr, const int32_t *indices, int32_t m, int32_t nthreads);
int rm_csr_sort_rows(const int32_t *indptr, int32_t *indices, void *values, int32_t value_bytes, int32_t m, int32_t nthreads);

#ifdef __cplusplus
}
#endif
#endif /* RECOMETRICS_HIP_H */
