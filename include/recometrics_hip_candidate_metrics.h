/* recometrics_hip_candidate_metrics.h -- the ten metrics over per-user CANDIDATE SETS: leave-one-out HR@10 / NDCG@10 over 1 + 99 items,
 * sampled-negative evaluation of a large catalogue, the metrics of a re-ranker over an ANN shortlist.
 *
 * rm_recommend_candidates_* (recometrics_hip_candidates.h) ranks a user's few hundred candidates in one kernel and returns the list.
 * These four entries rank the same pool the same way and return what rm_calc_metrics_* returns: the work is C gathered item rows per
 * user, not a sweep over n items, and no train matrix of m (n - C) entries is ever built.
 *
 * Contract.  The pool of user u is the set of DISTINCT ids of row u of the candidate CSR (int32; Xcand_csr_p[m + 1], ids in [0, n);
 * an id listed twice counts once; C of them).  Scores and order are rm_recommend_candidates_*': the k-ordered fma chain from +0,
 * score descending then item id ascending, -0 counts as +0; there is no tie noise and no seed.  Every output -- P / TP / R / AP / TAP /
 * NDCG / Hit / RR @K (K values per user when `cumulative`), ROC-AUC, PR-AUC; a null pointer = not requested -- is what rm_calc_metrics_*
 * writes for the same A, B and X_test with the train matrix that is the COMPLEMENT of the candidate rows, break_ties_with_noise = 0
 * and consider_cold_start = 1: the eligibility rules (with C in the place of n - ntr), the validity rule without noise, the NaN
 * overrides, the quirks and deviations of DESIGN.md section 4.  n is the catalogue's size and enters only through ntr = n - C.
 * Two cases the complement leaves open:
 *   * a test item of user u that is NOT among u's candidates: every requested output of u is NaN, as for an ineligible user (neither
 *     an error nor a silent miss);
 *   * a candidate row of more than 2,048 entries, duplicates included: RM_ERR_UNSUPPORTED naming the first such row, decided before
 *     the metric kernel is launched; no output is written.  A full ranking of a longer row is the catalogue sweep's job
 *     (rm_calc_metrics_* with the complement as X_train).
 * k_metrics may be up to 1,024 (beyond: RM_ERR_UNSUPPORTED) and may exceed a row's C and n.
 * Validation.  RM_ERR_INVALID, decided on the host before any device work: null A / B / Xcand_csr_p / Xtest_csr_p, null Xtest_csr_i
 * with entries to read, n <= 0, k <= 0, m < 0, k_metrics < 1, lda / ldb < k, a negative nnz, a null Xcand_csr_i with entries to read,
 * NDCG without test values.  m == 0 returns RM_OK and writes nothing.  Index pointers that decrease and ids outside [0, n), in either
 * CSR, are RM_ERR_INVALID naming the row, decided before any kernel indexes B by such an id; rows that are merely unsorted are sorted
 * in a copy and the call runs again.
 * Host entries: user batches, rm_set_devices shards, SIGINT, `nthreads` (the fall-back sort) and rm_get_timings (out[1]: the two
 * launches of the metric kernel, out[6]: their blocks) as for rm_recommend_candidates_*; results depend neither on the batch size nor
 * on the device list.  The _dev entries take DEVICE pointers and are asynchronous on `stream` apart from one small plan read-back.
 * Not here: rows beyond 2,048 entries, tie noise, 16-bit factors, an exclusion matrix next to the candidates.
 */
#ifndef RECOMETRICS_HIP_CANDIDATE_METRICS_H
#define RECOMETRICS_HIP_CANDIDATE_METRICS_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int rm_calc_metrics_candidates_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_candidates_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_candidates_dev_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int64_t nnz_cand,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_calc_metrics_candidates_dev_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int64_t nnz_cand,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int32_t min_items_pool, int32_t min_pos_test, void *stream);

#ifdef __cplusplus
}
#endif

#endif
