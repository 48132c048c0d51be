/* recometrics_hip_item_weights.h -- metrics and top-K lists of ITEM-ITEM models (EASE, SLIM, item-kNN): scores S = X_hist * W formed
 * from the history rows, never as a dense product.
 *
 * Such a model scores user u with the rows of a dense weight matrix W that u's history names.  Until now a caller had to form the
 * dense [users][items] product elsewhere (rm_calc_metrics_scores_*: 14.8 GB at MovieLens-20M, in somebody else's summation order) or
 * to pass dense(X_hist) as factors (rm_calc_metrics_*: 2 m n^2 flop for a 0.5 % dense operand).  These eight entries gather and
 * accumulate the rows of W on the device, a batch of users at a time, and run the from-scores stages on each batch.
 *
 * Scores.  W is row-major [n_in][n] with row stride `ldw` in elements (ldw >= n); n_in is the number of columns of the history matrix,
 * n the number of items (an item-item model has n_in == n; nothing assumes it).  The history is a CSR of m rows: hist_p[m + 1], ids
 * hist_i in [0, n_in), values hist_v (NULL: every value is 1).  For user u with stored entries (j_1, v_1) .. (j_h, v_h), ascending j:
 *     s_i = fma(v_h, W[j_h][i], .. fma(v_2, W[j_2][i], fma(v_1, W[j_1][i], +0)) ..)          in float / double
 * -- the library's k-ordered fma chain for A = dense(X_hist), B = W^T with its zero terms left out.  For a finite W every output is,
 * bit for bit, what rm_calc_metrics_* (break_ties_with_noise = 0) / rm_recommend_* return for that dense pair; the pair is never built.
 * Every stored entry is a step of the chain, an explicit zero and a repeated id included (nothing is summed beforehand); an entry that
 * is not stored is skipped, never multiplied by zero: a non-finite W[j][i] reaches exactly the users who have j.  A user without
 * history scores +0 everywhere.
 *
 * Everything behind the scores -- the train / exclusion matrix, the test matrix, k_metrics / k_top in [1, n], the ten outputs (a null
 * pointer = not requested), cumulative, cold start, the pool and positives' minima, idx / score / status of the lists -- is
 * rm_calc_metrics_scores_* / rm_recommend_scores_* (recometrics_hip.h), whose parameter lists these follow with `S, lds, m, n` replaced
 * by `W, ldw, n_in, m, n, hist_p, hist_i, hist_v` (and `nnz_hist` in the device form).  There is no tie noise and no seed.
 *
 * Validation.  RM_ERR_INVALID, decided on the host before any device work: null W / hist_p, null index pointers a metric call needs, a
 * null index array with entries to read, null idx / status of a list call, n <= 0, n_in <= 0, m < 0, ldw < n, k outside [1, n], a
 * negative nnz, NDCG without test values, index pointers that are negative or decrease (host form).  m == 0 returns RM_OK and writes
 * nothing.  The history rows are validated on the device like every other CSR input, with the column bound n_in: index pointers
 * beyond the arrays and ids outside [0, n_in) are RM_ERR_INVALID naming the row, decided before the gather indexes W; rows that are
 * merely unsorted (history, train or test) are sorted in a copy, values with them, and the call runs again.
 * Batches.  The user range is cut into batches sized by free device memory (the chunk of S plus what the stages behind it keep per
 * user; RM_BATCH_USERS caps them); results do not depend on the batch size.  An invalid train / test row is found by the batch that
 * holds it: a device call may have written the outputs of earlier batches by then, a host call hands nothing over.
 * Host entries upload W and the CSR arrays once, run the device form and download the outputs; they run on ONE device, the first of
 * rm_set_devices or the calling thread's current one (this source is not sharded), honour SIGINT between batches, and `nthreads` are
 * the threads of the fall-back sort.  The _dev entries take DEVICE pointers and are asynchronous on `stream` apart from the history's
 * verdict and one small plan read-back per batch.  rm_get_timings: out[12] is the gather kernel of the most recent batch, in ms.
 * Not here: 16-bit W, tie noise, several devices.
 */
#ifndef RECOMETRICS_HIP_ITEM_WEIGHTS_H
#define RECOMETRICS_HIP_ITEM_WEIGHTS_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int rm_calc_metrics_item_weights_f32(
    const float *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_item_weights_f64(
    const double *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_item_weights_dev_f32(
    const float *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v, int64_t nnz_hist,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_calc_metrics_item_weights_dev_f64(
    const double *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v, int64_t nnz_hist,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_recommend_item_weights_f32(
    const float *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_item_weights_f64(
    const double *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, int32_t nthreads);
int rm_recommend_item_weights_dev_f32(
    const float *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v, int64_t nnz_hist,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_item_weights_dev_f64(
    const double *W, size_t ldw, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v, int64_t nnz_hist,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
