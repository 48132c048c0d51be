/* recometrics_hip_item_weights_csr.h -- metrics and top-K lists of item-item models whose weight matrix is SPARSE (SLIM, item-kNN):
 * the entries of recometrics_hip_item_weights.h with W given as a CSR matrix.
 *
 * A SLIM row keeps a fraction of a percent of its entries and an item-kNN row its 50 to 200 neighbours; as a dense [n_in][n] matrix
 * such a model is 2.9 GB at the MovieLens-20M item count and cannot exist at a million items.  These eight entries form the scores
 * from the stored entries only.
 *
 * Scores.  W is a CSR of n_in rows over n columns: index pointers W_p[n_in + 1], column ids W_i in [0, n), values W_v in float / double.
 * The history is as in recometrics_hip_item_weights.h.  For user u with stored history entries (j_1, v_1) .. (j_h, v_h), ascending j,
 * the score of item i is the library's k-ordered chain
 *     acc = fma(v, W[j][i], acc)        over the j whose row STORES column i, in ascending j, from acc = +0
 * A stored zero is a step; an entry that W does not store is skipped, never multiplied; an item that no row of the history stores
 * scores +0.  Consequences:
 *   - For a finite W and finite history values every output equals, bit for bit, what rm_*_item_weights_* return for W densified, as
 *     long as no partial sum is a negative zero (a skipped fma(v, +0, acc) leaves every other acc unchanged, and the ranking reads -0
 *     as +0 anyway).
 *   - A non-finite stored W[j][i] reaches exactly the users who have j, and only item i -- sharper than the dense entries, where the
 *     whole row j is read.
 *
 * Rows of W.  Within a row the column ids must be strictly ascending once sorted: rows that are merely unsorted are sorted in a copy,
 * values with them, and the call runs again (as for the history, the train and the test matrix); a column id repeated inside one row,
 * an id outside [0, n) and index pointers that are negative, decrease or point beyond the arrays are RM_ERR_INVALID naming the row.
 * All of this is decided once per call, on the device, before the scores are formed.
 *
 * Everything else -- the history, the train / exclusion matrix, the test matrix, k_metrics / k_top in [1, n], the ten outputs,
 * cumulative, cold start, the minima, idx / score / status, batches sized by free memory (RM_BATCH_USERS), SIGINT between batches, one
 * device, `nthreads`, `stream` -- is recometrics_hip_item_weights.h, whose parameter lists these follow with `W, ldw` replaced by
 * `W_p, W_i, W_v` (and `nnz_W` next to `nnz_hist` in the device form).  There is no tie noise and no seed.
 *
 * Validation on the host, RM_ERR_INVALID before any device work and with the outputs untouched: null W_p / W_v, null W_i with entries
 * to read, a negative nnz_W, index pointers of W that are negative or decrease (host form), and everything the dense entries decide.
 * m == 0 returns RM_OK and writes nothing.  Host entries upload the three arrays once.
 * rm_get_timings: out[12] is the scores kernel of the most recent batch, in ms, whichever entry ran it.
 * Not here: 16-bit weights, implicit all-ones W_v, tie noise, several devices.
 */
#ifndef RECOMETRICS_HIP_ITEM_WEIGHTS_CSR_H
#define RECOMETRICS_HIP_ITEM_WEIGHTS_CSR_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int rm_calc_metrics_item_weights_csr_f32(
    const int32_t *W_p, const int32_t *W_i, const float *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_item_weights_csr_f64(
    const int32_t *W_p, const int32_t *W_i, const double *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_item_weights_csr_dev_f32(
    const int32_t *W_p, const int32_t *W_i, const float *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v, int64_t nnz_hist, int64_t nnz_W,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k, float *ndcg_at_k, float *hit_at_k, float *rr_at_k,
    float *roc_auc, float *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_calc_metrics_item_weights_csr_dev_f64(
    const int32_t *W_p, const int32_t *W_i, const double *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v, int64_t nnz_hist, int64_t nnz_W,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const double *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    double *p_at_k, double *tp_at_k, double *r_at_k, double *ap_at_k, double *tap_at_k, double *ndcg_at_k, double *hit_at_k, double *rr_at_k,
    double *roc_auc, double *pr_auc, int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_recommend_item_weights_csr_f32(
    const int32_t *W_p, const int32_t *W_i, const float *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_item_weights_csr_f64(
    const int32_t *W_p, const int32_t *W_i, const double *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, int32_t nthreads);
int rm_recommend_item_weights_csr_dev_f32(
    const int32_t *W_p, const int32_t *W_i, const float *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const float *hist_v, int64_t nnz_hist, int64_t nnz_W,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_item_weights_csr_dev_f64(
    const int32_t *W_p, const int32_t *W_i, const double *W_v, int32_t n_in, int32_t m, int32_t n,
    const int32_t *hist_p, const int32_t *hist_i, const double *hist_v, int64_t nnz_hist, int64_t nnz_W,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
