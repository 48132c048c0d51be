/* recometrics_hip_half.h -- the from-scores entries of recometrics_hip.h for score matrices in 16-bit floating point.
 *
 * The models evaluated through rm_calc_metrics_scores_* / rm_recommend_scores_* usually emit their scores in bfloat16 or IEEE
 * binary16.  These eight entries read such a matrix where it lies -- half the bytes of the fp32 matrix in memory, in the upload of
 * the host entries and in the one pass the device makes over it -- and widen every score EXACTLY to fp32 in registers:
 *   _f16   IEEE binary16: 1 sign, 5 exponent, 10 fraction bits; subnormals become fp32 normals (none is flushed);
 *   _bf16  bfloat16: the upper 16 bits of an fp32; subnormals stay (fp32) subnormals.
 * `S` holds the BIT PATTERNS (uint16_t), `lds` counts 2-byte elements (lds >= n; a row may start at any 2-byte address).
 * Everything else is the _f32 entry of the same name: the parameter list, Xtest_csr, the ten outputs and the list scores in
 * float.
 *
 * Contract: let W be the fp32 matrix with W[u][i] == S[u][i].  Every entry here returns what its _f32 counterpart returns for W
 * with lds counted in floats: the same status code, the same bits in the ten outputs, in idx, score and status, the same
 * RM_ERR_INVALID cases decided on the host before any device work, -0 equal to +0 and handed back as +0, NaN / +-Inf among a
 * user's candidates as there (the user NaN; list status 2), no look at a score at a train / excluded item, no tie noise.
 * m == 0 returns RM_OK and writes nothing.
 * Host entries: user batches, rm_set_devices shards, SIGINT, `nthreads` and rm_get_timings as for _f32; the two upload buffers hold
 * 2-byte scores, so a batch is about a quarter larger than the fp32 call's.  Device entries: lists up to k_top = 1024 keep no row
 * per user and never answer RM_ERR_NOMEM; beyond, and for metrics, the masked row that is kept is fp32 -- the bytes per row in the
 * RM_ERR_NOMEM message are the fp32 call's.
 * The 16-bit form of the factor entries is recometrics_hip_half_factors.h; there is none of the outputs or of fp64.
 */
#ifndef RECOMETRICS_HIP_HALF_H
#define RECOMETRICS_HIP_HALF_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* metrics: rm_calc_metrics_scores_f32 / rm_calc_metrics_scores_dev_f32 with S in 16 bits */
int rm_calc_metrics_scores_f16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_scores_bf16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, int32_t nthreads);
int rm_calc_metrics_scores_dev_f16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);
int rm_calc_metrics_scores_dev_bf16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test, void *stream);

/* lists: rm_recommend_scores_f32 / rm_recommend_scores_dev_f32 with S in 16 bits */
int rm_recommend_scores_f16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_scores_bf16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_scores_dev_f16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_scores_dev_bf16(
    const uint16_t *S, size_t lds, int32_t m, int32_t n,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
