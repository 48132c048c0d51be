/* recometrics_hip_half_factors.h -- the factor entries of recometrics_hip.h for factor matrices in 16-bit floating point.
 *
 * The models evaluated through rm_calc_metrics_* / rm_recommend_* usually keep their embedding tables in bfloat16 or IEEE binary16.
 * These eight entries read such tables where they lie -- half the bytes of the fp32 matrices in the caller's memory, in the uploads
 * and the fan-out between the shards of the host entries, and in every pass the device makes over A and B -- and widen every factor
 * EXACTLY to fp32 in registers:
 *   _f16   IEEE binary16: 1 sign, 5 exponent, 10 fraction bits; subnormals become fp32 normals (none is flushed);
 *   _bf16  bfloat16: the upper 16 bits of an fp32; subnormals stay (fp32) subnormals.
 * `A` and `B` hold the BIT PATTERNS (uint16_t) and share one type in a call; `lda` / `ldb` count 2-byte elements (>= k; a row may
 * start at any 2-byte address -- rows whose base and stride are multiples of 16 bytes take the 16-byte loads).  Everything else is
 * the _f32 entry of the same name: the parameter list, Xtest_csr, the ten outputs and the list scores in float.
 *
 * Contract: let WA, WB be the fp32 matrices with WA[u][f] == A[u][f], WB[i][f] == B[i][f].  Every entry here returns what its _f32
 * counterpart returns for WA, WB with lda / ldb counted in floats: the same status code, the same bits in the ten outputs, in idx,
 * score and status, the same RM_ERR_INVALID cases decided on the host before any device work, tie noise on or off with the same
 * seed.  A score is the k-ordered fp32 fma chain from +0 over the widened values, as everywhere in the library: nothing is ever
 * multiplied or accumulated in 16 bits.  m == 0 returns RM_OK and writes nothing.
 * Host entries: user batches, rm_set_devices shards, SIGINT, `nthreads` and rm_get_timings as for _f32; the resident copies of A and
 * B on the device hold 2-byte elements.  The only fp32 forms of the factors in device memory are the packed images of the _f32 call.
 * There is no 16-bit form of rm_rank_* or rm_debug_scores_*, of the outputs, or of fp64.
 */
#ifndef RECOMETRICS_HIP_HALF_FACTORS_H
#define RECOMETRICS_HIP_HALF_FACTORS_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* metrics: rm_calc_metrics_f32 / rm_calc_metrics_dev_f32 with A, B in 16 bits */
int rm_calc_metrics_f16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    int32_t nthreads, uint64_t seed);
int rm_calc_metrics_bf16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    int32_t nthreads, uint64_t seed);
int rm_calc_metrics_dev_f16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    uint64_t seed, void *stream);
int rm_calc_metrics_dev_bf16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb,
    int32_t m, int32_t n, int32_t k,
    const int32_t *Xtrain_csr_p, const int32_t *Xtrain_csr_i, int64_t nnz_train,
    const int32_t *Xtest_csr_p, const int32_t *Xtest_csr_i, const float *Xtest_csr, int64_t nnz_test,
    int32_t k_metrics, int cumulative, int break_ties_with_noise,
    float *p_at_k, float *tp_at_k, float *r_at_k, float *ap_at_k, float *tap_at_k,
    float *ndcg_at_k, float *hit_at_k, float *rr_at_k, float *roc_auc, float *pr_auc,
    int consider_cold_start, int32_t min_items_pool, int32_t min_pos_test,
    uint64_t seed, void *stream);

/* lists: rm_recommend_f32 / rm_recommend_dev_f32 with A, B in 16 bits */
int rm_recommend_f16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_bf16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_dev_f16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_dev_bf16(
    const uint16_t *A, size_t lda, const uint16_t *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xexcl_csr_p, const int32_t *Xexcl_csr_i, int64_t nnz_excl, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
