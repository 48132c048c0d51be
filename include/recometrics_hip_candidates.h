/* recometrics_hip_candidates.h -- top-K lists from per-user CANDIDATE SETS: rank these few hundred items for this user.
 *
 * rm_recommend_* ranks the whole catalogue minus an exclusion row.  A retrieval stage asks the opposite question: an ANN index or a
 * first-stage model hands over 100 - 2,000 candidates per user, an evaluation protocol fixes "positives + N sampled negatives", a
 * re-ranker scores a shortlist.  These four entries gather the candidates' item rows, score them and select the list in one kernel
 * (a block per user; no sweep over the catalogue, no score row in memory): the work is C gathered rows per user, not n.
 *
 * Candidates.  The candidates of user u are the DISTINCT item ids in row u of the candidate CSR (int32; Xcand_csr_p[m + 1], ids in
 * [0, n)).  An id listed twice counts once.  C = the number of distinct ids of the row.  Rows may be of any length.
 * Scores, order, output.  The score of (u, i) is the library's k-ordered fma chain from +0 over A[u], B[i]: the bits rm_recommend_*
 * writes for that pair.  Order: score descending, then item id ascending; -0 and +0 are equal and come out as +0; there is no tie
 * noise.  idx[m][k_top], score[m][k_top] (may be NULL), status[m] as rm_recommend_*:
 *   0  the first min(k_top, C) places hold the list, the rest -1 / NaN;
 *   1  the row is empty (-1 / NaN everywhere);
 *   2  some CANDIDATE's score is NaN or +-Inf (-1 / NaN everywhere).
 * A non-finite factor row of an item that is not the user's candidate affects nothing for that user.  Hence, for the exclusion
 * matrix that is the complement of the candidate rows, rm_recommend_* and these entries write the same ids, score bits and status.
 * Validation.  RM_ERR_INVALID, decided on the host before any device work: null A / B / Xcand_csr_p / idx / status, n <= 0, k <= 0,
 * m < 0, k_top < 1, lda / ldb < k, nnz_cand < 0, a null Xcand_csr_i with entries to read.  m == 0 returns RM_OK and writes nothing.
 * k_top may exceed a row's C (the padded case) and n, but not 1,024: beyond, RM_ERR_UNSUPPORTED.  Index pointers that decrease and
 * ids outside [0, n) are RM_ERR_INVALID naming the row, decided before any kernel indexes B by such an id; rows that are merely
 * unsorted are sorted in a copy and the call runs again.
 * Host entries: user batches, rm_set_devices shards, SIGINT, `nthreads` (the fall-back sort) and rm_get_timings (out[1]: the kernel,
 * out[6]: its blocks) as for rm_recommend_*; results depend neither on the batch size nor on the device list.  The _dev entries take
 * DEVICE pointers and are asynchronous on `stream`.
 * Not here: an exclusion matrix next to the candidates (the candidate row IS the pool: filter it beforehand), 16-bit factors.  The
 * metrics over the same pools are recometrics_hip_candidate_metrics.h's.
 */
#ifndef RECOMETRICS_HIP_CANDIDATES_H
#define RECOMETRICS_HIP_CANDIDATES_H

#include "recometrics_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int rm_recommend_candidates_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, int32_t nthreads);
int rm_recommend_candidates_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, int32_t nthreads);
int rm_recommend_candidates_dev_f32(
    const float *A, size_t lda, const float *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int64_t nnz_cand, int32_t k_top,
    int32_t *idx, float *score, int32_t *status, void *stream);
int rm_recommend_candidates_dev_f64(
    const double *A, size_t lda, const double *B, size_t ldb, int32_t m, int32_t n, int32_t k,
    const int32_t *Xcand_csr_p, const int32_t *Xcand_csr_i, int64_t nnz_cand, int32_t k_top,
    int32_t *idx, double *score, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif

#endif
