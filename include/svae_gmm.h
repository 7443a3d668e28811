/*
 * svae_gmm.h -- a diagonal-covariance Gaussian mixture over the content latents of a trained model, fitted by EM on the device
 * from a k-means result: responsibilities per point, a log-likelihood per fit, per-coordinate variances per class.  Every sum
 * has a fixed order, so the same buffers give the same bits on any run.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae_cluster.h stays, declaration for declaration, what its users and tests hold it to.  The reference has no
 * counterpart: it never groups the latents it infers.
 *
 * Data.  Points x are (N, D) floats, widened to double exactly.  weight (k), mean (k, D), var (k, D) are DOUBLES; resp (N, k)
 *   doubles, row-major, provided by the caller: it is also the staging area between the E and the M part.  label (N) int32,
 *   loglik_point (N) doubles (may be null).  Limits as svae_cluster.h: 1 <= D <= 64, 1 <= k <= 1024, k <= N < 2^31.
 *   All arithmetic is double with contraction off.  exp and log are the device library's; everything else is one IEEE operation
 *   per operator written below.
 *   Reductions over points use svae_cluster.h's two-level order: the chunk length P is 256, doubled until ceil(N / P) <= 1024;
 *     inside a chunk the values are added in point-index order onto +0, then the chunk totals in chunk-index order onto +0.
 *     No atomics anywhere.
 *
 * E part.  Component j is live iff weight[j] > 0.  Per live component iv[j,t] = 1 / var[j,t] and
 *     c[j] = log(weight[j]) - 0.5 * (sum_t log(var[j,t]) + D * log(2 pi)),
 *   the sum over t in index order from +0, D * log(2 pi) one product of (double)D and the double nearest log(2 pi).
 *   Per point i and live component j: q = sum_t (d * d) * iv[j,t] with d = (double)x[i,t] - mean[j,t], t in index order from +0;
 *   a[i,j] = c[j] - 0.5 * q.  A dead component has a = -inf and takes no part.
 *   m_i = max_j a[i,j]; label[i] starts at 0 and moves to j (walked upwards) only where a[i,j] > the best so far, strictly,
 *   starting from -inf.  s_i = sum_j exp(a[i,j] - m_i), j in index order from +0 (a dead component adds exp(-inf) = +0);
 *   resp[i,j] = exp(a[i,j] - m_i) / s_i, exactly 0 for a dead j; ll_i = m_i + log(s_i).
 *   Unassigned points.  A point with any non-finite coordinate -- and one that no live component scores above -inf -- is
 *   unassigned: label -1, an all-zero resp row, loglik_point 0; it enters no sum and no count.
 *   loglik = sum_i ll_i over the assigned points in the two-level order.
 *
 * M part, in the centred form (the variance never comes from E[x^2] - mu^2); mu is the INCOMING mean.
 *     R[j] = sum_i resp[i,j],  S1[j,t] = sum_i resp[i,j] * d,  S2[j,t] = sum_i resp[i,j] * (d * d),  d = (double)x[i,t] - mu[j,t],
 *   over the assigned points in the two-level order (a zero responsibility is skipped, which changes no bit).  Where
 *   !(R[j] > 0) the component is dead: weight[j] = 0, its mean and var are kept.  Otherwise delta = S1 / R,
 *   mean = mu + delta, var = max(S2 / R - delta * delta, 0) + reg, weight = R / (double)assigned.
 *
 * svae_gmm_record: ALL ZERO BYTES = a fresh record; 8-byte aligned device memory, so a replayed captured step advances it.
 *
 * Workspace.  svae_gmm_workspace_bytes(N, D, k) = 8 (C (2 + k (2 D + 1)) + k (D + 1) + 4) bytes with C = ceil(N / P): per chunk
 *   the sum of ll_i, the assigned count and per component S1, S2 (D each) and R; per component iv (D) and c; and four words that
 *   hold the record's deciding fields as the step found them.  0 for a geometry outside the limits.  `ws` is 256-byte aligned;
 *   one that is null, misaligned or too small is SVAE_E_WORKSPACE.  Its contents mean nothing between calls.
 *
 * svae_gmm_init: resp becomes the one-hot of label_in (an entry outside [0, k) or a non-finite point gives an all-zero row),
 *   then the M part runs with `mean` on input as mu -- the caller passes the k-means centres -- and writes weight, mean, var.
 *   The record is zeroed, then rec->assigned (points with finite coordinates) and rec->dead are set.  An empty k-means class
 *   comes out as a dead component.  Three launches.
 *
 * svae_gmm_step: the E part on the INCOMING parameters writes resp, label, loglik_point, rec->loglik, rec->assigned and
 *   rec->dead (the components with weight 0 in the parameters the call leaves).
 *   update == 0.  Nothing else is written: the final labelling call.  Three launches.
 *   update != 0.  Decided on the device: if rec->converged_at != 0 nothing further happens, the fit is frozen.  Else if
 *     rec->iterations >= 1 and loglik - rec->previous <= tol * |loglik|, rec->converged_at = rec->iterations and the parameters
 *     stay the ones that produced this loglik.  Else the M part is applied, rec->iterations += 1 and rec->previous = loglik.
 *     Four launches.  The caller enqueues a fixed number of steps and never reads a flag; once frozen, further steps are
 *     idempotent bit for bit.
 *
 * SVAE_E_INVALID: D outside 1..64, k outside 1..1024, N < k, N >= 2^31; a null x, weight, mean, var, resp or rec, a null
 *   label_in (init) or label (step); weight, mean, var, resp, rec or a non-null loglik_point not 8-byte aligned; reg not finite
 *   or not > 0; tol not finite or < 0.  A refused call leaves every buffer untouched.  All launches are filed under the
 *   `augment` kind of svae_profile_read.
 */
#ifndef SVAE_GMM_H
#define SVAE_GMM_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svae_gmm_record {
    int64_t iterations;   /* M parts applied so far */
    int64_t converged_at; /* the iteration count at which the gain first fell to tol |loglik|; 0 = not yet */
    int64_t assigned;     /* points with finite coordinates */
    int64_t dead;         /* components with weight 0 */
    double loglik;        /* of the last E part */
    double previous;      /* loglik of the E part before the last applied M part */
} svae_gmm_record;

size_t svae_gmm_workspace_bytes(int64_t N, int32_t D, int32_t k);
int svae_gmm_init(const float* x, int64_t N, int32_t D, int32_t k, const int32_t* label_in, double reg, double* weight, double* mean,
                  double* var, double* resp, svae_gmm_record* rec, void* ws, size_t ws_bytes, svae_stream_t stream);
int svae_gmm_step(const float* x, int64_t N, int32_t D, int32_t k, int32_t update, double reg, double tol, double* weight,
                  double* mean, double* var, double* resp, int32_t* label, double* loglik_point, svae_gmm_record* rec, void* ws,
                  size_t ws_bytes, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_GMM_H */
