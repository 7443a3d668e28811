/*
 * svae_pca.h -- principal axes of the content latents of a trained model, on the device: the mean and covariance of (N, D)
 * points, globally or per group, the eigen-decomposition of every covariance by cyclic Jacobi, and every point's coordinates
 * along the axes of its group.  Every sum and every rotation has a fixed order, so the same buffers give the same bits on any
 * run, any device and any stream.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae_cluster.h and svae_gmm.h stay, declaration for declaration, what their users and tests hold them to.  The
 * reference has no counterpart: it shows latent traversals and never computes the axes to walk along.
 *
 * Data.  Points x are (N, D) floats, widened to double exactly.  group is (N) int32 or NULL; G is the number of groups.  NULL
 *   puts every point in group 0 and requires G == 1.  A point whose entry is outside [0, G), and a point with any non-finite
 *   coordinate, is in NO group: it enters no sum and no count.  count (G) int64; mean (G, D), cov (G, D, D), eigenvalues (G, D),
 *   components (G, D, D), off_norm (G) and proj (N, P) are DOUBLES, row-major; sweeps (G) int32.
 *   All arithmetic is double with contraction off: one IEEE operation per operator written below, sqrt the correctly rounded
 *   one.  No atomics anywhere.
 *   Reductions over points use svae_cluster.h's two-level order, which depends on N only: the chunk length L is 256, doubled
 *     until ceil(N / L) <= 1024; chunk c holds the points [c L, min(N, (c+1) L)).  Inside a chunk the values of a group's points
 *     are added in point-index order onto +0, then the chunk totals in chunk-index order onto +0.  A point that does not take
 *     part is skipped, not added as 0.
 *   Limits.  1 <= D <= 64, 1 <= G <= 1024, G D (D + 1) / 2 <= 32768, 1 <= N < 2^31.
 *
 * Workspace (svae_pca_moments only).  svae_pca_workspace_bytes(N, D, G) = 8 (C G (1 + D + D (D + 1) / 2) + ceil(N / 2)) bytes
 *   with C = ceil(N / L): per chunk and group the member count, the D coordinate sums and the D (D + 1) / 2 centred products
 *   (at most 256 MiB under the limits), and one int32 per point, the group it counts in.  0 for a geometry outside the limits.
 *   `ws` is 256-byte aligned; one that is null, misaligned or too small is SVAE_E_WORKSPACE.  Its contents mean nothing between
 *   calls.
 *
 * svae_pca_moments: two passes, four launches.
 *   Pass 1.  count[g] = the number of points in group g; S[g,t] = the sum of (double)x[i,t] over them in the two-level order;
 *     mean[g,t] = S[g,t] / (double)count[g], and +0 where count[g] == 0.  (With one member the mean is that point, exactly.)
 *   Pass 2.  M[g,t,u] = the sum of d_t * d_u over the group's points in the two-level order, d_t = (double)x[i,t] - mean[g,t],
 *     for u <= t only; cov[g,t,u] = cov[g,u,t] = M[g,t,u] / (double)(count[g] - 1).  The variance never comes from
 *     E[x^2] - mu^2.
 *   Dead groups.  A group with count < 2 is dead: its cov is all +0 (its mean is as stated above).
 *
 * svae_pca_eigen: G symmetric D x D matrices `cov` (only what svae_pca_moments writes is promised to be symmetric; the
 *   rotations below read both triangles), one workgroup of 256 per matrix, cyclic Jacobi in LDS.  A starts as the matrix, V as
 *   the identity.
 *   Norms.  rowsum(r) = the sum of a_rq^2 over q != r in q order onto +0; off2 = the sum of rowsum(r) in r order onto +0.  fro2
 *     is the same with q == r included, taken once from the input.
 *   Skipped.  Where fro2 is not finite -- any non-finite entry makes it so -- the matrix is skipped: eigenvalues and components
 *     all +0, sweeps -1, off_norm +0.
 *   Stopping.  Before each sweep off2 is formed; the workgroup stops when off2 <= 2^-104 * fro2 or when 30 sweeps are done.  The
 *     decision is the workgroup's own; nothing is read back.  sweeps = the sweeps done, off_norm = sqrt(off2) of the last test.
 *     A diagonal matrix -- the all-zero one of a dead group among them -- takes 0 sweeps and leaves V the identity.
 *   A sweep is the round-robin tournament of n = D + (D & 1) players in n - 1 steps.  At step s = 0 .. n - 2 seat 0 holds
 *     player 0 and seat k >= 1 holds player 1 + ((k - 1 + (n - 1) - s) mod (n - 1)); the pairs of the step are the seats
 *     (k, n - 1 - k), k = 0 .. n / 2 - 1.  A pair with player D in it (the bye of an odd D) is skipped.  Each pair is written
 *     (p, q) with p < q.
 *   A step.  First every pair's (c, s) from the step's incoming matrix: where a_pq == 0, c = 1 and s = 0; else
 *       theta = (a_qq - a_pp) / (2 * a_pq),  t = sign(theta) / (|theta| + sqrt(theta * theta + 1)) with sign(0) = +1,
 *       c = 1 / sqrt(t * t + 1),  s = t * c.
 *     Then all row updates A <- J^T A:  a_pj' = c * a_pj - s * a_qj,  a_qj' = s * a_pj + c * a_qj  for every j.
 *     Then all column updates A <- A J and V <- V J:  a_jp' = c * a_jp - s * a_jq,  a_jq' = s * a_jp + c * a_jq, and the same
 *       on v_jp, v_jq, for every j.  Then a_pq = a_qp = +0 exactly.  The pairs of a step are disjoint, so their updates within
 *       each of the three phases touch different entries: the order stated is exact and the step's rotations run in parallel.
 *   Result.  lambda_j = a_jj, its vector column j of V.  Sorted by descending lambda, equal values by ascending j.  Each vector
 *     is scaled by -1 where its entry of largest magnitude (of equal magnitudes the lowest index) is negative.
 *     eigenvalues[g, r] is the r-th largest, components[g, r, :] its vector: ROWS are components.
 *
 * svae_pca_project: proj[i, p] = the sum over t, in index order onto +0, of ((double)x[i,t] - mean[g,t]) * components[g,p,t],
 *   for p < P (1 <= P <= D), g the point's group.  A point in no group, or in a group with count[g] < 2, gets a row of +0.  One
 *   thread per (i, p); no reduction across threads.
 *
 * SVAE_E_INVALID: D, G, N or G D (D + 1) / 2 outside the limits; P outside 1..D; a null x, count, mean, cov, eigenvalues,
 *   components, sweeps, off_norm or proj; a null group with G != 1; count, mean, cov, eigenvalues, components, off_norm or proj
 *   not 8-byte aligned.  A refused call leaves every buffer untouched.  All launches are filed under the `augment` kind of
 *   svae_profile_read.
 */
#ifndef SVAE_PCA_H
#define SVAE_PCA_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t svae_pca_workspace_bytes(int64_t N, int32_t D, int32_t G);
int svae_pca_moments(const float* x, int64_t N, int32_t D, int32_t G, const int32_t* group, int64_t* count, double* mean,
                     double* cov, void* ws, size_t ws_bytes, svae_stream_t stream);
int svae_pca_eigen(const double* cov, int32_t D, int32_t G, double* eigenvalues, double* components, int32_t* sweeps,
                   double* off_norm, svae_stream_t stream);
int svae_pca_project(const float* x, int64_t N, int32_t D, int32_t G, int32_t P, const int32_t* group, const int64_t* count,
                     const double* mean, const double* components, double* proj, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_PCA_H */
