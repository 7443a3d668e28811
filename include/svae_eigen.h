/*
 * svae_eigen.h -- per-class eigenimages of aligned images, on the device: the variance map and the leading eigenpairs of the
 * covariance of the members of every class about their class average, by block subspace iteration with a Rayleigh-Ritz step.
 * The D x D covariance (D = N C values per image) is never formed.  Every sum has a fixed order, so the same buffers give the
 * same bits on any run, any device and any stream.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae_align.h and svae_pca.h stay, declaration for declaration, what their users and tests hold them to.  The reference
 * has no counterpart: it ends at .sav files and PNG dumps of one minibatch.
 *
 * Data.  aligned (B, N, C) floats and cover (B, N) bytes or NULL (= covered everywhere) as svae_align_images writes them;
 *   label (B) int32; K classes; mean (K, N, C) DOUBLES, the class averages (sum / count of svae_class_sums_update where
 *   count > 0, else 0).  D = N C, and e = j C + c is the index of channel c of pixel j.  R is the width of the basis.
 *   Q, Y (K, D, R), ssq (K, D), T (B, R), G (K, R, R), W (K, R, R), lambda (K, R), eigenimages (K, P, D), residual (K, P),
 *   rot (K, P, R) and coords (B, P) are DOUBLES, row-major; members (K) int64 is the number of images of each class.
 *   The residual of image b in class k = label[b]:  d_b[e] = cover[b, j] ? (double)aligned[b, e] - mean[k, e] : +0  (the float
 *   is widened exactly).  An image whose label is outside [0, K) (use -1) is in no class.
 *   All arithmetic is double with contraction off: one IEEE operation per operator written below, sqrt the correctly rounded
 *   one.  No atomics anywhere, and no matrix instruction: its internal order of summation is not ours to state.
 *   Limits.  1 <= R <= 64, 1 <= P <= R, 1 <= K <= 4096, 1 <= C <= SVAE_MAX_OUT, 1 <= B, 1 <= N, B N C < 2^31, K D R <= 2^28.
 *   Non-finite pixels.  Nothing filters them: a non-finite covered pixel of an image makes that image's row of T, and from
 *     there its class's Y at every index the image covers and its own entry of ssq, non-finite.  It reaches its own class and
 *     no other.
 *
 * The orders of summation.
 *   Segments (svae_eig_project, svae_eig_gram).  R' is the least power of two >= R and S = 256 / R' (4 .. 256) the number of
 *     segments; L = ceil(D / S); segment s holds the indices [s L, min(D, (s + 1) L)), possibly none.  A sum over e is formed per
 *     segment in index order onto +0, then the S segment sums are added in segment order onto +0.
 *   Lanes (svae_eig_orthonormalise, svae_eig_rotate).  Lane t = 0 .. 255 holds the indices e = t, t + 256, t + 512, ... below D.
 *     A sum over e is formed per lane in index order onto +0, then the 256 lane sums are added in lane order onto +0.
 *   Both are functions of D and R alone.
 *
 * svae_eig_project: T[b, r] = the sum over e, in the segment order, of d_b[e] * Q[k, e, r], k = label[b].  An uncovered index
 *   is skipped, not added as 0.  An image in no class gets a row of +0.  One workgroup per image.
 *
 * svae_eig_accumulate: for every class k, index e and column r, Y[k, e, r] takes, onto the value it holds, d_b[e] * T[b, r] for
 *   the images b of this call with label[b] == k and e covered, IN INDEX ORDER of b; where ssq is not NULL, ssq[k, e] takes
 *   d_b[e] * d_b[e] the same way.  The caller zeroes Y (and ssq) before the first call of a walk.  One thread per (k, e, r)
 *   walks the B labels, so one call equals two calls on the two halves of the minibatch, bit for bit.  After a walk over all the
 *   images with T from svae_eig_project, Y_k = (n_k - 1) S_k Q_k, S_k the class's covariance.
 *
 * svae_eig_orthonormalise: per class, Q = the columns of Y made orthonormal by modified Gram-Schmidt applied twice, one
 *   workgroup per class, every sum in the lane order.  For column j = 0 .. R - 1, with q = Y[k, :, j]:
 *     before = sqrt(sum of q[e]^2);
 *     twice over:  for i = 0 .. j - 1 in order, dead columns skipped:  c = sum of Q[k, e, i] * q[e];  q[e] = q[e] - c * Q[k, e, i];
 *     after = sqrt(sum of q[e]^2).
 *   Column j is DEAD where after is 0 or not finite or after < 2^-26 * before (SVAE_EIG_DEAD_LOG2): Q[k, :, j] is then all +0.
 *   Else Q[k, e, j] = q[e] / after.  A class whose members span fewer than R directions, and a box with D < R, end with dead
 *   columns; so does a direction whose weight in Y has fallen below 2^-26 of the column's.  The start array of the iteration goes
 *   through the same call.  Y is not written.
 *
 * svae_eig_gram: G[k, r, s] = ((A[r, s] + A[s, r]) * 0.5) / (double)(members[k] - 1) with A[r, s] = the sum over e, in the segment
 *   order, of Q[k, e, r] * Y[k, e, s]; exactly symmetric.  A class with members[k] < 2 is dead: its G is all +0.  One workgroup
 *   per (class, row).  G is what svae_pca_eigen takes as `cov` with its D = R.
 *
 * svae_eig_rotate: W (K, R, R) and lambda (K, R) as svae_pca_eigen writes components and eigenvalues from G: row p of W[k] is
 *   the p-th vector.  For p < P, one workgroup per (class, p):
 *     v[e] = the sum over r, in index order onto +0, of Q[k, e, r] * W[k, p, r];
 *     u[e] = (the sum over r, in index order onto +0, of Y[k, e, r] * W[k, p, r]) / (double)(members[k] - 1);
 *     sg = -1 where the entry of v of largest magnitude (of equal magnitudes the lowest e) is negative, else +1;
 *     eigenimages[k, p, e] = sg * v[e];  rot[k, p, r] = sg * W[k, p, r];
 *     residual[k, p] = sqrt(the sum over e, in the lane order, of w * w),  w = sg * u[e] - lambda[k, p] * (sg * v[e]).
 *   A dead class gets +0 in all three.  A dead column of Q has an all-zero row and column in G, which svae_pca_eigen returns as
 *   an eigenvalue of zero with a unit vector: its eigenimage is all +0.
 *
 * svae_eig_coords: coords[b, p] = the sum over r, in index order onto +0, of T[b, r] * rot[k, p, r], k = label[b], T that of
 *   the last walk; an image in no class gets a row of +0.  One thread per (b, p).
 *
 * SVAE_E_INVALID: a size outside the limits above; a null pointer (cover and ssq aside); a double or int64 buffer that is not
 *   8-byte aligned; an output that overlaps an input of the same call.  A refused call leaves every buffer untouched.  All
 *   launches are filed under the `augment` kind of svae_profile_read.  No call needs a workspace.
 */
#ifndef SVAE_EIGEN_H
#define SVAE_EIGEN_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_EIG_MAX_R 64
#define SVAE_EIG_DEAD_LOG2 (-26)

int svae_eig_project(const float* aligned, const uint8_t* cover, const int32_t* label, const double* mean, const double* Q,
                     int32_t B, int32_t N, int32_t C, int32_t K, int32_t R, double* T, svae_stream_t stream);
int svae_eig_accumulate(const float* aligned, const uint8_t* cover, const int32_t* label, const double* mean, const double* T,
                        int32_t B, int32_t N, int32_t C, int32_t K, int32_t R, double* Y, double* ssq, svae_stream_t stream);
int svae_eig_orthonormalise(const double* Y, int32_t K, int64_t D, int32_t R, double* Q, svae_stream_t stream);
int svae_eig_gram(const double* Q, const double* Y, const int64_t* members, int32_t K, int64_t D, int32_t R, double* G,
                  svae_stream_t stream);
int svae_eig_rotate(const double* Q, const double* Y, const double* W, const double* lambda, const int64_t* members, int32_t K,
                    int64_t D, int32_t R, int32_t P, double* eigenimages, double* residual, double* rot, svae_stream_t stream);
int svae_eig_coords(const double* T, const int32_t* label, const double* rot, int32_t B, int32_t K, int32_t R, int32_t P,
                    double* coords, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_EIGEN_H */
