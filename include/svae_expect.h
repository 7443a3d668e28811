/*
 * svae_expect.h -- maximum-likelihood (expectation-maximisation) class averages: spread each image over the references and
 * poses of svae_classify.h's neighbourhood by its posterior probability under a Gaussian noise model, and add it, so weighted,
 * into every class it may belong to.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h, svae_align.h, svae_ctfcorr.h, svae_cluster.h, svae_frc.h, svae_refine.h, svae_classify.h and
 * svae_gmm.h stay, declaration for declaration, what their users and tests hold them to.  The reference has no counterpart.
 *
 * svae_pose_expect
 * Inputs.  y (B, rows*cols, C) floats, ref (n_ref, rows*cols, C) doubles, weight (rows*cols) doubles or NULL (= 1), cand (B, M)
 *   int32, pose_in (B, 3) floats, A, step, S and interp: exactly what they are in svae_classify.h, but M in 1..64.  log_prior
 *   (n_ref) doubles or NULL (= 0 everywhere); inv_sigma2 a double, finite and >= 0: the reciprocal of the noise variance.
 *   N = rows*cols, nA = 2A+1, nS = 2S+1, V = nA nS nS.
 * Live slots.  Slot j of image b is live when r = cand[b, j] lies in [0, n_ref), no earlier slot of the row holds the same r,
 *   and log_prior[r] is finite.  Every other slot is dead.
 * Log-weights.  For a live slot, an angle k = -A..A and a shift (sy, sx), D(j, k, sy, sx) = sum_{pix,c} wr[pix, c] Q[pix, c] with
 *   wr = weight * ref[r] (ref[r] itself where weight is NULL) and P_k, Q those of svae_refine.h; the sum in that header's order
 *   (per lane over its pixels upwards with stride 64, the channels upwards within a pixel, one wave's butterfly): the numerator
 *   of svae_pose_classify's score before its division.  A prologue launch, one workgroup of 256 per reference, takes
 *   h[r] = sum_{pix,c} (weight[pix] ref[r, pix, c]) ref[r, pix, c] with the loop and the block sum of svae_classify.h's norms (per
 *   thread over its elements upwards with stride 256, a butterfly over each wave, the four waves in index order).  Then
 *     L(j, k, sy, sx) = inv_sigma2 * (D - 0.5 * h[r]) + log_prior[r],
 *   evaluated as written.  This is the Gaussian log-likelihood -1/2 sum weight (Q - ref[r])^2 / sigma^2 of the image under the
 *   reference with per-pixel precision weight / sigma^2, plus the log prior, WITHOUT its term -1/2 sum weight Q^2 / sigma^2.
 *   That term is dropped as a constant across the candidates: it does not depend on the reference at all, it depends on the
 *   angle only through the resampling of the same image, and across the shifts it varies only by what a shift moves across the
 *   box border (the pixels of P_k that leave the box, and the zeros that enter).
 * Posterior.  The live volume is walked slot upwards, then k, then sy, then sx.  Lmax is its first maximum under strict `>`
 *   starting from -infinity.  Z = sum exp(L - Lmax) over the live volume: per thread over the flat index i = ((j nA + k + A) nS
 *   + sy + S) nS + sx + S upwards with stride 256 (dead slots contribute nothing), a butterfly over each wave, the four waves in
 *   index order.  p = exp(L - Lmax) / Z.  log_evidence[b] = Lmax + log(Z).  class_post[b, j] = sum_{k,sy,sx} p, one wave's
 *   work per slot: per lane over the slot's V entries upwards with stride 64, a butterfly; 0 for a dead slot.
 *   best[b] = (slot, k, sx, sy) of Lmax, int32.
 * Contributions.  contrib[b, j, pix, c] = sum_k sum_sy sum_sx p(j, k, sy, sx) Q_{k,sy,sx}[pix, c], doubles: each element is the work
 *   of one thread, which adds the terms k upwards, then sy, then sx, each as p * Q rounded and then added; a term whose source
 *   pixel lies outside the box, or whose p is exactly 0, is skipped (it would add 0).  cover_w[b, j, pix] is the same sum of
 *   p * cov, cov being 1 where svae_align.h's coverage flag of P_k holds at the shifted source pixel and 0 elsewhere and
 *   outside the box.  The rows of dead slots are written as zeros.
 * Skipped.  An image with no live slot, with a non-finite component in its pose, or with any L of a live slot that is not
 *   finite is skipped: class_post 0, log_evidence 0, best = (-1, 0, 0, 0), contrib and cover_w rows all zero.
 * Order of work.  Each angle is resampled TWICE: a first pass over the angles fills the L volume, the posterior is formed, and
 *   a second pass over the angles resamples P_k again (the same bits) and adds the contributions.  Only one plane is ever
 *   held.  Doubles with contraction off, no atomics, one workgroup of 256 per image, which sees nothing of the others: two
 *   runs give the same bits, and one call on B images equals two calls on its halves, bit for bit.
 * Memory.  `ws` is always needed (non-NULL, 256-byte aligned, at least svae_pose_expect_workspace_bytes long); its first
 *   roundup32(n_ref) doubles hold h (roundup32 = up to a multiple of 32).  The workgroup keeps the plane (N C doubles), its
 *   coverage (N doubles), the L volume (M V doubles), 8 doubles of reduction space and the M slot references (64 int32 = 32
 *   doubles) in LDS while 8 (N C + N + M V + 40) bytes fit the 160 KiB of one compute unit; the query then returns
 *   8 roundup32(n_ref).  Above that the plane, the coverage and the volume live in a per-workgroup slice of `ws` of
 *   roundup32(N C + N + M V) doubles after h (at most 512 slices, the grid striding over the images; the same arithmetic in the
 *   same order) and the query returns 8 (roundup32(n_ref) + min(B, 512) roundup32(N C + N + M V)).
 *
 * svae_expect_sums_update
 *   The soft counterpart of svae_align.h's svae_class_sums_update, on the same `sum` (n_classes, N, C) and `count`
 *   (n_classes, N) doubles: contrib (B, M, N, C) and cover_w (B, M, N) as svae_pose_expect wrote them for cand (B, M); target
 *   (n_ref) int32 maps a reference to its accumulator class, NULL = identity.  One thread per (class t, pixel) walks b upwards
 *   and within it the slots j upwards; where r = cand[b, j] lies in [0, n_ref) and target[r] == t it adds contrib[b, j, pix, c]
 *   into sum[t, pix, c] and cover_w[b, j, pix] into count[t, pix].  A target outside [0, n_classes) matches no thread and is
 *   skipped.  No atomics: the same sequence of updates gives the same bits.
 *
 * SVAE_E_INVALID, every buffer untouched.  svae_pose_expect: B < 1, n_ref < 1, rows or cols outside 2..1024, C outside
 *   1..SVAE_MAX_OUT, B*rows*cols*C or n_ref*rows*cols*C >= 2^31, A outside 0..32, S outside 0..8, M outside 1..64,
 *   B*M*rows*cols*C >= 2^31, A > 0 with a step that is not finite and > 0, an interp that is neither constant, an inv_sigma2 that
 *   is not finite or is negative, a null y, ref, cand, pose_in, contrib, cover_w, class_post, log_evidence or best, a workspace
 *   that is null, misaligned or too small.  svae_pose_expect_workspace_bytes returns 0 for sizes outside these ranges.
 *   svae_expect_sums_update: B < 1, N < 1, C outside 1..SVAE_MAX_OUT, n_classes outside 1..4096, n_ref < 1, B*N*C or
 *   n_classes*N*C >= 2^31 (svae_class_sums_update's), M outside 1..64, B*M*N*C >= 2^31, a null contrib, cover_w, cand, sum or
 *   count.
 *
 * All launches are filed under the `augment` kind of svae_profile_read.
 */
#ifndef SVAE_EXPECT_H
#define SVAE_EXPECT_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t svae_pose_expect_workspace_bytes(int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A,
                                        int32_t S);
int svae_pose_expect(const float* y, const double* ref, const double* weight, const double* log_prior, const int32_t* cand,
                     const float* pose_in, int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A,
                     double step, int32_t S, int32_t interp, double inv_sigma2, double* contrib, double* cover_w,
                     double* class_post, double* log_evidence, int32_t* best, void* ws, size_t ws_bytes, svae_stream_t stream);
int svae_expect_sums_update(const double* contrib, const double* cover_w, const int32_t* cand, const int32_t* target, int32_t B,
                            int32_t M, int32_t N, int32_t C, int32_t n_ref, int32_t n_classes, double* sum, double* count,
                            svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_EXPECT_H */
