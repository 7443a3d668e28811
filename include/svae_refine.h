/*
 * svae_refine.h -- reference-based pose refinement: search a small neighbourhood of rotations and integer-pixel shifts around
 * each image's current pose for the one whose canonical-frame image correlates best with a reference (a class average).
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h, svae_align.h, svae_ctfcorr.h, svae_cluster.h and svae_frc.h stay, declaration for declaration,
 * what their users and tests hold them to.  The reference has no counterpart.
 *
 * Inputs.  y (B, rows*cols, C) floats, the observed images; ref (n_ref, rows*cols, C) doubles; weight (rows*cols) doubles or
 *   NULL (= 1 everywhere); ref_index (B) int32, the reference of each image; pose_in (B, 3) floats = theta, dx0, dx1 in the
 *   decoder's units, exactly what svae_align_images takes as theta[b], dx[b, 0], dx[b, 1].  A = angles on each side (0..32),
 *   step = their spacing in radians (finite and > 0; ignored and taken as 0 where A == 0), S = shift radius in pixels (0..8),
 *   interp one of the SVAE_ALIGN_* constants of svae_align.h.  N = rows*cols, nA = 2A+1, nS = 2S+1.
 * Candidates.  For k = -A..A: theta_k = (double)theta + (double)k * step, and P_k (N, C) is the image brought into the canonical
 *   frame at (theta_k, dx0, dx1) by the arithmetic of svae_align.h's alignment (one device function serves both): its geometry,
 *   coverage, clamping, interpolation and the 0 of an uncovered pixel -- but kept in double, NOT rounded to float.  An integer
 *   shift (sx, sy), |sx|, |sy| <= S, stands for the pose (theta_k, dx0 + sx/a, dx1 + sy/bq), a = (cols-1)/2, bq = (rows-1)/2,
 *   and its image is Q[jy, jx] = P_k[jy + sy, jx - sx] where that lies inside the box, 0 elsewhere.  On the pixel lattice this
 *   IS that pose's alignment, without a second resampling: in svae_align.h U = X - a*dx0 and V = Y - bq*dx1, so adding sx/a to
 *   dx0 turns U(X) into U(X - sx), i.e. column jx reads what column jx - sx read, and adding sy/bq to dx1 turns V(Y) into
 *   V(Y - sy), i.e. (Y = bq - jy) row jy reads what row jy + sy read; only what the shift moves across the border differs.
 * Score.  wr[j, c] = weight[j] * ref[r, j, c] (ref[r, j, c] itself where weight is NULL), r = ref_index[b];
 *   score(k, sy, sx) = sum_{j,c} wr[j, c] * Q[j, c] / ( sqrt(sum_{j,c} wr[j, c]^2) * sqrt(sum_{j,c} P_k[j, c]^2) ),
 *   and exactly 0 where either sum of squares is 0.  (The image norm is that of P_k, whatever the shift.)  Doubles with
 *   contraction off.  Each sum is taken in a fixed order -- per lane over its elements upwards, a butterfly over the 64 lanes
 *   of a wave, the waves in index order -- which is not index order: a float64 restatement agrees to rounding, not bit for bit.
 *   No atomics: two runs give the same bits, and since every image is the work of one workgroup that sees nothing of the
 *   others, one call on B images equals two calls on its halves, bit for bit.
 * Winner.  The volume is walked k upwards, then sy, then sx; the winner is the first maximum, compared with strict `>`
 *   starting from -infinity, so a NaN never wins.
 * Sub-step.  On each of the three axes (k, sx, sy), where the winner is interior to the axis: with l, c, r the scores at the
 *   lower neighbour, the winner and the upper neighbour along that axis, d = l - 2c + r, the offset is
 *   f = clamp(0.5 (l - r) / d, -0.5, 0.5) where d < 0 and 0 otherwise.  Where the winner sits at an end of the axis f = 0, and
 *   if that axis has more than one entry a flag bit is set: bit 0 for the angle, bit 1 for either shift axis.
 *   pose_out = (theta + (k + fk) * step, dx0 + (sx + fx) / a, dx1 + (sy + fy) / bq), evaluated in double as written from the
 *   pose widened to double, and rounded to float once.  With A = S = 0 that is pose_in exactly.
 * Outputs.  pose_out (B, 3) floats; score (B) doubles, the winner's grid score; offset (B, 4) int32 = k, sx, sy, flags; scores
 *   (B, nA, nS, nS) doubles, indexed [k + A, sy + S, sx + S], or NULL.
 * Skipped.  An image whose ref_index is outside [0, n_ref), whose pose has a non-finite component, whose reference has
 *   sum wr^2 == 0, or none of whose scores compares greater than -infinity (all NaN) is skipped: pose_out = pose_in bit for
 *   bit, score 0, offset 0, 0, 0 and flags = 4 (bit 2).  Its volume is all 0 in the first three cases and what was computed in
 *   the last.
 * Memory.  One workgroup of 256 per image keeps P_k and the image's score volume as doubles in LDS while
 *   8 (N C + nA nS nS + 8) bytes fit the 160 KiB of one compute unit; svae_pose_search_workspace_bytes then returns 0 and `ws`
 *   may be NULL.  Above that both live in a per-workgroup slice of `ws` (256-byte aligned, at least
 *   svae_pose_search_workspace_bytes long; at most 512 slices, the grid striding over the images): the same arithmetic in the
 *   same order.
 *
 * SVAE_E_INVALID, every buffer untouched: B < 1, n_ref < 1, rows or cols outside 2..1024, C outside 1..SVAE_MAX_OUT,
 *   B*rows*cols*C or n_ref*rows*cols*C >= 2^31, A outside 0..32, S outside 0..8, A > 0 with a step that is not finite and > 0,
 *   an interp that is neither constant, a null y, ref, ref_index, pose_in, pose_out, score or offset, a workspace that is null,
 *   misaligned or too small where one is needed.  svae_pose_search_workspace_bytes returns 0 for sizes outside these ranges.
 *
 * The launch is filed under the `augment` kind of svae_profile_read.
 */
#ifndef SVAE_REFINE_H
#define SVAE_REFINE_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t svae_pose_search_workspace_bytes(int32_t B, int32_t rows, int32_t cols, int32_t C, int32_t A, int32_t S);
int svae_pose_search(const float* y, const double* ref, const double* weight, const int32_t* ref_index, const float* pose_in,
                     int32_t B, int32_t n_ref, int32_t rows, int32_t cols, int32_t C, int32_t A, double step, int32_t S,
                     int32_t interp, float* pose_out, double* score, int32_t* offset, double* scores, void* ws, size_t ws_bytes,
                     svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_REFINE_H */
