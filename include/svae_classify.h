/*
 * svae_classify.h -- multi-reference alignment: score each image against several references (class averages) over the pose
 * neighbourhood of svae_refine.h and name the reference it fits best.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h, svae_align.h, svae_ctfcorr.h, svae_cluster.h, svae_frc.h and svae_refine.h stay, declaration for
 * declaration, what their users and tests hold them to.  The reference has no counterpart.
 *
 * Inputs.  y (B, rows*cols, C) floats, ref (n_ref, rows*cols, C) doubles, weight (rows*cols) doubles or NULL, pose_in (B, 3)
 *   floats, A, step, S and interp: exactly what they are in svae_refine.h.  cand (B, M) int32: the references image b is scored
 *   against, slot by slot; an entry outside [0, n_ref) is an empty slot.  M in 1..4096.  N = rows*cols.
 * Candidate scores.  For image b and slot j, take the score volume of svae_refine.h against the reference r = cand[b, j]: the
 *   same candidates P_k (k = -A..A), the same shifts, the same wr = weight * ref[r], the same normalisation by
 *   sqrt(sum wr^2) * sqrt(sum P_k^2) and the same exact 0 where sum P_k^2 == 0.  cand_score[b, j] is the maximum of that volume,
 *   taken with strict `>` starting from -infinity (a NaN never enters it).  Every sum keeps svae_refine.h's fixed order (the
 *   norms: per thread over its elements upwards with stride 256, a butterfly over each wave, the four waves in index order;
 *   the correlations: per lane with stride 64 and one wave's butterfly; doubles, contraction off), so cand_score[b, j] equals
 *   BIT FOR BIT the `score` svae_pose_search returns for image b with ref_index = cand[b, j] wherever that search is not
 *   skipped.  Where it would skip -- an empty slot, a pose with a non-finite component, a reference with sum wr^2 == 0, every
 *   score NaN -- cand_score[b, j] is -infinity, and the slot is not live.
 * Winner.  choice[b] is the first slot j, walked upwards, whose cand_score is the maximum, compared with strict `>` starting
 *   from -infinity: -1 if no slot is live, and a reference repeated in a later slot never wins.  ref_chosen[b] =
 *   cand[b, choice[b]], or -1.  margin[b] = the winner's cand_score minus the largest cand_score among the other live slots;
 *   +infinity where fewer than two slots are live (no winner included).  margin may be NULL and is then not written.
 * Pose.  This entry point does not refine the pose: the refined pose of the winner is, by definition, what svae_pose_search
 *   gives with ref_index = ref_chosen, and the caller makes that second call (1/M of this one's work).
 * Determinism.  No atomics: two runs give the same bits, and since every image is the work of one workgroup that sees nothing
 *   of the others, one call on B images equals two calls on its halves, bit for bit.
 * Memory.  `ws` is always needed (non-NULL, 256-byte aligned, at least svae_pose_classify_workspace_bytes long).  A prologue
 *   launch, one workgroup of 256 per reference, puts each reference's sum wr^2 into the first roundup32(n_ref) doubles of
 *   `ws` (roundup32 = up to a multiple of 32): once per call, not once per image.  The main launch runs one workgroup of 256
 *   per image and keeps the plane P_k (N C doubles), the M running maxima and 8 doubles of reduction space in LDS while
 *   8 (N C + M + 8) bytes fit the 160 KiB of one compute unit; the query then returns 8 roundup32(n_ref).  Above that the plane
 *   and the maxima live in a per-workgroup slice of `ws` of roundup32(N C + M) doubles after the norms (at most 512 slices, the
 *   grid striding over the images; the same arithmetic in the same order) and the query returns
 *   8 (roundup32(n_ref) + min(B, 512) roundup32(N C + M)).
 *
 * SVAE_E_INVALID, every buffer untouched: B < 1, n_ref < 1, rows or cols outside 2..1024, C outside 1..SVAE_MAX_OUT,
 *   B*rows*cols*C or n_ref*rows*cols*C >= 2^31, A outside 0..32, S outside 0..8, M outside 1..4096, B*M >= 2^31, A > 0 with a
 *   step that is not finite and > 0, an interp that is neither constant, a null y, ref, cand, pose_in, choice, ref_chosen or
 *   cand_score, a workspace that is null, misaligned or too small.  svae_pose_classify_workspace_bytes returns 0 for sizes
 *   outside these ranges.
 *
 * Both launches are filed under the `augment` kind of svae_profile_read.
 */
#ifndef SVAE_CLASSIFY_H
#define SVAE_CLASSIFY_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t svae_pose_classify_workspace_bytes(int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C);
int svae_pose_classify(const float* y, const double* ref, const double* weight, const int32_t* cand, const float* pose_in,
                       int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A, double step,
                       int32_t S, int32_t interp, int32_t* choice, int32_t* ref_chosen, double* cand_score, double* margin,
                       void* ws, size_t ws_bytes, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_CLASSIFY_H */
