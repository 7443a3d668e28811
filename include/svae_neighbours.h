/*
 * svae_neighbours.h -- latent-space neighbour averages, on the device: an exact K-nearest-neighbour search over the content
 * latents of a whole split, and the gather-average of every image's neighbours' aligned images.  One denoised image per image
 * and no partition into classes.  Every sum has a fixed order, so the same buffers give the same bits on any run, any device
 * and any stream.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that the other headers stay, declaration for declaration, what their users and tests hold them to.  The reference has no
 * counterpart.
 *
 *   All arithmetic is double with contraction off: one IEEE operation per operator written below.  No atomics anywhere, and
 *   no matrix instruction: its internal order of summation is not ours to state.
 *
 * svae_nbr_search: one update of the running neighbour lists of B query images from M candidate images.
 *   Data.  query (B, D) and cand (M, D) DOUBLES, row-major: row b of query is image query_base + b, row c of cand is image
 *     cand_base + c.  best_d2 (B, K) DOUBLES and best_index (B, K) int64 are the running lists, read AND written.
 *   Distance.  d2[b, c] = the sum over j = 0 .. D - 1, in index order onto +0, of t * t with t = query[b, j] - cand[c, j].
 *   Order.  The total order is (d2, index), ascending: of equal d2 the lower image index comes first.
 *   Lists.  An empty slot is (+inf, -1); a slot is read as empty where its index is negative.  The caller fills the lists with
 *     empty slots before the first call.  A list is always its non-empty entries in the order above, followed by empty slots.
 *   Admissible.  Candidate c is admissible for row b where cand_base + c != query_base + b (an image is never its own
 *     neighbour) and d2[b, c] is finite.  A NaN or an inf never enters: an image with a non-finite latent lists nothing and is
 *     listed by nobody.
 *   After the call row b holds the K smallest, under the order, of the union of its old non-empty entries and the admissible
 *     candidates of the call, and nothing else.  So the result is a property of the SET offered: any split of the candidates
 *     into calls, in any order, gives the same bits, and so does any split of the queries.  Entries are not de-duplicated:
 *     offering an image twice is the caller's error, and it then appears twice.
 *   Limits.  1 <= D <= 512, 1 <= K <= 256 (SVAE_NBR_MAX_K), 1 <= B, 1 <= M, query_base >= 0, cand_base >= 0.
 *   SVAE_E_INVALID: a size outside the limits; a null pointer; a buffer that is not 8-byte aligned; an output that overlaps
 *     an input or the other output.
 *
 * svae_nbr_average: the weighted average of the listed images, pixel by pixel over the pixels they cover.
 *   Data.  stack (images, N, C) floats and cover (images, N) bytes or NULL (= covered everywhere) as svae_align_images writes
 *     them; index (B, T) int64; weight (B, T) DOUBLES or NULL (= all 1); average (B, N, C) floats; support (B, N) DOUBLES or
 *     NULL.
 *   For image b, pixel j and channel c walk the slots t = 0 .. T - 1 in index order, num and den starting from +0:
 *     a slot whose index i = index[b, t] is outside [0, images) is skipped (use -1 for an empty slot);
 *     a slot with cover[i, j] == 0 is skipped;
 *     otherwise  num = num + weight[b, t] * (double)stack[i, j, c]  and  den = den + weight[b, t]  (the float widened exactly).
 *   average[b, j, c] = den > 0 ? (float)(num / den) : +0 (one division, rounded once to float);  support[b, j] = den.
 *   Nothing filters non-finite pixels or weights: they reach the rows that list them and no others.
 *   Limits.  1 <= T <= 257 (SVAE_NBR_MAX_K + 1: the image itself and its list), 1 <= C <= SVAE_MAX_OUT, 1 <= N, N C < 2^31,
 *     1 <= images < 2^31, 1 <= B.  All indexing is in 64 bits.
 *   SVAE_E_INVALID: a size outside the limits; a null stack, index or average; a double or int64 buffer that is not 8-byte
 *     aligned; an output that overlaps an input or the other output.
 *
 * A refused call leaves every buffer untouched.  All launches are filed under the `augment` kind of svae_profile_read.  No call
 * needs a workspace.
 */
#ifndef SVAE_NEIGHBOURS_H
#define SVAE_NEIGHBOURS_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_NBR_MAX_K 256

int svae_nbr_search(const double* query, int32_t B, int64_t query_base, const double* cand, int32_t M, int64_t cand_base,
                    int32_t D, int32_t K, double* best_d2, int64_t* best_index, svae_stream_t stream);
int svae_nbr_average(const float* stack, const uint8_t* cover, int64_t images, int32_t N, int32_t C, const int64_t* index,
                     const double* weight, int32_t B, int32_t T, float* average, double* support, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_NEIGHBOURS_H */
