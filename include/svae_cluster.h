/*
 * svae_cluster.h -- k-means over the content latents of a trained model, on the device: k-means++ seeding from host-drawn
 * uniforms and Lloyd iterations whose every sum has a fixed order, so that the same buffers give the same bits on any run.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h, svae_align.h and svae_ctfcorr.h stay, declaration for declaration, what their users and tests
 * hold them to.  The reference has no counterpart: it never groups the latents it infers.
 *
 * Shared arithmetic.  Points x are (N, D) floats, centres (k, D) DOUBLES, both row-major.
 *   Distance.  d2(i, j) = sum_t ((double)x[i,t] - c[j,t])^2, t in index order starting from +0, in double with contraction off
 *     (one rounding for the difference, one for its square, one for the addition).
 *   Unassigned points.  A point with any non-finite coordinate is unassigned: its label is -1 and it enters no sum and no count.
 *   Ties.  label[i] starts at centre 0 and moves to centre j (walked upwards) only where d2(i, j) < the best so far, strictly:
 *     equal distances keep the lowest index.
 *   Reductions over points have a two-level order that depends on N only.  The chunk length P is 256, doubled until
 *     ceil(N / P) <= 1024 (the rule of svae_grad_guard_norm); chunk c holds the points [c P, min(N, (c+1) P)).  Inside a chunk
 *     the values are added in point-index order onto +0, then the chunk totals are added in chunk-index order onto +0.  A point
 *     that does not take part contributes nothing (it is skipped, not added as 0).  No atomics anywhere.
 *   Limits.  1 <= D <= 64, 1 <= k <= 1024, k <= N < 2^31.  The centres are staged in LDS 4096 doubles at a time (whole
 *     centres: floor(4096 / D) of them); with more than that they are walked slab after slab, still upwards, which leaves the
 *     tie rule as stated.
 *
 * Workspace.  svae_kmeans_workspace_bytes(N, D, k) = 8 (N + 3 C + C k + C k D) bytes with C = ceil(N / P): the running minimum
 *   distances of the seeding (N doubles), and per chunk the inertia, the changed and assigned counts, the member counts per
 *   centre and the coordinate sums per centre.  0 for a geometry outside the limits.  `ws` is 256-byte aligned; one that is
 *   null, misaligned or too small is SVAE_E_WORKSPACE.  Its contents mean nothing between calls.
 *
 * svae_kmeans_seed: k-means++ from k uniforms u[j] in [0, 1) (device doubles the host drew and uploaded once).
 *   fallback(j) = min(floor(u[j] N), N - 1).  seed_index[0] = fallback(0).  For j >= 1, m_i = min over the seeds chosen so far
 *   of d2(i, seed) -- the distance to the seed point's coordinates widened to double -- and 0 for an unassigned point;
 *   T = sum_i m_i in the two-level order (every point takes part); prefix(i) = (the total of the chunks before i's, in chunk
 *   order) + (the running sum inside i's chunk through i).  seed_index[j] is the smallest i with prefix(i) > u[j] T, hence one
 *   with m_i > 0; where T == 0 (or T is not finite, or no such i exists) it is fallback(j).  centres[j,:] = (double)
 *   x[seed_index[j],:] exactly.  2 k - 1 small launches, nothing read back.
 *
 * svae_kmeans_step: one Lloyd iteration.
 *   Assign.  label[i] = argmin_j d2(i, j) against the INCOMING centres (ties and unassigned points as above); members[j] = the
 *     number of points labelled j; rec->inertia = the sum of the winning d2 over the assigned points in the two-level order;
 *     rec->changed = the number of i whose label differs from the incoming label[i] -- while rec->iterations == 0 the incoming
 *     labels are ignored and it is the number of assigned points --; rec->assigned = the number of points with finite
 *     coordinates; rec->empty = the number of centres without a member.
 *   update != 0.  Then centres[j,t] = S[j,t] / (double)members[j] (one double division), S[j,t] the sum of (double)x[i,t] over
 *     the points labelled j in the two-level order; a centre without a member keeps its coordinates.  rec->iterations += 1,
 *     and rec->converged_at = that count the first time changed == 0.
 *   update == 0.  centres, rec->iterations and rec->converged_at are left alone: the final labelling call, after which the
 *     labels are the argmin against the centres returned.
 *   Once changed == 0 the same labels give the same sums and so the same centres bit for bit: the caller simply enqueues a
 *   fixed number of steps.  The count lives on the device, so a replayed captured step advances it.
 *
 * svae_kmeans_record: ALL ZERO BYTES = a fresh record (like svae_guard_control); 8-byte aligned device memory.
 *
 * SVAE_E_INVALID: D outside 1..64, k outside 1..1024, N < k, N >= 2^31, a null x, centres, label, members or rec (step), a null
 *   x, u, centres or seed_index (seed), centres, members, rec or u not 8-byte aligned.  A refused call leaves every buffer
 *   untouched.  All launches are filed under the `augment` kind of svae_profile_read.
 */
#ifndef SVAE_CLUSTER_H
#define SVAE_CLUSTER_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct svae_kmeans_record {
    int64_t iterations;   /* update steps applied so far */
    int64_t changed;      /* labels the last step changed */
    int64_t converged_at; /* the iteration count at which changed first was 0; 0 = not yet */
    int64_t assigned;     /* points with finite coordinates */
    int64_t empty;        /* centres without a member at the last step */
    double inertia;       /* sum of the winning squared distances at the last step */
} svae_kmeans_record;

size_t svae_kmeans_workspace_bytes(int64_t N, int32_t D, int32_t k);
int svae_kmeans_seed(const float* x, int64_t N, int32_t D, int32_t k, const double* u, double* centres, int32_t* seed_index,
                     void* ws, size_t ws_bytes, svae_stream_t stream);
int svae_kmeans_step(const float* x, int64_t N, int32_t D, int32_t k, int32_t update, double* centres, int32_t* label,
                     int64_t* members, svae_kmeans_record* rec, void* ws, size_t ws_bytes, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_CLUSTER_H */
