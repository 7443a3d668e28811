/*
 * svae_stream.h -- streaming K-sample scorer: per-image bound, pose and latents with K unbounded.
 *
 * An addition to the C ABI of svae.h (same library, same conventions, SVAE_ABI_VERSION unchanged); it is a header of its
 * own so that svae.h stays, declaration for declaration, what its users and tests already hold it to.  The reference has no
 * counterpart: it ends at the minibatch means of eval_minibatch (train_mnist.py:86-90) and never reports anything per image.
 *
 * svae_iw_head_forward reduces one call's K <= SVAE_IW_MAX_SAMPLES samples per image to three batch scalars, and the decoder
 * in front of it holds all B*K rows of activations at once.  Here the samples arrive in chunks: after each chunk's decoder
 * and log-likelihood calls, svae_iw_stream_update merges its loglik, log_ratio and sampled coordinates into a small
 * per-image record, so the total K is any positive number and memory is that of one chunk.
 *
 * With a = loglik + log_ratio over the n samples of image b seen so far, M their max and w_k = exp(a_k - M):
 *   s = sum w, s2 = sum w^2, L_b = M + log s - log n (the bound of svae_iw_head_forward at K = n),
 *   effective sample size s^2 / s2 in [1, n],
 *   the importance-weighted posterior mean of every latent coordinate, sum w v / s -- for the rotation the circular mean
 *   atan2(S, C) of S = sum w sin(theta), C = sum w cos(theta), with resultant length R = sqrt(C^2 + S^2) / s --,
 *   and the best sample: the largest a and that sample's coordinates (replaced on a strictly larger a only: ties keep the
 *   earliest chunk and the lowest index).
 * A chunk whose max exceeds M rescales the running sums by exp(M_old - M_new) (s2 by its square); doubles throughout, each
 * output rounded once; fixed summation order, no atomics: the same chunking gives the same bits.
 *
 * `state` is an opaque record in DEVICE memory, svae_iw_stream_state_bytes(B, inf_dim) bytes, 8-byte aligned, owned by the
 * caller.  svae_iw_stream_reset empties it and must come first; the library remembers, per state address, the B and inf_dim
 * it was reset for and whether a chunk has been merged since (host side, a few words per address, replaced by the next reset
 * of that address), which is what lets the calls below refuse a mismatch without reading the device.  Calls on one state
 * take effect in the order they are enqueued on one stream.
 *
 * svae_iw_stream_update: one chunk of K samples per image, 1 <= K <= SVAE_IW_MAX_SAMPLES, B*K < 2^31; row b*K + k is sample
 *   k of image b.  loglik, log_ratio (B*K); theta (B*K) iff rotate, dx (B*K, 2) iff translate, zc (B*K, inf_dim - rotate -
 *   2*translate) iff non-empty: the outputs of svae_latent_iw_forward for that chunk and descriptor, NULL when absent.
 * svae_iw_stream_finish: per_image (B, SVAE_IW_STREAM_COLS(inf_dim)) and, unless NULL, out3 = {mean_b L_b, mean over all
 *   samples of loglik, mean over all samples of -log_ratio}.  The state is not consumed: update and finish may alternate.
 *   Columns of per_image:
 *     0 L_b   1 mean loglik   2 mean(-log_ratio)   3 effective sample size   4 best a   5 R (1 when rotate = 0)
 *     6 .. 6+inf_dim           importance-weighted mean per latent coordinate, in latent order (rotation, dx0, dx1, content),
 *                              in the units the decoder received: radians, dx already times dx_scale, content times z_scale
 *     6+inf_dim .. 6+2*inf_dim the best sample's coordinates, same order and units
 * Edges as in svae_iw_head_forward: a = -inf weighs 0; an image whose a are all -inf so far has L_b = -inf, effective
 * sample size 0, R 0 when rotate, weighted means 0 and keeps its first sample as best; a NaN stays in its image's row.
 * SVAE_E_INVALID: K out of range, B*K >= 2^31, a null required pointer, a state that was not reset, a B or inf_dim that
 * disagrees with the state's, finish before any update.
 */
#ifndef SVAE_STREAM_H
#define SVAE_STREAM_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_IW_STREAM_COLS(inf_dim) (6 + 2 * (inf_dim)) /* floats per image in per_image */

size_t svae_iw_stream_state_bytes(int32_t B, int32_t inf_dim); /* 0 = invalid B or inf_dim */
int svae_iw_stream_reset(void* state, int32_t B, int32_t inf_dim, svae_stream_t stream);
int svae_iw_stream_update(void* state, const svae_latent_desc* d, int32_t K, const float* loglik, const float* log_ratio,
                          const float* theta, const float* dx, const float* zc, svae_stream_t stream);
int svae_iw_stream_finish(const void* state, const svae_latent_desc* d, float* per_image, float* out3,
                          svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_STREAM_H */
