/*
 * svae_frc.h -- Fourier ring correlation of pairs of real planes (the half-set averages of a class) and the filter of a plane
 * by per-ring weights: how good a class average is, and the average low-passed by that figure.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h, svae_align.h, svae_ctfcorr.h and svae_cluster.h stay, declaration for declaration, what their
 * users and tests hold them to.  The reference has no counterpart.
 *
 * Rings.  Frequency (u, v) of an n x m plane has the signed indices ku, kv in numpy's fftfreq order (a <= (len-1)/2 ? a :
 *   a - len, as in svae_ctfcorr.h).  With L = min(n, m) and R = L/2 + 1 (integer division) its ring is the largest integer
 *   r >= 1 with (2r-1)^2 (n m)^2 <= 4 ((ku L m)^2 + (kv L n)^2), evaluated in 64-bit integers, and 0 where no r >= 1
 *   qualifies (the DC term; on a box more than twice as long as it is wide also its nearest neighbours).  This is
 *   floor(L sqrt((ku/n)^2 + (kv/m)^2) + 1/2) without a rounding question.  Frequencies with r >= R (the corners beyond
 *   Nyquist) belong to no ring.  2 <= n, m <= 1024, so every product stays below 2^63.  Ring r stands for r / L cycles per
 *   pixel.
 * Mask.  Optional, in real space, applied to both planes before the transform: with d the distance in pixels of pixel
 *   (row a, column b) from the centre ((n-1)/2, (m-1)/2) (the centre svae_align_images uses), w = 1 for d <= radius,
 *   w = 0.5 (1 + cospi((d - radius)/edge)) for radius < d < radius + edge, w = 0 beyond.  mask_radius == 0 means no mask and
 *   mask_edge is then ignored; otherwise both are positive and finite.  Doubles, contraction off.
 * DFT.  Unnormalised forward transform, separable, rows then columns, doubles with contraction off, twiddles from a sincospi
 *   table indexed by k*v mod len, every sum in index order (svae_ctfcorr.h's construction): two runs give the same bits.
 *   svae_frc transforms z = w (a + i b) once as a complex plane and takes FA(u,v) = (Z(u,v) + conj Z(-u,-v)) / 2 and
 *   FB(u,v) = (Z(u,v) - conj Z(-u,-v)) / (2i): two forward passes, no inverse.  Its twiddle table is conjugate-symmetric
 *   (entry len - k is the conjugate of entry k bit for bit), so a plane b that is exactly 0 gives FB = 0 and pb = 0 exactly.
 * Workspace.  As in svae_ctfcorr.h: an n x m plane needs 32 n m + 16 (n + m) bytes; while that fits the 160 KiB of LDS of one
 *   compute unit (up to 71 x 71) the *_workspace_bytes calls return 0 and `ws` may be NULL; larger planes live in a
 *   per-workgroup slice of `ws` (256-byte aligned, at least *_workspace_bytes long; at most 512 slices, the grid striding over
 *   the planes) with only the twiddles in LDS: the same arithmetic in the same order.
 *
 * svae_frc: a, b (planes, n, m) doubles; sums (planes, R, 3) doubles; frc (planes, R) doubles; ring_count (R) int32.  For each
 *   plane p and ring r, over the ring's frequencies in ascending e = u m + v, each sum started from +0:
 *   sums[p, r] = [ sum Re(FA conj FB), sum |FA|^2, sum |FB|^2 ] = [num, pa, pb]; frc[p, r] = num / sqrt(pa pb), and exactly 0
 *   where pa pb == 0.  ring_count[r] is the number of frequencies in ring r; it depends on the shape only and is written by
 *   the workgroup that handles plane 0.  One workgroup of 256 per plane, no atomics.  SVAE_E_INVALID: n or m outside 2..1024,
 *   planes < 1, planes n m >= 2^31, a null a, b, sums, frc or ring_count, a or b overlapping an output, a negative or
 *   non-finite mask_radius, mask_radius > 0 with a mask_edge that is not positive and finite, a workspace that is null,
 *   misaligned or too small where one is needed.
 *
 * svae_frc_filter: x (planes, n, m) doubles, weight (planes, R) doubles, out (planes, n, m) floats:
 *   out[p] = Re IDFT( weight[p, ring(u,v)] DFT(x[p]) ), a frequency in no ring contributing 0.  The arithmetic, the 1/(n m) and
 *   the single rounding to float are those of svae_wiener_finish.  No mask.  SVAE_E_INVALID: n or m outside 2..1024,
 *   planes < 1, planes n m >= 2^31, a null x, weight or out, x or weight overlapping out, a workspace that is null, misaligned
 *   or too small where one is needed.
 *
 * Both launches are filed under the `augment` kind of svae_profile_read.  A refused call leaves every buffer untouched.
 */
#ifndef SVAE_FRC_H
#define SVAE_FRC_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t svae_frc_workspace_bytes(int32_t planes, int32_t n, int32_t m);
int svae_frc(const double* a, const double* b, int32_t planes, int32_t n, int32_t m, double mask_radius, double mask_edge,
             double* sums, double* frc, int32_t* ring_count, void* ws, size_t ws_bytes, svae_stream_t stream);
size_t svae_frc_filter_workspace_bytes(int32_t planes, int32_t n, int32_t m);
int svae_frc_filter(const double* x, const double* weight, int32_t planes, int32_t n, int32_t m, float* out, void* ws,
                    size_t ws_bytes, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_FRC_H */
