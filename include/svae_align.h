/*
 * svae_align.h -- bring observed images into the model's canonical frame, and accumulate class sums of the result.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h and svae_stream.h stay, declaration for declaration, what their users and tests hold them to.  The reference
 * has no counterpart: it ends at .sav files and PNG dumps of one minibatch.  svae_rotate_bicubic is a different thing (Pillow's
 * Image.rotate bit for bit, from host-made matrices, with Pillow's cubic and no notion of coverage) and is not used here.
 *
 * Geometry.  The decoder sees pixel i of image b at x''[b,i] = grid[i] @ [[cos t, sin t], [-sin t, cos t]] + dx[b]
 * (svae_pose), on the grid column jx -> -1 + 2 jx/(cols-1), row jy -> 1 - 2 jy/(rows-1), y up.  The canonical image is
 * A[j] = f(grid[j]), so output pixel j is read from the observed image at the grid position p = (grid[j] - dx) R^T.  In
 * centred pixel units, with a = (cols-1)/2, bq = (rows-1)/2, X = jx - a, Y = bq - jy, c = cos(theta), s = sin(theta)
 * (double, from (double)theta; theta NULL means c = 1, s = 0 exactly; dx NULL means 0):
 *
 *     U  = X - a*dx0              V  = Y - bq*dx1
 *     SX = c*U + s*(a/bq)*V       SY = -s*(bq/a)*U + c*V
 *     fx = SX + a                 fy = bq - SY            (source column / row, continuous)
 *
 * so the identity pose reads every pixel from itself, exactly.
 *   Coverage.  A pixel is covered iff -1e-6 <= fx <= cols-1+1e-6 and -1e-6 <= fy <= rows-1+1e-6 (the slack lets a quarter
 *     turn cover the whole image although cos(pi/2) != 0); covered positions are clamped to [0, cols-1] x [0, rows-1].
 *     Uncovered pixels (a non-finite pose among them) get 0 in every channel and cover = 0.
 *   SVAE_ALIGN_BILINEAR.  i0 = min(floor(fx), cols-2), t = fx - i0, value (1-t) s0 + t s1 along a row; the two rows j0 =
 *     min(floor(fy), rows-2), j0+1 are then combined the same way with u = fy - j0.
 *   SVAE_ALIGN_BICUBIC.  Catmull-Rom (a = -0.5) on the taps i0-1 .. i0+2 (same i0, t), indices clamped to the image, with the
 *     weights (-t^3+2t^2-t)/2, (3t^3-5t^2+2)/2, (-3t^3+4t^2+t)/2, (t^3-t^2)/2; the four taps of a row are summed left to
 *     right, then the four rows j0-1 .. j0+2 top to bottom with the weights of u.
 *   All arithmetic is in double with contraction off, and the result is rounded to float once.
 *
 * svae_align_images: y, aligned (B, rows*cols, C), distinct buffers that do not overlap; theta (B) or NULL; dx (B, 2) or NULL,
 *   in the decoder's units (already times dx_scale); cover (B, rows*cols), 1 = covered, or NULL.  One thread per output
 *   element.  SVAE_E_INVALID: rows < 2, cols < 2, C outside 1..SVAE_MAX_OUT, B < 1, B*rows*cols*C >= 2^31, an interp that is
 *   neither constant below, a null y or aligned, y and aligned overlapping.
 *
 * svae_class_sums_update: aligned (B, N, C) and cover (B, N) or NULL (= covered everywhere) as written by svae_align_images
 *   (N = rows*cols), label (B); sum (n_classes, N, C) and count (n_classes, N) are doubles the caller zeroes once.  A call
 *   adds, for every class k and every image b of this call with label[b] == k, IN INDEX ORDER, aligned[b,j,c] (float to
 *   double: exact) into sum[k,j,c] and 1 into count[k,j] wherever cover[b,j] != 0.  Labels outside [0, n_classes) (use -1)
 *   are skipped.  One thread per (class, pixel) walks the B labels: no atomics, so the sums are a function of the sequence of
 *   calls alone and two runs are bit-equal.  SVAE_E_INVALID: B < 1, N < 1, C outside 1..SVAE_MAX_OUT, n_classes outside
 *   1..4096, B*N*C or n_classes*N*C >= 2^31, a null aligned, label, sum or count.
 *
 * Both launches are filed under the `augment` kind of svae_profile_read.  A refused call leaves every buffer untouched.
 */
#ifndef SVAE_ALIGN_H
#define SVAE_ALIGN_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_ALIGN_BILINEAR 0
#define SVAE_ALIGN_BICUBIC 1

int svae_align_images(const float* y, const float* theta, const float* dx, int32_t B, int32_t rows, int32_t cols,
                      int32_t C, int32_t interp, float* aligned, uint8_t* cover, svae_stream_t stream);
int svae_class_sums_update(const float* aligned, const uint8_t* cover, const int32_t* label, int32_t B, int32_t N,
                           int32_t C, int32_t n_classes, double* sum, double* count, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_ALIGN_H */
