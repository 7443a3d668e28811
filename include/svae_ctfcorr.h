/*
 * svae_ctfcorr.h -- CTF correction of observed particles in Fourier space: phase flipping, multiplication by the transfer
 * function, per-class sums of the squared transfer functions and the Wiener quotient of a class sum by them.
 *
 * An addition to the C ABI of svae.h (same library, same conventions: device pointers, nothing allocates or synchronises,
 * work is enqueued on `stream`, 0 or SVAE_E_* with svae_last_error; SVAE_ABI_VERSION unchanged), in a header of its own so
 * that svae.h, svae_stream.h and svae_align.h stay, declaration for declaration, what their users and tests hold them to.
 * The reference has no counterpart: it applies its CTF filters to the decoder's output inside the likelihood and never
 * corrects an observed image.
 *
 * Transfer function.  `params` is (B, 8) doubles, one row per image in the column order of svae_ctf_filter: defocus um, cs mm,
 *   voltage kV, apix A, bfactor, ampcont %, dfdiff, dfang deg.  c_i is the closed form svae_ctf_filter evaluates (both defoci
 *   are defocus*10000, dfdiff is unused, so dfang does not enter either; the B-factor envelope is included; doubles), here on
 *   the IMAGE'S OWN grid: frequency (a, b) of an n x m image is (fftfreq(n)[a], fftfreq(m)[b]) / (apix*scale), in numpy's
 *   fftfreq order.  H_i = -c_i, the sign svae_ctf_filter's real-space filters carry.  u_i = sqrt(1-w^2) sin(gamma) - w cos(gamma)
 *   is c_i without the envelope, and s_i = (u_i <= 0) ? +1 : -1 is the sign of H_i taken from it: the envelope underflows H
 *   at high frequency but never changes its sign.
 *   Because both defoci are equal, H_i is radially symmetric in physical frequency, so on a square box multiplying by a
 *   function of H_i commutes with the in-plane rotation and the translation of svae_align_images: correct the raw observed
 *   image (which has no zero-filled border), then align.  Were astigmatism honoured, the transfer function would have to be
 *   rotated with the image; that is not built.
 * DFT.  Unnormalised forward transform, 1/(n m) on the inverse (numpy's convention).  Separable, rows then columns, doubles
 *   with contraction off, twiddles from a sincospi table indexed by k*v mod len, every sum in index order: two runs give the
 *   same bits.  The imaginary part of the inverse is dropped and the result rounded to float once.
 * Workspace.  An n x m plane needs 32 n m + 16 (n + m) bytes.  While that fits the 160 KiB of LDS of one compute unit (up to
 *   71 x 71) the *_workspace_bytes calls return 0 and `ws` may be NULL; larger planes live in a per-workgroup slice of `ws`
 *   (256-byte aligned, at least *_workspace_bytes long) with only the twiddles in LDS: the same arithmetic in the same order.
 *   n + m <= 10240 (svae_ctf_filter's limit).
 *
 * svae_ctf_apply: y, out (B, n, m) floats (one channel), two buffers that do not overlap.  mode SVAE_CTF_FLIP:
 *   out_i = Re IDFT( s_i * DFT(y_i) ); SVAE_CTF_MULTIPLY: out_i = Re IDFT( H_i * DFT(y_i) ).  One workgroup per image; with a
 *   workspace the grid strides over the images.  SVAE_E_INVALID: n < 2 or m < 2, B < 1, B*n*m >= 2^31, n + m > 10240, scale
 *   not positive, a mode that is neither constant below, a null y, out or params, y and out overlapping, a workspace that is
 *   null, misaligned or too small where one is needed.
 *
 * svae_ctf_power_update: den (n_classes, n, m) doubles, in fftfreq order, that the caller zeroes once; label (B).  A call adds,
 *   for every image b of this call with 0 <= label[b] < n_classes, IN INDEX ORDER, H_b(a,b)^2 into den[label[b], a, b].  Labels
 *   outside the range (use -1) are skipped.  One thread per (class, frequency) walks the B labels and evaluates the closed form
 *   only where the label matches: no atomics, so one call equals two calls on the halves bit for bit.  SVAE_E_INVALID: n < 2
 *   or m < 2, B < 1, n_classes outside 1..4096, n_classes*n*m >= 2^31, scale not positive, a null params, label or den.
 *
 * svae_wiener_finish: sum (n_classes, n, m) doubles, real-space class sums of aligned, CTF-multiplied images (what
 *   svae_class_sums_update accumulates at C == 1); den as above; average (n_classes, n, m) floats:
 *   average[k] = Re IDFT( DFT(sum[k]) / (den[k] + lambda) ).  A frequency whose den + lambda is 0 contributes 0, so lambda = 0
 *   is legal.  One workgroup per class; with a workspace the grid strides over the classes.  SVAE_E_INVALID: n < 2 or m < 2,
 *   n_classes outside 1..4096, n_classes*n*m >= 2^31, n + m > 10240, a negative or non-finite lambda, a null sum, den or
 *   average, a workspace that is null, misaligned or too small where one is needed.
 *
 * All three launches are filed under the `augment` kind of svae_profile_read.  A refused call leaves every buffer untouched.
 */
#ifndef SVAE_CTFCORR_H
#define SVAE_CTFCORR_H

#include "svae.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVAE_CTF_FLIP 0
#define SVAE_CTF_MULTIPLY 1

size_t svae_ctf_apply_workspace_bytes(int32_t B, int32_t n, int32_t m);
int svae_ctf_apply(const float* y, const double* params, int32_t B, int32_t n, int32_t m, double scale, int32_t mode,
                   float* out, void* ws, size_t ws_bytes, svae_stream_t stream);
int svae_ctf_power_update(const double* params, const int32_t* label, int32_t B, int32_t n, int32_t m, double scale,
                          int32_t n_classes, double* den, svae_stream_t stream);
size_t svae_wiener_finish_workspace_bytes(int32_t n_classes, int32_t n, int32_t m);
int svae_wiener_finish(const double* sum, const double* den, double lambda, int32_t n_classes, int32_t n, int32_t m,
                       float* average, void* ws, size_t ws_bytes, svae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SVAE_CTFCORR_H */
