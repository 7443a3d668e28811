// Alignment into the model's canonical frame (include/svae_align.h): each observed image resampled at the positions the
// decoder's pose transform maps its grid to, with the poses read from device memory, a coverage mask, and per-class sums of
// the result.  The geometry, the two interpolations and the order of every sum are stated in the header; tests/align_ref.py
// is the float64 restatement the kernels are held to.  Doubles with contraction off, one rounding to float on the way out;
// no LDS, no atomics.
#pragma once
#include "common.h"

namespace svae {

struct AlignGeo {
    int B, rows, cols, C;
};

// Catmull-Rom weights of the taps i0-1 .. i0+2 at the fraction t
__device__ __forceinline__ void align_cubic_weights(double t, double w[4]) {
#pragma clang fp contract(off)
    const double t2 = t * t, t3 = t2 * t;
    w[0] = (-t3 + 2.0 * t2 - t) / 2.0;
    w[1] = (3.0 * t3 - 5.0 * t2 + 2.0) / 2.0;
    w[2] = (-3.0 * t3 + 4.0 * t2 + t) / 2.0;
    w[3] = (t3 - t2) / 2.0;
}

// The canonical-frame value of output pixel (jy, jx), channel ch, of the image `img` (h, w, C) at the pose (c = cos theta,
// s = sin theta, dx0, dx1), in double: the header's geometry, coverage, clamping and interpolation, before the one rounding to
// float.  *covered is false (and the value 0) where the observed image does not cover the pixel; a NaN pose lands there too,
// every comparison being false.  align_images_kernel and refine.h's pose search share it.
template <bool CUBIC>
__device__ __forceinline__ double align_sample(const float* __restrict__ img, double c, double s, double dx0, double dx1, int jy,
                                               int jx, int ch, int h, int w, int C, bool* covered_out) {
#pragma clang fp contract(off)
    const double a = (double)(w - 1) / 2.0, bq = (double)(h - 1) / 2.0;
    const double X = (double)jx - a, Y = bq - (double)jy;
    const double U = X - a * dx0, V = Y - bq * dx1;
    const double SX = c * U + s * (a / bq) * V;
    const double SY = -s * (bq / a) * U + c * V;
    double fx = SX + a, fy = bq - SY;
    const bool covered = fx >= -1e-6 && fx <= (double)(w - 1) + 1e-6 && fy >= -1e-6 && fy <= (double)(h - 1) + 1e-6;
    *covered_out = covered;
    if (!covered) return 0.0;
    fx = fmin(fmax(fx, 0.0), (double)(w - 1));
    fy = fmin(fmax(fy, 0.0), (double)(h - 1));
    const int i0 = min((int)floor(fx), w - 2), j0 = min((int)floor(fy), h - 2);
    const double tx = fx - (double)i0, ty = fy - (double)j0;
    auto sample = [&](int yy, int xx) -> double { return (double)img[((long)yy * w + xx) * C + ch]; };
    double v;
    if (CUBIC) {
        double wx[4], wy[4];
        align_cubic_weights(tx, wx);
        align_cubic_weights(ty, wy);
        int xc[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) xc[k] = min(max(i0 - 1 + k, 0), w - 1);
        v = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int yy = min(max(j0 - 1 + r, 0), h - 1);
            const double row = wx[0] * sample(yy, xc[0]) + wx[1] * sample(yy, xc[1]) + wx[2] * sample(yy, xc[2]) +
                               wx[3] * sample(yy, xc[3]);
            v = r == 0 ? wy[0] * row : v + wy[r] * row;
        }
    } else {
        const double r0 = (1.0 - tx) * sample(j0, i0) + tx * sample(j0, i0 + 1);
        const double r1 = (1.0 - tx) * sample(j0 + 1, i0) + tx * sample(j0 + 1, i0 + 1);
        v = (1.0 - ty) * r0 + ty * r1;
    }
    return v;
}

// One thread per output element (b, jy, jx, c); the thread of channel 0 also writes the pixel's coverage.
template <bool CUBIC>
__global__ void align_images_kernel(const float* __restrict__ y, const float* __restrict__ theta, const float* __restrict__ dx,
                                    float* __restrict__ out, uint8_t* __restrict__ cover, AlignGeo g) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const long per = (long)g.rows * g.cols * g.C;
    if (t >= per * g.B) return;
    const int b = (int)(t / per);
    const int rem = (int)(t - (long)b * per);
    const int ch = rem % g.C;
    const int pix = rem / g.C;
    const int jx = pix % g.cols, jy = pix / g.cols;
    double c = 1.0, s = 0.0;
    if (theta) {
        const double th = (double)theta[b];
        c = cos(th);
        s = sin(th);
    }
    const double dx0 = dx ? (double)dx[2 * b] : 0.0, dx1 = dx ? (double)dx[2 * b + 1] : 0.0;
    bool covered;
    const double v = align_sample<CUBIC>(y + (long)b * per, c, s, dx0, dx1, jy, jx, ch, g.rows, g.cols, g.C, &covered);
    if (cover && ch == 0) cover[(long)b * g.rows * g.cols + pix] = covered ? 1 : 0;
    out[t] = covered ? (float)v : 0.0f;
}

// One thread per (class k, pixel j): walks the call's B labels in index order and adds the images of its class into
// sum[k, j, :] and count[k, j].  Every thread of a wave reads the same label (a broadcast), and neighbouring threads
// neighbouring pixels.
__global__ void class_sums_update_kernel(const float* __restrict__ aligned, const uint8_t* __restrict__ cover,
                                         const int* __restrict__ label, int B, int N, int C, int n_classes,
                                         double* __restrict__ sum, double* __restrict__ count) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n_classes * N) return;
    const int k = (int)(t / N);
    const int j = (int)(t - (long)k * N);
    double acc[SVAE_MAX_OUT];
#pragma unroll
    for (int c = 0; c < SVAE_MAX_OUT; ++c) acc[c] = c < C ? sum[t * C + c] : 0.0;
    double n = count[t];
    for (int b = 0; b < B; ++b) {
        if (label[b] != k) continue;
        const long p = (long)b * N + j;
        if (cover && cover[p] == 0) continue;
#pragma unroll
        for (int c = 0; c < SVAE_MAX_OUT; ++c)
            if (c < C) acc[c] += (double)aligned[p * C + c];
        n += 1.0;
    }
#pragma unroll
    for (int c = 0; c < SVAE_MAX_OUT; ++c)
        if (c < C) sum[t * C + c] = acc[c];
    count[t] = n;
}

}  // namespace svae
