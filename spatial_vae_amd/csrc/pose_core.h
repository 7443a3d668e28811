// What the three pose kernels share (refine.h, classify.h, expect.h), each piece written once: the geometry, the two fixed-order
// sums, the resampling of the image at one angle into the plane P_k (as doubles, by align.h's align_sample), the references'
// norms, and the shifted correlation of the plane with weight * ref.  Every single correlation is one wave's work, the lanes
// striding over the pixels and a butterfly closing the sum: that one order is why a candidate's maximum in svae_pose_classify
// and a D of svae_pose_expect are bit for bit svae_pose_search's numbers.  Doubles with contraction off, no atomics.
// The read of an image's (theta, dx0, dx1) with its finiteness test stays a line of each kernel: as a function of this file the
// test compiles to other code in each kernel's per-image prologue, and svae_pose_expect then measured 2.6 % slower.
#pragma once
#include "align.h"

namespace svae {

struct PoseGeo {
    int B, n_ref, M, rows, cols, C, A, S;     // M = 1 for the search
    double step, inv_sigma2;                  // inv_sigma2 = 0 where unused
};

// the sum of v over the 64 lanes of the wave, the same bits in every lane (each level adds the two partners' values, and
// IEEE addition commutes)
__device__ __forceinline__ double pose_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the sum of v over the 256 threads: waves first, then the four wave sums in index order.  Every thread gets the result;
// `red` (4 doubles of LDS) is free again on return.
__device__ __forceinline__ double pose_block_sum(double v, double* red) {
#pragma clang fp contract(off)
    v = pose_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return t;
}

// The image at angle k into the plane and, with COVER, its coverage (1.0 / 0.0) into cov; the caller's barrier publishes both.
// Returns the thread's part of the plane's sum of squares, which pose_block_sum closes.
template <bool CUBIC, bool COVER>
__device__ __forceinline__ double pose_resample(const float* __restrict__ img, double th, double dx0, double dx1, int k, double step,
                                                int h, int w, int C, double* __restrict__ plane, double* __restrict__ cov) {
#pragma clang fp contract(off)
    const double thk = th + (double)k * step;
    const double c = cos(thk), s = sin(thk);
    const int NC = h * w * C;
    double part = 0.0;
    for (int e = threadIdx.x; e < NC; e += 256) {
        const int pix = e / C, ch = e - pix * C;
        const int jy = pix / w, jx = pix - jy * w;
        bool covered;
        const double v = align_sample<CUBIC>(img, c, s, dx0, dx1, jy, jx, ch, h, w, C, &covered);
        plane[e] = v;
        part += v * v;
        if (COVER && ch == 0) cov[pix] = covered ? 1.0 : 0.0;
    }
    return part;
}

// sum over (pix, c) of wr * wr (SQUARED) or wr * ref (not), wr = weight[pix] * rp[pix, c] (rp itself where weight is NULL):
// per thread with stride 256, then the block sum
template <bool SQUARED>
__device__ __forceinline__ double pose_ref_sum(const double* __restrict__ rp, const double* __restrict__ weight, int NC, int C,
                                               double* red) {
#pragma clang fp contract(off)
    double part = 0.0;
    for (int e = threadIdx.x; e < NC; e += 256) {
        const double wr = weight ? weight[e / C] * rp[e] : rp[e];
        part += SQUARED ? wr * wr : wr * rp[e];
    }
    return pose_block_sum(part, red);
}

// norms[r] = pose_ref_sum<SQUARED> of reference r: one workgroup of 256 per reference
template <bool SQUARED>
__global__ void __launch_bounds__(256) pose_norms_kernel(const double* __restrict__ ref, const double* __restrict__ weight, int NC,
                                                          int C, double* __restrict__ norms) {
    __shared__ double red[8];
    const double sum = pose_ref_sum<SQUARED>(ref + (long)blockIdx.x * NC, weight, NC, C, red);
    if (threadIdx.x == 0) norms[blockIdx.x] = sum;
}

constexpr int kPoseShifts = 9;    // shifts one pass over the pixels serves: the whole 3 x 3 of S = 1, 9 + 9 + 7 of S = 2

// The correlations of the plane with weight * rp at the `count` (<= kPoseShifts) shifts q0, q0 + dq, ...: one wave's work,
// the same bits in every lane.  One pass over the lane's pixels reads weight and reference once and feeds every shift's
// accumulator, so each single sum runs over its pixels upwards, channels innermost; a shift past `count` sees no pixel.
__device__ __forceinline__ void pose_correlate(const double* __restrict__ plane, const double* __restrict__ rp,
                                               const double* __restrict__ weight, int q0, int dq, int count, int nS, int S, int h,
                                               int w, int C, int lane, double acc[kPoseShifts]) {
#pragma clang fp contract(off)
    const int N = h * w;
    int sy[kPoseShifts], sx[kPoseShifts];
#pragma unroll
    for (int t = 0; t < kPoseShifts; ++t) {
        const int q = q0 + t * dq;
        sy[t] = t < count ? q / nS - S : h;         // row jy + h is outside every box
        sx[t] = t < count ? q - (q / nS) * nS - S : 0;
        acc[t] = 0.0;
    }
    for (int pix = lane; pix < N; pix += 64) {
        const int jy = pix / w, jx = pix - jy * w;
        const double wt = weight ? weight[pix] : 1.0;
        const double* rr = rp + (long)pix * C;
        double wr[SVAE_MAX_OUT];
#pragma unroll
        for (int ch = 0; ch < SVAE_MAX_OUT; ++ch)
            if (ch < C) wr[ch] = weight ? wt * rr[ch] : rr[ch];
#pragma unroll
        for (int t = 0; t < kPoseShifts; ++t) {
            const int yy = jy + sy[t], xx = jx - sx[t];
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const double* src = plane + ((long)yy * w + xx) * C;
#pragma unroll
            for (int ch = 0; ch < SVAE_MAX_OUT; ++ch)
                if (ch < C) acc[t] += wr[ch] * src[ch];
        }
    }
#pragma unroll
    for (int t = 0; t < kPoseShifts; ++t) acc[t] = pose_wave_sum(acc[t]);
}

}  // namespace svae
