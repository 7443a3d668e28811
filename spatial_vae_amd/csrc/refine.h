// Reference-based pose search (include/svae_refine.h).  One workgroup of 256 per image (SCRATCH: the grid strides over the
// images).  Per angle the image is resampled once into the plane P_k; its (2S+1)^2 shifted correlations with weight * ref are
// pose_core.h's pose_correlate, the four waves sharing the shifts as classify.h's M < 4 branch does (wave, wave + 4, ...).  The
// image's score volume stays beside the plane (LDS, or the workgroup's slice of the workspace above the LDS limit: the same
// arithmetic in the same order); the winner and the three parabolas are thread 0's work at the end.  tests/refine_ref.py is
// the float64 restatement the kernel is held to.
#pragma once
#include "pose_core.h"

namespace svae {

// the sub-step offset of a winner with the neighbours l and r along one axis
__device__ __forceinline__ double refine_parabola(double l, double c, double r) {
#pragma clang fp contract(off)
    const double d = l - 2.0 * c + r;
    if (!(d < 0.0)) return 0.0;
    return fmin(fmax(0.5 * (l - r) / d, -0.5), 0.5);
}

template <bool CUBIC, bool SCRATCH>
__global__ void __launch_bounds__(256) pose_search_kernel(const float* __restrict__ y, const double* __restrict__ ref,
                                                           const double* __restrict__ weight, const int* __restrict__ ref_index,
                                                           const float* __restrict__ pose_in, PoseGeo g,
                                                           float* __restrict__ pose_out, double* __restrict__ score,
                                                           int* __restrict__ offset, double* __restrict__ scores,
                                                           double* __restrict__ scratch, long slice) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_refine[];
    const int N = g.rows * g.cols, NC = N * g.C;
    const int nA = 2 * g.A + 1, nS = 2 * g.S + 1, nQ = nS * nS, V = nA * nQ;
    double* red = lds_refine;                                   // 8 doubles: 4 of the block sums, 4 spare
    double* plane = SCRATCH ? scratch + (long)blockIdx.x * slice : lds_refine + 8;
    double* vol = plane + NC;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = g.rows, w = g.cols, C = g.C;
    const double a = (double)(w - 1) / 2.0, bq = (double)(h - 1) / 2.0;
    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const double th = (double)pose_in[3 * b], dx0 = (double)pose_in[3 * b + 1], dx1 = (double)pose_in[3 * b + 2];
        const int r = ref_index[b];
        bool skip = r < 0 || r >= g.n_ref || !isfinite(th) || !isfinite(dx0) || !isfinite(dx1);   // uniform over the workgroup
        const double* rp = ref + (long)(skip ? 0 : r) * NC;
        double ref_sq = 0.0;
        if (!skip) {
            ref_sq = pose_ref_sum<true>(rp, weight, NC, C, red);
            skip = ref_sq == 0.0;
        }
        if (skip) {
            for (int i = tid; i < V; i += 256) vol[i] = 0.0;
        } else {
            const double ref_norm = sqrt(ref_sq);
            const float* img = y + (long)b * NC;
            for (int k = -g.A; k <= g.A; ++k) {
                const double part = pose_resample<CUBIC, false>(img, th, dx0, dx1, k, g.step, h, w, C, plane, nullptr);
                const double p_sq = pose_block_sum(part, red);          // its barriers also publish the plane
                const double denom = ref_norm * sqrt(p_sq);
                double* vk = vol + (k + g.A) * nQ;
                for (int q0 = wave; q0 < nQ; q0 += 4 * kPoseShifts) {   // this wave's shifts: wave, wave + 4, ...
                    const int count = min(kPoseShifts, (nQ - q0 + 3) / 4);
                    double acc[kPoseShifts];
                    pose_correlate(plane, rp, weight, q0, 4, count, nS, g.S, h, w, C, lane, acc);
#pragma unroll
                    for (int t = 0; t < kPoseShifts; ++t)
                        if (lane == 0 && t < count) vk[q0 + 4 * t] = p_sq == 0.0 ? 0.0 : acc[t] / denom;
                }
                __syncthreads();    // the waves have finished with the plane before the next angle overwrites it
            }
        }
        __syncthreads();            // the volume is complete
        if (scores)
            for (int i = tid; i < V; i += 256) scores[(long)b * V + i] = vol[i];
        if (tid == 0) {
            int best = -1;
            double top = -INFINITY;
            if (!skip)
                for (int i = 0; i < V; ++i)
                    if (vol[i] > top) {
                        top = vol[i];
                        best = i;
                    }
            float* po = pose_out + 3 * b;
            int* off = offset + 4 * b;
            if (best < 0) {
                po[0] = pose_in[3 * b];
                po[1] = pose_in[3 * b + 1];
                po[2] = pose_in[3 * b + 2];
                score[b] = 0.0;
                off[0] = off[1] = off[2] = 0;
                off[3] = 4;
            } else {
                const int ik = best / (nS * nS), iy = (best - ik * nS * nS) / nS, ix = best - ik * nS * nS - iy * nS;
                int flags = 0;
                double fk = 0.0, fx = 0.0, fy = 0.0;
                if (ik > 0 && ik < nA - 1) fk = refine_parabola(vol[best - nS * nS], top, vol[best + nS * nS]);
                else if (nA > 1) flags |= 1;
                if (ix > 0 && ix < nS - 1) fx = refine_parabola(vol[best - 1], top, vol[best + 1]);
                else if (nS > 1) flags |= 2;
                if (iy > 0 && iy < nS - 1) fy = refine_parabola(vol[best - nS], top, vol[best + nS]);
                else if (nS > 1) flags |= 2;
                const int k = ik - g.A, sx = ix - g.S, sy = iy - g.S;
                po[0] = (float)(th + ((double)k + fk) * g.step);
                po[1] = (float)(dx0 + ((double)sx + fx) / a);
                po[2] = (float)(dx1 + ((double)sy + fy) / bq);
                score[b] = top;
                off[0] = k;
                off[1] = sx;
                off[2] = sy;
                off[3] = flags;
            }
        }
        __syncthreads();            // thread 0 has read the volume before the next image's candidates overwrite it
    }
}

}  // namespace svae
