// Multi-reference alignment (include/svae_classify.h).  A prologue (pose_norms_kernel<true>) takes each reference's
// sum (weight * ref)^2 once per call.  The main kernel runs one workgroup of 256 per image (SCRATCH: the grid strides over the
// images) with the angle loop outermost: the image is resampled ONCE per angle into the plane P_k, and that plane is
// correlated with every live candidate at every shift by pose_core.h's pose_correlate, so that a candidate's maximum is bit
// for bit the score of refine.h's pose search against that reference.  With M >= 4 a wave takes whole candidates and keeps
// their running maximum alone; with fewer the waves share each candidate's shifts and combine their maxima in turn.  Plane
// and maxima stay in LDS, or in the workgroup's slice of the workspace above the LDS limit: the same arithmetic in the same
// order.  The winner and the runner-up are thread 0's walk at the end.
// tests/classify_ref.py is the float64 restatement the kernel is held to.
#pragma once
#include "pose_core.h"

namespace svae {

template <bool CUBIC, bool SCRATCH>
__global__ void __launch_bounds__(256) pose_classify_kernel(const float* __restrict__ y, const double* __restrict__ ref,
                                                             const double* __restrict__ weight, const int* __restrict__ cand,
                                                             const float* __restrict__ pose_in, PoseGeo g,
                                                             const double* __restrict__ norms, int* __restrict__ choice,
                                                             int* __restrict__ ref_chosen, double* __restrict__ cand_score,
                                                             double* __restrict__ margin, double* __restrict__ scratch, long slice) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_classify[];
    const int N = g.rows * g.cols, NC = N * g.C, M = g.M;
    const int nS = 2 * g.S + 1, nQ = nS * nS;
    double* red = lds_classify;                                 // 8 doubles: 4 of the block sums, 4 spare
    double* plane = SCRATCH ? scratch + (long)blockIdx.x * slice : lds_classify + 8;
    double* top = plane + NC;                                   // the M running maxima
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = g.rows, w = g.cols, C = g.C;
    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const double th = (double)pose_in[3 * b], dx0 = (double)pose_in[3 * b + 1], dx1 = (double)pose_in[3 * b + 2];
        const bool skip = !isfinite(th) || !isfinite(dx0) || !isfinite(dx1);    // uniform over the workgroup
        const int* cb = cand + (long)b * M;
        for (int j = tid; j < M; j += 256) top[j] = -INFINITY;
        if (!skip) {
            const float* img = y + (long)b * NC;
            for (int k = -g.A; k <= g.A; ++k) {
                const double part = pose_resample<CUBIC, false>(img, th, dx0, dx1, k, g.step, h, w, C, plane, nullptr);
                const double p_sq = pose_block_sum(part, red);          // its barriers also publish the plane and the maxima
                const double p_norm = sqrt(p_sq);
                if (M >= 4) {
                    for (int j = wave; j < M; j += 4) {                 // whole candidates: no two waves touch the same maximum
                        const int r = cb[j];
                        if (r < 0 || r >= g.n_ref) continue;
                        const double ref_sq = norms[r];
                        if (ref_sq == 0.0) continue;
                        const double denom = sqrt(ref_sq) * p_norm;
                        const double* rp = ref + (long)r * NC;
                        double best = -INFINITY;
                        for (int q0 = 0; q0 < nQ; q0 += kPoseShifts) {
                            const int count = min(kPoseShifts, nQ - q0);
                            double acc[kPoseShifts];
                            pose_correlate(plane, rp, weight, q0, 1, count, nS, g.S, h, w, C, lane, acc);
#pragma unroll
                            for (int t = 0; t < kPoseShifts; ++t) {
                                const double sc = p_sq == 0.0 ? 0.0 : acc[t] / denom;
                                if (t < count && sc > best) best = sc;
                            }
                        }
                        if (lane == 0 && best > top[j]) top[j] = best;
                    }
                    __syncthreads();    // the waves have finished with the plane before the next angle overwrites it
                } else {
                    double best[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
                    for (int j = 0; j < 3; ++j) {                       // the shifts of each candidate shared over the waves
                        if (j >= M) continue;
                        const int r = cb[j];
                        if (r < 0 || r >= g.n_ref) continue;
                        const double ref_sq = norms[r];
                        if (ref_sq == 0.0) continue;
                        const double denom = sqrt(ref_sq) * p_norm;
                        const double* rp = ref + (long)r * NC;
                        for (int q0 = wave; q0 < nQ; q0 += 4 * kPoseShifts) {         // this wave's shifts: wave, wave + 4, ...
                            const int count = min(kPoseShifts, (nQ - q0 + 3) / 4);
                            double acc[kPoseShifts];
                            pose_correlate(plane, rp, weight, q0, 4, count, nS, g.S, h, w, C, lane, acc);
#pragma unroll
                            for (int t = 0; t < kPoseShifts; ++t) {
                                const double sc = p_sq == 0.0 ? 0.0 : acc[t] / denom;
                                if (t < count && sc > best[j]) best[j] = sc;
                            }
                        }
                    }
                    for (int turn = 0; turn < 4; ++turn) {              // the waves fold their maxima in, one after the other
                        if (wave == turn && lane == 0) {
#pragma unroll
                            for (int j = 0; j < 3; ++j)
                                if (j < M && best[j] > top[j]) top[j] = best[j];
                        }
                        __syncthreads();                                // the last one also frees the plane for the next angle
                    }
                }
            }
        }
        __syncthreads();                // the maxima are complete (and initialised, for a skipped image)
        for (int j = tid; j < M; j += 256) cand_score[(long)b * M + j] = top[j];
        if (tid == 0) {
            int first = -1;
            double high = -INFINITY, second = -INFINITY;
            for (int j = 0; j < M; ++j)
                if (top[j] > high) {
                    high = top[j];
                    first = j;
                }
            for (int j = 0; j < M; ++j)
                if (j != first && top[j] > second) second = top[j];
            choice[b] = first;
            ref_chosen[b] = first < 0 ? -1 : cb[first];
            if (margin) margin[b] = (first >= 0 && second > -INFINITY) ? high - second : INFINITY;
        }
        __syncthreads();                // thread 0 has read the maxima before the next image's overwrite them
    }
}

}  // namespace svae
