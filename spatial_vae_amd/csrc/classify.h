// Multi-reference alignment (include/svae_classify.h).  A prologue, one workgroup of 256 per reference, takes each reference's
// sum (weight * ref)^2 once per call.  The main kernel runs one workgroup of 256 per image (SCRATCH: the grid strides over the
// images) with the angle loop outermost: the image is resampled ONCE per angle into the plane P_k, as doubles, by align.h's
// align_sample, and that plane is correlated with every live candidate at every shift, each single correlation one wave's
// work in refine.h's order (lanes striding over the pixels, a butterfly closing the sum), so that a candidate's maximum is bit
// for bit the score of refine.h's pose search against that reference; a wave takes nine shifts in one pass over its pixels, so
// weight, reference and pixel index are read once for nine multiply-adds from the plane.  With M >= 4 a wave takes whole
// candidates and keeps their running maximum alone; with fewer the waves share each candidate's shifts and combine their
// maxima in turn.  Plane and maxima stay in LDS, or in the workgroup's slice of the workspace above the LDS limit: the same
// arithmetic in the same order.  The winner and the runner-up are thread 0's walk at the end.  Doubles with contraction off,
// no atomics.
// tests/classify_ref.py is the float64 restatement the kernel is held to.
#pragma once
#include "refine.h"

namespace svae {

struct ClassifyGeo {
    int B, n_ref, M, rows, cols, C, A, S;
    double step;
};

// norms[r] = sum over (j, c) of (weight[j] * ref[r, j, c])^2: the loop and the block sum of pose_search_kernel's ref_sq
__global__ void __launch_bounds__(256) classify_norms_kernel(const double* __restrict__ ref, const double* __restrict__ weight, int NC,
                                                              int C, double* __restrict__ norms) {
#pragma clang fp contract(off)
    __shared__ double red[8];
    const int tid = threadIdx.x;
    const double* rp = ref + (long)blockIdx.x * NC;
    double part = 0.0;
    for (int e = tid; e < NC; e += 256) {
        const double wr = weight ? weight[e / C] * rp[e] : rp[e];
        part += wr * wr;
    }
    const double ref_sq = refine_block_sum(part, red);
    if (tid == 0) norms[blockIdx.x] = ref_sq;
}

constexpr int kClassifyShifts = 9;    // shifts one pass over the pixels serves: the whole 3 x 3 of S = 1, 9 + 9 + 7 of S = 2

// The correlations of the plane with weight * rp at the `count` (<= kClassifyShifts) shifts q0, q0 + dq, ...: one wave's work,
// the same bits in every lane.  One pass over the lane's pixels reads weight and reference once and feeds every shift's
// accumulator, so each single sum still runs over its pixels upwards in refine.h's order; a shift past `count` sees no pixel.
__device__ __forceinline__ void classify_correlate(const double* __restrict__ plane, const double* __restrict__ rp,
                                                   const double* __restrict__ weight, int q0, int dq, int count, int nS, int S, int h,
                                                   int w, int C, int lane, double acc[kClassifyShifts]) {
#pragma clang fp contract(off)
    const int N = h * w;
    int sy[kClassifyShifts], sx[kClassifyShifts];
#pragma unroll
    for (int t = 0; t < kClassifyShifts; ++t) {
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
        for (int t = 0; t < kClassifyShifts; ++t) {
            const int yy = jy + sy[t], xx = jx - sx[t];
            if (yy < 0 || yy >= h || xx < 0 || xx >= w) continue;
            const double* src = plane + ((long)yy * w + xx) * C;
#pragma unroll
            for (int ch = 0; ch < SVAE_MAX_OUT; ++ch)
                if (ch < C) acc[t] += wr[ch] * src[ch];
        }
    }
#pragma unroll
    for (int t = 0; t < kClassifyShifts; ++t) acc[t] = refine_wave_sum(acc[t]);
}

template <bool CUBIC, bool SCRATCH>
__global__ void __launch_bounds__(256) pose_classify_kernel(const float* __restrict__ y, const double* __restrict__ ref,
                                                             const double* __restrict__ weight, const int* __restrict__ cand,
                                                             const float* __restrict__ pose_in, ClassifyGeo g,
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
                const double thk = th + (double)k * g.step;
                const double c = cos(thk), s = sin(thk);
                double part = 0.0;
                for (int e = tid; e < NC; e += 256) {
                    const int pix = e / C, ch = e - pix * C;
                    const int jy = pix / w, jx = pix - jy * w;
                    bool covered;
                    const double v = align_sample<CUBIC>(img, c, s, dx0, dx1, jy, jx, ch, h, w, C, &covered);
                    plane[e] = v;
                    part += v * v;
                }
                const double p_sq = refine_block_sum(part, red);        // its barriers also publish the plane and the maxima
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
                        for (int q0 = 0; q0 < nQ; q0 += kClassifyShifts) {
                            const int count = min(kClassifyShifts, nQ - q0);
                            double acc[kClassifyShifts];
                            classify_correlate(plane, rp, weight, q0, 1, count, nS, g.S, h, w, C, lane, acc);
#pragma unroll
                            for (int t = 0; t < kClassifyShifts; ++t) {
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
                        for (int q0 = wave; q0 < nQ; q0 += 4 * kClassifyShifts) {     // this wave's shifts: wave, wave + 4, ...
                            const int count = min(kClassifyShifts, (nQ - q0 + 3) / 4);
                            double acc[kClassifyShifts];
                            classify_correlate(plane, rp, weight, q0, 4, count, nS, g.S, h, w, C, lane, acc);
#pragma unroll
                            for (int t = 0; t < kClassifyShifts; ++t) {
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
