// Maximum-likelihood class averages (include/svae_expect.h).  A prologue (pose_norms_kernel<false>) takes each reference's
// h = sum weight * ref^2 once per call.  The main kernel runs one workgroup of 256 per image (SCRATCH: the grid strides
// over the images) in two passes over the angles.  The first resamples the image into the plane P_k and its coverage and
// fills the log-weight volume L: each (slot, nine shifts) is one wave's call of pose_correlate, so every D is bit for bit the
// numerator of svae_pose_classify's score.  Between the passes the workgroup finds the first maximum, the sum of exp(L - Lmax)
// and the posterior p, which takes L's place.  The second pass resamples each angle again and adds p * Q into the image's
// contribution rows: a thread owns (slot, pixel) with all its channels and the coverage, reads p as a broadcast, and carries
// its running sums through global memory from one angle to the next (the same thread, so no atomics).  Plane, coverage and
// volume stay in LDS, or in the workgroup's slice of the workspace above the LDS limit: the same arithmetic in the same order.
// tests/expect_ref.py is the float64 restatement the kernels are held to.
#pragma once
#include "pose_core.h"

namespace svae {

constexpr int kExpectMaxSlots = 64;
constexpr int kExpectFixed = 8 + kExpectMaxSlots / 2;    // doubles of LDS every form keeps: 8 of reduction space, the slot references

template <bool CUBIC, bool SCRATCH>
__global__ void __launch_bounds__(256) pose_expect_kernel(const float* __restrict__ y, const double* __restrict__ ref,
                                                           const double* __restrict__ weight, const double* __restrict__ log_prior,
                                                           const int* __restrict__ cand, const float* __restrict__ pose_in, PoseGeo g,
                                                           const double* __restrict__ hn, double* __restrict__ contrib,
                                                           double* __restrict__ cover_w, double* __restrict__ class_post,
                                                           double* __restrict__ log_evidence, int* __restrict__ best,
                                                           double* __restrict__ scratch, long slice) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_expect[];
    const int h = g.rows, w = g.cols, C = g.C, M = g.M;
    const int N = h * w, NC = N * C;
    const int nA = 2 * g.A + 1, nS = 2 * g.S + 1, nQ = nS * nS, V = nA * nQ, MV = M * V;
    const int G = (nQ + kPoseShifts - 1) / kPoseShifts;             // groups of nine shifts per (slot, angle)
    double* red = lds_expect;                                       // 4 doubles of the block sums / maxima, 4 of the maxima's indices
    int* slots = reinterpret_cast<int*>(lds_expect + 8);            // the reference of each live slot, -1 for a dead one
    double* plane = SCRATCH ? scratch + (long)blockIdx.x * slice : lds_expect + kExpectFixed;
    double* cov = plane + NC;
    double* vol = cov + N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int b = blockIdx.x; b < g.B; b += gridDim.x) {
        const double th = (double)pose_in[3 * b], dx0 = (double)pose_in[3 * b + 1], dx1 = (double)pose_in[3 * b + 2];
        const int* cb = cand + (long)b * M;
        int mine = 0;
        if (tid < M) {
            int r = cb[tid];
            bool live = r >= 0 && r < g.n_ref;
            for (int i = 0; live && i < tid; ++i) live = cb[i] != r;
            if (live && log_prior) live = isfinite(log_prior[r]);
            slots[tid] = live ? r : -1;
            mine = live ? 1 : 0;
        }
        const int any_live = __syncthreads_or(mine);                // also publishes the slots
        bool skip = !any_live || !isfinite(th) || !isfinite(dx0) || !isfinite(dx1);   // uniform over the workgroup
        const float* img = y + (long)b * NC;
        int top_i = 0;
        double top_v = 0.0, Z = 1.0;
        if (!skip) {
            // ---- first pass: the log-weight volume
            for (int k = -g.A; k <= g.A; ++k) {
                pose_resample<CUBIC, true>(img, th, dx0, dx1, k, g.step, h, w, C, plane, cov);
                __syncthreads();
                for (int it = wave; it < M * G; it += 4) {          // uniform over the wave
                    const int j = it / G, q0 = (it - j * G) * kPoseShifts;
                    const int r = slots[j];
                    if (r < 0) continue;
                    const int count = min(kPoseShifts, nQ - q0);
                    double acc[kPoseShifts];
                    pose_correlate(plane, ref + (long)r * NC, weight, q0, 1, count, nS, g.S, h, w, C, lane, acc);
                    if (lane == 0) {
                        const double half_h = 0.5 * hn[r], lp = log_prior ? log_prior[r] : 0.0;
                        double* vk = vol + ((long)j * nA + (k + g.A)) * nQ + q0;
#pragma unroll
                        for (int t = 0; t < kPoseShifts; ++t)
                            if (t < count) vk[t] = g.inv_sigma2 * (acc[t] - half_h) + lp;
                    }
                }
                __syncthreads();        // the volume's rows of this angle are written, and the plane is free for the next
            }
            // ---- the first maximum of the live volume, and whether every entry is finite
            double bv = -INFINITY;
            int bi = 0x7fffffff, bad = 0;
            for (int i = tid; i < MV; i += 256) {
                if (slots[i / V] < 0) continue;
                const double v = vol[i];
                if (!isfinite(v)) bad = 1;
                if (v > bv) {
                    bv = v;
                    bi = i;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (ov > bv || (ov == bv && oi < bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            if (lane == 0) {
                red[wave] = bv;
                red[4 + wave] = (double)bi;
            }
            bad = __syncthreads_or(bad);
            top_v = red[0];
            top_i = (int)red[4];
            for (int t = 1; t < 4; ++t) {
                const int oi = (int)red[4 + t];
                if (red[t] > top_v || (red[t] == top_v && oi < top_i)) {
                    top_v = red[t];
                    top_i = oi;
                }
            }
            __syncthreads();            // red is free again
            skip = bad != 0;
        }
        if (!skip) {
            // ---- the posterior takes the volume's place
            double part = 0.0;
            for (int i = tid; i < MV; i += 256)
                if (slots[i / V] >= 0) part += exp(vol[i] - top_v);
            Z = pose_block_sum(part, red);
            for (int i = tid; i < MV; i += 256)
                if (slots[i / V] >= 0) vol[i] = exp(vol[i] - top_v) / Z;
            __syncthreads();
            for (int j = wave; j < M; j += 4) {
                double s = 0.0;
                if (slots[j] >= 0) {
                    const double* pj = vol + (long)j * V;
                    for (int i = lane; i < V; i += 64) s += pj[i];
                    s = pose_wave_sum(s);
                }
                if (lane == 0) class_post[(long)b * M + j] = s;
            }
            if (tid == 0) {
                log_evidence[b] = top_v + log(Z);
                const int j = top_i / V, rem = top_i - j * V;
                const int ik = rem / nQ, iy = (rem - ik * nQ) / nS, ix = rem - ik * nQ - iy * nS;
                int* bo = best + 4 * (long)b;
                bo[0] = j;
                bo[1] = ik - g.A;
                bo[2] = ix - g.S;
                bo[3] = iy - g.S;
            }
            // ---- second pass: the contributions, each (slot, pixel) one thread's running sums
            for (int k = -g.A; k <= g.A; ++k) {
                pose_resample<CUBIC, true>(img, th, dx0, dx1, k, g.step, h, w, C, plane, cov);
                __syncthreads();
                for (int t = tid; t < M * N; t += 256) {
                    const int j = t / N, pix = t - j * N;
                    if (slots[j] < 0) continue;
                    const int jy = pix / w, jx = pix - jy * w;
                    const long o = ((long)b * M + j) * N + pix;
                    double acc[SVAE_MAX_OUT], cw = 0.0;
#pragma unroll
                    for (int ch = 0; ch < SVAE_MAX_OUT; ++ch) acc[ch] = (ch < C && k > -g.A) ? contrib[o * C + ch] : 0.0;
                    if (k > -g.A) cw = cover_w[o];
                    const double* pk = vol + ((long)j * nA + (k + g.A)) * nQ;
                    for (int iy = 0; iy < nS; ++iy) {
                        const int yy = jy + iy - g.S;
                        if (yy < 0 || yy >= h) continue;
                        for (int ix = 0; ix < nS; ++ix) {
                            const int xx = jx - (ix - g.S);
                            if (xx < 0 || xx >= w) continue;
                            const double p = pk[iy * nS + ix];
                            if (p == 0.0) continue;
                            const int src = yy * w + xx;
#pragma unroll
                            for (int ch = 0; ch < SVAE_MAX_OUT; ++ch)
                                if (ch < C) acc[ch] += p * plane[(long)src * C + ch];
                            cw += p * cov[src];
                        }
                    }
#pragma unroll
                    for (int ch = 0; ch < SVAE_MAX_OUT; ++ch)
                        if (ch < C) contrib[o * C + ch] = acc[ch];
                    cover_w[o] = cw;
                }
                __syncthreads();        // the plane is free for the next angle
            }
        } else {
            for (int j = tid; j < M; j += 256) class_post[(long)b * M + j] = 0.0;
            if (tid == 0) {
                log_evidence[b] = 0.0;
                int* bo = best + 4 * (long)b;
                bo[0] = -1;
                bo[1] = bo[2] = bo[3] = 0;
            }
        }
        for (int t = tid; t < M * N; t += 256) {                    // the rows of dead slots, and every row of a skipped image
            const int j = t / N;
            if (!skip && slots[j] >= 0) continue;
            const long o = ((long)b * M + j) * N + (t - j * N);
            for (int ch = 0; ch < C; ++ch) contrib[o * C + ch] = 0.0;
            cover_w[o] = 0.0;
        }
        __syncthreads();                // every thread has read the slots before the next image's overwrite them
    }
}

// One thread per (class t, pixel): walks the call's images upwards and within each its slots upwards, adding the rows whose
// reference maps to its class.  Every thread of a wave reads the same candidate (a broadcast), and neighbouring threads
// neighbouring pixels.
__global__ void expect_sums_update_kernel(const double* __restrict__ contrib, const double* __restrict__ cover_w,
                                          const int* __restrict__ cand, const int* __restrict__ target, int B, int M, int N, int C,
                                          int n_ref, int n_classes, double* __restrict__ sum, double* __restrict__ count) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)n_classes * N) return;
    const int k = (int)(t / N);
    const int pix = (int)(t - (long)k * N);
    double acc[SVAE_MAX_OUT];
#pragma unroll
    for (int c = 0; c < SVAE_MAX_OUT; ++c) acc[c] = c < C ? sum[t * C + c] : 0.0;
    double n = count[t];
    for (long bj = 0; bj < (long)B * M; ++bj) {
        const int r = cand[bj];
        if (r < 0 || r >= n_ref) continue;
        if ((target ? target[r] : r) != k) continue;
        const long p = bj * N + pix;
#pragma unroll
        for (int c = 0; c < SVAE_MAX_OUT; ++c)
            if (c < C) acc[c] += contrib[p * C + c];
        n += cover_w[p];
    }
#pragma unroll
    for (int c = 0; c < SVAE_MAX_OUT; ++c)
        if (c < C) sum[t * C + c] = acc[c];
    count[t] = n;
}

}  // namespace svae
