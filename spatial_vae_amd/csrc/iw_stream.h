// Streaming K-sample importance-weighted scorer (include/svae_stream.h): the log-mean-exp, effective sample size, weighted
// pose / latent means and best sample of each image, merged chunk by chunk so that K is unbounded and only one chunk of
// samples is resident.  Row b*K + k is sample k of image b, as in the iw_* kernels of elementwise.h, whose group helpers are
// reused.  Arithmetic is in doubles and rounded once on the way out; sums are taken in an order that depends on the chunk
// sizes only (no atomics), so two runs with the same chunking are bit-equal.
#pragma once
#include "elementwise.h"

namespace svae {

// Per-image record, in doubles: kIwsHeader scalars, inf_dim + 1 weighted sums, inf_dim best-sample coordinates.
//   [0] M   running max of a = loglik + log_ratio (-inf until a finite a is seen)
//   [1] s   sum exp(a - M)          [2] s2  sum exp(2 (a - M))
//   [3] sum loglik                  [4] sum log_ratio          [5] n samples seen
//   [6] best a                      [7] unused
//   weighted sums: slot 0 = sum e cos(theta), slot 1 = sum e sin(theta) (rotation), slot j + 1 = sum e v_j for every other
//   latent coordinate j, e = exp(a - M); then the best sample's coordinates in latent order.
constexpr int kIwsHeader = 8;
__host__ __device__ inline long iws_stride(int inf) { return kIwsHeader + 2L * inf + 1; }
constexpr int kIwsPerLane = SVAE_IW_MAX_SAMPLES / 64;               // samples one lane of a 64-wide group holds at the largest K

__global__ void iw_stream_reset_kernel(double* __restrict__ state, int B, int inf) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long stride = iws_stride(inf);
    if (i >= (long)B * stride) return;
    const int f = (int)(i % stride);
    state[i] = (f == 0 || f == 6) ? -INFINITY : 0.0;
}

// coordinate j of sample `row` in the units the decoder received (the outputs of latent_iw_fwd_kernel)
__device__ __forceinline__ double iws_coord(const float* __restrict__ theta, const float* __restrict__ dx,
                                            const float* __restrict__ zc, long row, int j, int off, int c0, int zd) {
    if (j < off) return theta[row];
    if (j < c0) return dx[2 * row + (j - off)];
    return zc[row * zd + (j - c0)];
}

// A group of G = iw_group_width(K) lanes per image, 256 / G images per block.  The chunk's exp(a - M_new) stay in registers
// (at most kIwsPerLane per lane) while the coordinates are summed one after the other; the old sums are rescaled by
// exp(M_old - M_new) (its square for s2), the chunk's own are formed against M_new directly.
__global__ void iw_stream_update_kernel(double* __restrict__ state, const float* __restrict__ loglik,
                                        const float* __restrict__ log_ratio, const float* __restrict__ theta,
                                        const float* __restrict__ dx, const float* __restrict__ zc, int K, LatentGeo g) {
    const int G = iw_group_width(K), groups = 256 / G;
    const int grp = threadIdx.x / G, lane = threadIdx.x & (G - 1);
    const long b = (long)blockIdx.x * groups + grp;
    const bool live = b < g.B;                                        // whole groups are live or not: every lane shuffles
    const int off = g.rotate ? 1 : 0, c0 = off + (g.translate ? 2 : 0), zd = g.inf - c0;
    double* st = state + (live ? b : 0) * iws_stride(g.inf);
    const float* ll = loglik + (live ? b : 0) * K;
    const float* lr = log_ratio + (live ? b : 0) * K;
    // the record as it stood, read by every lane before any lane writes
    const double M_old = st[0], n_old = st[5], best_old = st[6];

    double m = -INFINITY, sp = 0.0, sr = 0.0, la = -INFINITY;
    int li = 0x7fffffff;                                             // this lane's first sample at its largest a
    if (live)
        for (int k = lane; k < K; k += G) {
            const double a = (double)ll[k] + (double)lr[k];
            m = fmax(m, a);
            sp += ll[k];
            sr += lr[k];
            if (li == 0x7fffffff || a > la) {
                la = a;
                li = k;
            }
        }
    m = iw_group_max(m, G);
    sp = iw_group_sum(sp, G);
    sr = iw_group_sum(sr, G);
    // lowest index among the samples that reach the chunk's max (sample 0 when every a is -inf)
    int kbest = (int)-iw_group_max((li != 0x7fffffff && la == m) ? -(double)li : -(double)0x7fffffff, G);
    if (kbest >= K) kbest = 0;                                       // no lane matched (a NaN among the a): any row of this image

    const double M_new = fmax(M_old, m);
    const double ref = M_new > -INFINITY ? M_new : 0.0;              // all -inf so far: every exp below is 0
    const double f = (M_old == M_new) ? 1.0 : (M_old > -INFINITY ? exp(M_old - M_new) : 0.0);

    double e[kIwsPerLane];
    double s = 0.0, s2 = 0.0;
#pragma unroll
    for (int i = 0; i < kIwsPerLane; ++i) {
        const int k = lane + i * G;
        e[i] = (live && k < K) ? exp((double)ll[k] + (double)lr[k] - ref) : 0.0;
        s += e[i];
        s2 += e[i] * e[i];
    }
    s = iw_group_sum(s, G);
    s2 = iw_group_sum(s2, G);

    for (int j = 0; j < g.inf; ++j) {
        double wc = 0.0, ws = 0.0;                                    // rotation: cos and sin sums; else wc alone
#pragma unroll
        for (int i = 0; i < kIwsPerLane; ++i) {
            const int k = lane + i * G;
            if (live && k < K) {
                const double v = iws_coord(theta, dx, zc, b * K + k, j, off, c0, zd);
                if (j < off) {
                    wc += e[i] * cos(v);
                    ws += e[i] * sin(v);
                } else {
                    wc += e[i] * v;
                }
            }
        }
        wc = iw_group_sum(wc, G);
        if (j < off) ws = iw_group_sum(ws, G);
        if (live && lane == 0) {
            double* w = st + kIwsHeader;
            if (j < off) {
                w[0] = w[0] * f + wc;
                w[1] = w[1] * f + ws;
            } else {
                w[j + 1] = w[j + 1] * f + wc;
            }
        }
    }
    if (!live) return;
    // the best sample: replaced on a strictly larger a only; the first chunk always sets it
    if (n_old == 0.0 || m > best_old) {
        double* best = st + kIwsHeader + g.inf + 1;
        for (int j = lane; j < g.inf; j += G) best[j] = iws_coord(theta, dx, zc, b * K + kbest, j, off, c0, zd);
        if (lane == 0) st[6] = m;
    }
    if (lane == 0) {
        st[0] = M_new;
        st[1] = st[1] * f + s;
        st[2] = st[2] * f * f + s2;
        st[3] += sp;
        st[4] += sr;
        st[5] = n_old + (double)K;
    }
}

// one thread per image: the per_image row (6 + 2 inf_dim floats), each value one double rounded once
__global__ void iw_stream_finish_kernel(const double* __restrict__ state, float* __restrict__ per_image, int B, int inf,
                                        int rotate) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const double* st = state + b * iws_stride(inf);
    const double* w = st + kIwsHeader;
    const double* best = w + inf + 1;
    float* row = per_image + b * (6 + 2L * inf);
    const double M = st[0] > -INFINITY ? st[0] : 0.0, s = st[1], s2 = st[2], n = st[5];
    row[0] = (float)(M + log(s) - log(n));
    row[1] = (float)(st[3] / n);
    row[2] = (float)(-st[4] / n);
    row[3] = (float)(s == 0.0 ? 0.0 : s * s / s2);                    // s == 0: every a was -inf; a NaN s stays NaN
    row[4] = (float)st[6];
    row[5] = (float)(!rotate ? 1.0 : (s == 0.0 ? 0.0 : sqrt(w[0] * w[0] + w[1] * w[1]) / s));
    for (int j = 0; j < inf; ++j) {
        double v;
        if (j == 0 && rotate) v = (s == 0.0) ? 0.0 : atan2(w[1], w[0]);
        else v = (s == 0.0) ? 0.0 : w[j + 1] / s;
        row[6 + j] = (float)v;
        row[6 + inf + j] = (float)best[j];
    }
}

// One block: {mean_b L_b, sum loglik / sum n, -sum log_ratio / sum n} in the fixed order of iw_head_fwd_kernel's tail.
__global__ void iw_stream_means_kernel(const double* __restrict__ state, float* __restrict__ out, int B, int inf) {
    __shared__ double red[4][4];
    const long stride = iws_stride(inf);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < B; b += 256) {
        const double* st = state + b * stride;
        const double M = st[0] > -INFINITY ? st[0] : 0.0;
        acc[0] += M + log(st[1]) - log(st[5]);
        acc[1] += st[3];
        acc[2] += st[4];
        acc[3] += st[5];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[i] = iw_group_sum(acc[i], 64);
        if ((threadIdx.x & 63) == 0) red[i][threadIdx.x >> 6] = acc[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = red[3][0] + red[3][1] + red[3][2] + red[3][3];
        out[0] = (float)((red[0][0] + red[0][1] + red[0][2] + red[0][3]) / (double)B);
        out[1] = (float)((red[1][0] + red[1][1] + red[1][2] + red[1][3]) / n);
        out[2] = (float)(-(red[2][0] + red[2][1] + red[2][2] + red[2][3]) / n);
    }
}

}  // namespace svae
