// Per-class eigenimages of aligned images (include/svae_eigen.h): block subspace iteration on the covariance of every class's
// members about their class average, which is never formed.  The arithmetic and the order of every sum are stated in the
// header; tests/eigen_ref.py is the float64 restatement the kernels are held to.  Plain fp64 vector kernels: doubles with
// contraction off, no atomics, no matrix instruction, no scratch.
#pragma once
#include "common.h"

namespace svae {

constexpr int kEigMaxR = 64;
constexpr int kEigMaxK = 4096;
constexpr long kEigMaxBasis = 1L << 28;     // K D R: 2 GiB per basis
constexpr double kEigDead = 0x1p-26;

struct EigGeo {
    int B, N, C, K, R;
    long D;
};

// the header's segments: S = 256 / R' of L indices each
struct EigSegments {
    int Rp, S;
    long L;
    __host__ __device__ EigSegments(long D, int R) : Rp(1) {
        while (Rp < R) Rp *= 2;
        S = 256 / Rp;
        L = (D + S - 1) / S;
    }
};

// the 256 values of a workgroup, one per thread, added in thread order onto +0; every thread gets the total
__device__ __forceinline__ double eig_lane_total(double mine, double* s_part) {
#pragma clang fp contract(off)
    __syncthreads();    // the last total has been read
    s_part[threadIdx.x] = mine;
    __syncthreads();
    double total = 0.0;
    for (int t = 0; t < 256; ++t) total += s_part[t];
    return total;
}

// One workgroup per image: thread (s, r) = (tid / R', tid % R') forms segment s of column r, thread (0, r) adds the segments.
__global__ __launch_bounds__(256) void eig_project_kernel(const float* __restrict__ aligned, const uint8_t* __restrict__ cover,
                                                          const int* __restrict__ label, const double* __restrict__ mean,
                                                          const double* __restrict__ Q, EigGeo g, double* __restrict__ T) {
#pragma clang fp contract(off)
    __shared__ double s_part[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int k = label[b];
    if (k < 0 || k >= g.K) {    // the same decision in every thread
        if (tid < g.R) T[(long)b * g.R + tid] = 0.0;
        return;
    }
    const EigSegments seg(g.D, g.R);
    const int s = tid / seg.Rp, r = tid - s * seg.Rp;
    double acc = 0.0;
    if (r < g.R) {
        const long lo = s * seg.L, hi = lo + seg.L < g.D ? lo + seg.L : g.D;
        const float* a = aligned + (long)b * g.D;
        const uint8_t* cv = cover ? cover + (long)b * g.N : nullptr;
        const double* mu = mean + (long)k * g.D;
        const double* q = Q + (long)k * g.D * g.R + r;
        for (long e = lo; e < hi; ++e) {
            if (cv && cv[e / g.C] == 0) continue;
            const double d = (double)a[e] - mu[e];
            acc += d * q[e * g.R];
        }
    }
    s_part[tid] = acc;
    __syncthreads();
    if (tid < g.R) {
        double total = 0.0;
        for (int i = 0; i < seg.S; ++i) total += s_part[i * seg.Rp + tid];
        T[(long)b * g.R + tid] = total;
    }
}

// One thread per (class, index, column), the column fastest, walking the labels of the call in index order.
__global__ __launch_bounds__(256) void eig_accumulate_kernel(const float* __restrict__ aligned, const uint8_t* __restrict__ cover,
                                                             const int* __restrict__ label, const double* __restrict__ mean,
                                                             const double* __restrict__ T, EigGeo g, double* __restrict__ Y,
                                                             double* __restrict__ ssq) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)g.K * g.D * g.R) return;
    const long ke = t / g.R;            // k D + e
    const int r = (int)(t - ke * g.R);
    const int k = (int)(ke / g.D);
    const long e = ke - (long)k * g.D;
    const long j = e / g.C;
    const double mu = mean[ke];
    const bool squares = ssq && r == 0;
    double y = Y[t];
    double q = squares ? ssq[ke] : 0.0;
    for (int b = 0; b < g.B; ++b) {
        if (label[b] != k) continue;
        if (cover && cover[(long)b * g.N + j] == 0) continue;
        const double d = (double)aligned[(long)b * g.D + e] - mu;
        y += d * T[(long)b * g.R + r];
        if (squares) q += d * d;
    }
    Y[t] = y;
    if (squares) ssq[ke] = q;
}

// One workgroup per class; lane t owns the indices t, t + 256, ... of every column, so only the totals cross threads.
__global__ __launch_bounds__(256) void eig_orthonormalise_kernel(const double* __restrict__ Y, long D, int R, double* __restrict__ Q) {
#pragma clang fp contract(off)
    __shared__ double s_part[256];
    __shared__ int s_live[kEigMaxR];
    const int tid = threadIdx.x;
    const double* y = Y + (long)blockIdx.x * D * R;
    double* q = Q + (long)blockIdx.x * D * R;
    for (int j = 0; j < R; ++j) {
        double p = 0.0;
        for (long e = tid; e < D; e += 256) {
            const double v = y[e * R + j];
            q[e * R + j] = v;
            p += v * v;
        }
        const double before = sqrt(eig_lane_total(p, s_part));
        for (int round = 0; round < 2; ++round)
            for (int i = 0; i < j; ++i) {
                if (!s_live[i]) continue;       // written before the barriers of column i's last total
                p = 0.0;
                for (long e = tid; e < D; e += 256) p += q[e * R + i] * q[e * R + j];
                const double c = eig_lane_total(p, s_part);
                for (long e = tid; e < D; e += 256) q[e * R + j] = q[e * R + j] - c * q[e * R + i];
            }
        p = 0.0;
        for (long e = tid; e < D; e += 256) p += q[e * R + j] * q[e * R + j];
        const double after = sqrt(eig_lane_total(p, s_part));
        const bool dead = !(after > 0.0) || !isfinite(after) || after < kEigDead * before;
        if (tid == 0) s_live[j] = !dead;
        for (long e = tid; e < D; e += 256) q[e * R + j] = dead ? 0.0 : q[e * R + j] / after;
        __syncthreads();    // s_live[j] is there for the columns to come
    }
}

// One workgroup per (class, row r): thread (s, c) forms segment s of A[r, c] and of A[c, r], thread (0, c) adds the segments.
__global__ __launch_bounds__(256) void eig_gram_kernel(const double* __restrict__ Q, const double* __restrict__ Y,
                                                       const long long* __restrict__ members, long D, int R, double* __restrict__ G) {
#pragma clang fp contract(off)
    __shared__ double s_a[256], s_b[256];
    const int k = blockIdx.x / R, r = blockIdx.x - k * R, tid = threadIdx.x;
    const long long n = members[k];
    double* out = G + ((long)k * R + r) * R;
    if (n < 2) {
        if (tid < R) out[tid] = 0.0;
        return;
    }
    const EigSegments seg(D, R);
    const int s = tid / seg.Rp, c = tid - s * seg.Rp;
    double a = 0.0, b = 0.0;
    if (c < R) {
        const long lo = s * seg.L, hi = lo + seg.L < D ? lo + seg.L : D;
        const double* q = Q + (long)k * D * R;
        const double* y = Y + (long)k * D * R;
        for (long e = lo; e < hi; ++e) {
            a += q[e * R + r] * y[e * R + c];
            b += q[e * R + c] * y[e * R + r];
        }
    }
    s_a[tid] = a;
    s_b[tid] = b;
    __syncthreads();
    if (tid < R) {
        double ta = 0.0, tb = 0.0;
        for (int i = 0; i < seg.S; ++i) ta += s_a[i * seg.Rp + tid];
        for (int i = 0; i < seg.S; ++i) tb += s_b[i * seg.Rp + tid];
        out[tid] = ((ta + tb) * 0.5) / (double)(n - 1);
    }
}

// One workgroup per (class, p < P); lane t owns the indices t, t + 256, ...: it writes v unsigned, the workgroup finds the
// sign, and each lane signs its own entries and forms its part of the residual.
__global__ __launch_bounds__(256) void eig_rotate_kernel(const double* __restrict__ Q, const double* __restrict__ Y,
                                                         const double* __restrict__ W, const double* __restrict__ lambda,
                                                         const long long* __restrict__ members, long D, int R, int P,
                                                         double* __restrict__ eigenimages, double* __restrict__ residual,
                                                         double* __restrict__ rot) {
#pragma clang fp contract(off)
    __shared__ double s_part[256];
    __shared__ double s_big[256], s_val[256];
    __shared__ long s_at[256];
    __shared__ double s_w[kEigMaxR];
    const int k = blockIdx.x / P, p = blockIdx.x - k * P, tid = threadIdx.x;
    const long long n = members[k];
    double* img = eigenimages + ((long)k * P + p) * D;
    if (n < 2) {
        for (long e = tid; e < D; e += 256) img[e] = 0.0;
        if (tid < R) rot[((long)k * P + p) * R + tid] = 0.0;
        if (tid == 0) residual[(long)k * P + p] = 0.0;
        return;
    }
    if (tid < R) s_w[tid] = W[((long)k * R + p) * R + tid];
    __syncthreads();
    const double* q = Q + (long)k * D * R;
    const double* y = Y + (long)k * D * R;
    double big = -1.0, val = 0.0;
    long at = D;
    for (long e = tid; e < D; e += 256) {
        double v = 0.0;
        for (int r = 0; r < R; ++r) v += q[e * R + r] * s_w[r];
        img[e] = v;
        if (fabs(v) > big) {    // a NaN is never the largest
            big = fabs(v);
            val = v;
            at = e;
        }
    }
    s_big[tid] = big;
    s_val[tid] = val;
    s_at[tid] = at;
    __syncthreads();
    big = -1.0, val = 0.0, at = D;
    for (int t = 0; t < 256; ++t)
        if (s_big[t] > big || (s_big[t] == big && s_at[t] < at)) {
            big = s_big[t];
            val = s_val[t];
            at = s_at[t];
        }
    const bool flip = val < 0.0;
    const double lam = lambda[(long)k * R + p];
    const double scale = (double)(n - 1);
    double part = 0.0;
    for (long e = tid; e < D; e += 256) {
        double u = 0.0;
        for (int r = 0; r < R; ++r) u += y[e * R + r] * s_w[r];
        u = u / scale;
        const double v = flip ? -img[e] : img[e];
        img[e] = v;
        const double w = (flip ? -u : u) - lam * v;
        part += w * w;
    }
    const double total = eig_lane_total(part, s_part);
    if (tid == 0) residual[(long)k * P + p] = sqrt(total);
    if (tid < R) rot[((long)k * P + p) * R + tid] = flip ? -s_w[tid] : s_w[tid];
}

// One thread per (image, component).
__global__ __launch_bounds__(256) void eig_coords_kernel(const double* __restrict__ T, const int* __restrict__ label,
                                                         const double* __restrict__ rot, int B, int K, int R, int P,
                                                         double* __restrict__ coords) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)B * P) return;
    const int b = (int)(t / P), p = (int)(t - (long)b * P);
    const int k = label[b];
    double acc = 0.0;
    if (k >= 0 && k < K) {
        const double* w = rot + ((long)k * P + p) * R;
        for (int r = 0; r < R; ++r) acc += T[(long)b * R + r] * w[r];
    }
    coords[t] = acc;
}

}  // namespace svae
