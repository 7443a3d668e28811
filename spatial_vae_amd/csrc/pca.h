// Principal axes of (N, D) float points, globally or per group (include/svae_pca.h), a sibling of cluster.h and gmm.h built from
// the same latent_core.h: its chunk rule and its two-level order of every sum over points; the covariances are then diagonalised by
// cyclic Jacobi, one workgroup per matrix with A and V in LDS.  The arithmetic and its order are stated in the header;
// tests/pca_ref.py is the float64 restatement the kernels are held to.  Doubles with contraction off, no atomics, no scratch.
#pragma once
#include "cluster.h"

namespace svae {

constexpr int kPcaMaxG = 1024;
constexpr int kPcaMaxPartials = 32768;      // G D (D + 1) / 2: bounds the per-chunk products to 256 MiB
constexpr int kPcaMaxSweeps = 30;
constexpr int kPcaLd = kKmeansMaxD + 1;     // row stride of A and V in LDS: odd, so a column walk spreads over the banks
constexpr double kPcaStop = 0x1p-104;

__host__ __device__ inline bool pca_sizes_ok(long long N, int D, int G) {
    return D >= 1 && D <= kKmeansMaxD && G >= 1 && G <= kPcaMaxG && (long)G * (D * (D + 1) / 2) <= kPcaMaxPartials && N >= 1 &&
           N <= 0x7fffffffLL;
}

// where the pieces of the workspace start, in 8-byte words
struct PcaWs {
    long long* count;    // (chunks, G) members per chunk
    double* sum;         // (chunks, G, D) coordinate sums per chunk
    double* prod;        // (chunks, G, D (D + 1) / 2) centred products per chunk, (t, u <= t) at t (t + 1) / 2 + u
    int* member;         // (N) the group each point counts in, -1 = none
};

__host__ __device__ inline size_t pca_ws_words(long N, int D, int G) {
    const size_t C = LatentChunks(N).n;
    return C * G * (1 + D + D * (D + 1) / 2) + ((size_t)N + 1) / 2;
}

inline PcaWs pca_ws(void* ws, long N, int D, int G) {
    const size_t C = LatentChunks(N).n;
    PcaWs w;
    w.count = static_cast<long long*>(ws);
    w.sum = reinterpret_cast<double*>(w.count + C * G);
    w.prod = w.sum + C * G * D;
    w.member = reinterpret_cast<int*>(w.prod + C * G * (D * (D + 1) / 2));
    return w;
}

// the group point i counts in: its entry of `group` (0 without one) where that lies in [0, G) and every coordinate is finite
__device__ __forceinline__ int pca_member(const float* __restrict__ x, long i, int D, int G, const int* __restrict__ group) {
    const int g = group ? group[i] : 0;
    if (g < 0 || g >= G) return -1;
    return point_finite(x, i, D) ? g : -1;
}

// entry e of a lower triangle stored row by row: (t, u <= t) with e = t (t + 1) / 2 + u
struct PcaTri {
    int t, u;
    __device__ __forceinline__ explicit PcaTri(int e) : t(0) {
        while ((t + 1) * (t + 2) / 2 <= e) ++t;
        u = e - t * (t + 1) / 2;
    }
};

// Pass 1: one workgroup per chunk.  A thread per point first writes the chunk's entries of w.member; then a thread per
// (group, t) pair with t in 0..D walks the chunk's points in index order: the coordinate sum for t < D, the member count for
// t == D.
__global__ __launch_bounds__(256) void pca_sums_kernel(const float* __restrict__ x, long N, int D, int G, long P,
                                                       const int* __restrict__ group, PcaWs w) {
#pragma clang fp contract(off)
    const ChunkSpan span(blockIdx.x, P, N);
    for (long i = span.lo + threadIdx.x; i < span.hi; i += 256) w.member[i] = pca_member(x, i, D, G, group);
    __syncthreads();
    const int* member = w.member;
    for (int p = threadIdx.x; p < G * (D + 1); p += 256) {
        const int g = p / (D + 1), t = p - g * (D + 1);
        if (t == D) {
            long long n = 0;
            for (long i = span.lo; i < span.hi; ++i) n += member[i] == g;
            w.count[(long)blockIdx.x * G + g] = n;
        } else {
            double s = 0.0;
            for (long i = span.lo; i < span.hi; ++i)
                if (member[i] == g) s += (double)x[i * D + t];
            w.sum[((long)blockIdx.x * G + g) * D + t] = s;
        }
    }
}

// The chunks of pass 1 added in index order: thread (g, t) writes mean[g, t], thread (g, D) count[g].
__global__ __launch_bounds__(256) void pca_mean_kernel(int D, int G, int chunks, long long* __restrict__ count, double* __restrict__ mean,
                                                       PcaWs w) {
#pragma clang fp contract(off)
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)G * (D + 1)) return;
    const int g = (int)(p / (D + 1)), t = (int)(p - (long)g * (D + 1));
    const long long n = chunk_total(w.count, chunks, G, g);
    if (t == D) {
        count[g] = n;
        return;
    }
    mean[(long)g * D + t] = n > 0 ? chunk_total(w.sum, chunks, (long)G * D, (long)g * D + t) / (double)n : 0.0;
}

// Pass 2: one workgroup per chunk, a thread per (group, t, u <= t) walking the chunk's points in index order.
__global__ __launch_bounds__(256) void pca_products_kernel(const float* __restrict__ x, long N, int D, int G, long P,
                                                           const double* __restrict__ mean, PcaWs w) {
#pragma clang fp contract(off)
    const ChunkSpan span(blockIdx.x, P, N);
    const int T = D * (D + 1) / 2;
    const int* __restrict__ member = w.member;
    for (int p = threadIdx.x; p < G * T; p += 256) {
        const int g = p / T, e = p - g * T;
        const PcaTri tri(e);
        const int t = tri.t, u = tri.u;
        const double mt = mean[(long)g * D + t], mu = mean[(long)g * D + u];
        double m = 0.0;
        for (long i = span.lo; i < span.hi; ++i)
            if (member[i] == g) {
                const double dt = (double)x[i * D + t] - mt;
                const double du = (double)x[i * D + u] - mu;
                m += dt * du;
            }
        w.prod[((long)blockIdx.x * G + g) * T + e] = m;
    }
}

// The chunks of pass 2 added in index order: thread (g, t, u <= t) writes cov[g, t, u] and cov[g, u, t].
__global__ __launch_bounds__(256) void pca_cov_kernel(int D, int G, int chunks, const long long* __restrict__ count, double* __restrict__ cov,
                                                      PcaWs w) {
#pragma clang fp contract(off)
    const int T = D * (D + 1) / 2;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= (long)G * T) return;
    const int g = (int)(p / T), e = (int)(p - (long)g * T);
    const PcaTri tri(e);
    const int t = tri.t, u = tri.u;
    const long long n = count[g];
    const double v = n >= 2 ? chunk_total(w.prod, chunks, (long)G * T, p) / (double)(n - 1) : 0.0;
    cov[((long)g * D + t) * D + u] = v;
    cov[((long)g * D + u) * D + t] = v;
}

// the player in seat k at step s of the round-robin of n players (the header's rule)
__device__ __forceinline__ int pca_seat(int k, int s, int n) { return k == 0 ? 0 : 1 + (k - 1 + (n - 1) - s) % (n - 1); }

// Cyclic Jacobi: one workgroup per matrix.  Thread r < D forms row r's part of the norms, thread 0 their total and the decision
// (shared through s_go); thread k < n / 2 forms pair k's rotation; the three update phases spread (pair, j) over all threads.
__global__ __launch_bounds__(256) void pca_eigen_kernel(const double* __restrict__ cov, int D, double* __restrict__ eigenvalues,
                                                        double* __restrict__ components, int* __restrict__ sweeps,
                                                        double* __restrict__ off_norm) {
#pragma clang fp contract(off)
    __shared__ double A[kKmeansMaxD * kPcaLd];
    __shared__ double V[kKmeansMaxD * kPcaLd];
    __shared__ double srow[kKmeansMaxD];
    __shared__ double sc[kKmeansMaxD / 2], ss[kKmeansMaxD / 2];
    __shared__ int sp[kKmeansMaxD / 2], sq[kKmeansMaxD / 2];
    __shared__ int srank[kKmeansMaxD];
    __shared__ double ssign[kKmeansMaxD];
    __shared__ double s_fro2, s_off2;
    __shared__ int s_go;
    const int tid = threadIdx.x;
    const long g = blockIdx.x;
    const double* in = cov + g * D * D;
    double* val = eigenvalues + g * D;
    double* comp = components + g * D * D;
    for (int e = tid; e < D * D; e += 256) {
        const int r = e / D, q = e - r * D;
        A[r * kPcaLd + q] = in[e];
        V[r * kPcaLd + q] = r == q ? 1.0 : 0.0;
    }
    __syncthreads();
    if (tid < D) {
        double f = 0.0;
        for (int q = 0; q < D; ++q) f += A[tid * kPcaLd + q] * A[tid * kPcaLd + q];
        srow[tid] = f;
    }
    __syncthreads();
    if (tid == 0) {
        double f = 0.0;
        for (int r = 0; r < D; ++r) f += srow[r];
        s_fro2 = f;
    }
    __syncthreads();
    const double fro2 = s_fro2;
    if (!isfinite(fro2)) {      // skipped: the same decision in every thread
        for (int e = tid; e < D * D; e += 256) comp[e] = 0.0;
        if (tid < D) val[tid] = 0.0;
        if (tid == 0) {
            sweeps[g] = -1;
            off_norm[g] = 0.0;
        }
        return;
    }
    const int n = D + (D & 1), half = n / 2;
    int done = 0;
    for (;;) {
        if (tid < D) {
            double f = 0.0;
            for (int q = 0; q < D; ++q)
                if (q != tid) f += A[tid * kPcaLd + q] * A[tid * kPcaLd + q];
            srow[tid] = f;
        }
        __syncthreads();
        if (tid == 0) {
            double f = 0.0;
            for (int r = 0; r < D; ++r) f += srow[r];
            s_off2 = f;
            s_go = !(f <= kPcaStop * fro2) && done < kPcaMaxSweeps;
        }
        __syncthreads();
        if (!s_go) break;
        for (int s = 0; s < n - 1; ++s) {
            if (tid < half) {
                const int a = pca_seat(tid, s, n), b = pca_seat(n - 1 - tid, s, n);
                const int p = a < b ? a : b, q = a < b ? b : a;
                double c = 1.0, sn = 0.0;
                if (q < D) {
                    const double apq = A[p * kPcaLd + q];
                    if (apq != 0.0) {
                        const double theta = (A[q * kPcaLd + q] - A[p * kPcaLd + p]) / (2.0 * apq);
                        const double root = sqrt(theta * theta + 1.0);
                        const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + root);
                        c = 1.0 / sqrt(t * t + 1.0);
                        sn = t * c;
                    }
                }
                sp[tid] = q < D ? p : -1;       // -1: the bye
                sq[tid] = q;
                sc[tid] = c;
                ss[tid] = sn;
            }
            __syncthreads();
            for (int e = tid; e < half * D; e += 256) {         // rows: A <- J^T A
                const int k = e / D, j = e - k * D;
                const int p = sp[k], q = sq[k];
                if (p < 0) continue;
                const double c = sc[k], sn = ss[k];
                const double ap = A[p * kPcaLd + j], aq = A[q * kPcaLd + j];
                A[p * kPcaLd + j] = c * ap - sn * aq;
                A[q * kPcaLd + j] = sn * ap + c * aq;
            }
            __syncthreads();
            for (int e = tid; e < half * D; e += 256) {         // columns: A <- A J, V <- V J
                const int k = e / D, j = e - k * D;
                const int p = sp[k], q = sq[k];
                if (p < 0) continue;
                const double c = sc[k], sn = ss[k];
                const double ap = A[j * kPcaLd + p], aq = A[j * kPcaLd + q];
                A[j * kPcaLd + p] = c * ap - sn * aq;
                A[j * kPcaLd + q] = sn * ap + c * aq;
                const double vp = V[j * kPcaLd + p], vq = V[j * kPcaLd + q];
                V[j * kPcaLd + p] = c * vp - sn * vq;
                V[j * kPcaLd + q] = sn * vp + c * vq;
            }
            __syncthreads();
            if (tid < half && sp[tid] >= 0) {
                A[sp[tid] * kPcaLd + sq[tid]] = 0.0;
                A[sq[tid] * kPcaLd + sp[tid]] = 0.0;
            }
            __syncthreads();
        }
        ++done;
    }
    // the rank of column j: how many columns come before it (a larger value, or an equal one of lower index), and its sign
    if (tid < D) {
        const double mine = A[tid * kPcaLd + tid];
        int rank = 0;
        for (int i = 0; i < D; ++i) {
            const double other = A[i * kPcaLd + i];
            rank += other > mine || (other == mine && i < tid);
        }
        double big = -1.0, at = 0.0;
        for (int r = 0; r < D; ++r) {
            const double v = V[r * kPcaLd + tid];
            if (fabs(v) > big) {
                big = fabs(v);
                at = v;
            }
        }
        srank[tid] = rank;
        ssign[tid] = at < 0.0 ? -1.0 : 1.0;
        val[rank] = mine;
    }
    __syncthreads();
    for (int e = tid; e < D * D; e += 256) {
        const int j = e / D, r = e - j * D;
        const double v = V[r * kPcaLd + j];
        comp[srank[j] * D + r] = ssign[j] < 0.0 ? -v : v;
    }
    if (tid == 0) {
        sweeps[g] = done;
        off_norm[g] = sqrt(s_off2);
    }
}

// One thread per (point, component).
__global__ __launch_bounds__(256) void pca_project_kernel(const float* __restrict__ x, long N, int D, int G, int P,
                                                          const int* __restrict__ group, const long long* __restrict__ count,
                                                          const double* __restrict__ mean, const double* __restrict__ components,
                                                          double* __restrict__ proj) {
#pragma clang fp contract(off)
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= N * P) return;
    const long i = e / P;
    const int p = (int)(e - i * P);
    const int g = pca_member(x, i, D, G, group);
    double acc = 0.0;
    if (g >= 0 && count[g] >= 2) {
        const double* mu = mean + (long)g * D;
        const double* axis = components + ((long)g * D + p) * D;
        for (int t = 0; t < D; ++t) {
            const double d = (double)x[i * D + t] - mu[t];
            acc += d * axis[t];
        }
    }
    proj[e] = acc;
}

}  // namespace svae
