// Diagonal-covariance Gaussian mixture over (N, D) float points by EM (include/svae_gmm.h), a sibling of cluster.h built from
// the same latent_core.h: its chunk rule, its two-level order of every sum over points, a point's coordinates in registers and
// the component parameters in LDS.  The arithmetic and its order are stated in the header; tests/gmm_ref.py is the float64
// restatement the kernels are held to.  Doubles with contraction off, no atomics, no scratch.
#pragma once
#include "cluster.h"

namespace svae {

constexpr double kGmmLog2Pi = 1.8378770664093453;   // log(2 pi) rounded to double

// where the pieces of the workspace start, in 8-byte words
struct GmmWs {
    double* ll;          // (chunks) per-chunk sums of ll_i
    long long* assigned; // (chunks)
    double* part;        // (chunks, k, 2D + 1) per chunk and component: S1 (D), S2 (D), R
    double* iv;          // (k, D) 1 / var
    double* c;           // (k) the log-normaliser, -inf for a dead component
    long long* snap;     // (4) the record as the step found it: converged_at, iterations, bits of previous, unused
};

__host__ __device__ inline size_t gmm_ws_words(long N, int D, int k) {
    const size_t C = LatentChunks(N).n;
    return C * (2 + (size_t)k * (2 * D + 1)) + (size_t)k * (D + 1) + 4;
}

inline GmmWs gmm_ws(void* ws, long N, int D, int k) {
    const size_t C = LatentChunks(N).n;
    GmmWs w;
    w.ll = static_cast<double*>(ws);
    w.assigned = reinterpret_cast<long long*>(w.ll + C);
    w.part = reinterpret_cast<double*>(w.assigned + C);
    w.iv = w.part + C * k * (2 * D + 1);
    w.c = w.iv + (size_t)k * D;
    w.snap = reinterpret_cast<long long*>(w.c + k);
    return w;
}

// Prologue: a thread per component writes iv and c; thread 0 keeps the record's three deciding words aside, so that the tail's
// workgroups all decide on what the step found while workgroup 0 writes the record.
__global__ __launch_bounds__(256) void gmm_prologue_kernel(int D, int k, const double* __restrict__ weight, const double* __restrict__ var,
                                                           const svae_gmm_record* __restrict__ rec, GmmWs w) {
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) {
        w.snap[0] = rec->converged_at;
        w.snap[1] = rec->iterations;
        w.snap[2] = __double_as_longlong(rec->previous);
        w.snap[3] = 0;
    }
    if (j >= k) return;
    const double wj = weight[j];
    if (!(wj > 0.0)) {
        for (int t = 0; t < D; ++t) w.iv[(long)j * D + t] = 0.0;
        w.c[j] = -INFINITY;
        return;
    }
    double lv = 0.0;
    for (int t = 0; t < D; ++t) {
        const double v = var[(long)j * D + t];
        w.iv[(long)j * D + t] = 1.0 / v;
        lv += log(v);
    }
    const double dl = (double)D * kGmmLog2Pi;
    w.c[j] = log(wj) - 0.5 * (lv + dl);
}

// a[i, j] of the header against one staged component: mean (D), iv (D), c (every lane reads the same LDS address, a broadcast)
template <int DMAX>
__device__ __forceinline__ double gmm_score(const float (&xr)[DMAX], const double* comp, int D) {
#pragma clang fp contract(off)
    const double c = comp[2 * D];
    if (c == -INFINITY) return c;
    double q = 0.0;
#pragma unroll
    for (int t = 0; t < DMAX; ++t)
        if (t < D) {
            const double d = (double)xr[t] - comp[t];
            q += (d * d) * comp[D + t];
        }
    return c - 0.5 * q;
}

// E part: one workgroup per chunk, 256 points per round, one thread per point.  The scores a[i, :] are staged in the point's
// row of resp while the slabs are walked, then read back twice: for s_i, and for the responsibilities written over them.  Per
// chunk the in-order sum of ll_i and the assigned count (RoundFold).
template <int DMAX>
__global__ __launch_bounds__(256) void gmm_e_kernel(const float* __restrict__ x, long N, int D, int k, long P,
                                                    const double* __restrict__ mean, double* __restrict__ resp, int* __restrict__ label,
                                                    double* __restrict__ loglik_point, GmmWs w) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const ChunkSpan span(blockIdx.x, P, N);
    RoundFold fold;     // sum: ll; bit 0: assigned
    for (long r0 = span.lo; r0 < span.hi; r0 += 256) {
        const long i = r0 + tid;
        const bool live = i < span.hi;
        float xr[DMAX];
        const bool finite = point_load<DMAX>(x, i, live, D, xr);
        double* row = resp + (live ? i : 0) * (long)k;
        double m = -INFINITY;
        int bj = 0;
        slab_walk(      // a staged component: mean (D), iv (D), c
            k, 2 * D + 1, finite,
            [&](int j, int u) { return u < D ? mean[(long)j * D + u] : u < 2 * D ? w.iv[(long)j * D + (u - D)] : w.c[j]; },
            [&](int j, const double* comp) {
                const double a = gmm_score<DMAX>(xr, comp, D);
                row[j] = a;
                if (a > m) {
                    m = a;
                    bj = j;
                }
            });
        const bool ok = finite && m > -INFINITY;    // a point no live component scores above -inf is unassigned too
        double ll = 0.0;
        if (ok) {
            double s = 0.0;
            for (int j = 0; j < k; ++j) s += exp(row[j] - m);
            for (int j = 0; j < k; ++j) row[j] = exp(row[j] - m) / s;
            ll = m + log(s);
        } else if (live) {
            for (int j = 0; j < k; ++j) row[j] = 0.0;
        }
        if (live) {
            label[i] = ok ? bj : -1;
            if (loglik_point) loglik_point[i] = ll;
        }
        fold.add(ll, ok ? 1 : 0);       // + 0 where no point took part
    }
    if (tid == 0) w.ll[blockIdx.x] = fold.sum;
    if (tid == 64) w.assigned[blockIdx.x] = fold.n0;
}

// Init: the one-hot rows of label_in.  One workgroup per chunk; a thread per point finds its row's column (-1: an entry
// outside [0, k) or a non-finite point), then the round's rows are written by all threads, consecutive lanes to consecutive words.
__global__ __launch_bounds__(256) void gmm_onehot_kernel(const float* __restrict__ x, long N, int D, int k, long P,
                                                         const int* __restrict__ label_in, double* __restrict__ resp, GmmWs w) {
    __shared__ int scol[256];
    const int tid = threadIdx.x;
    const ChunkSpan span(blockIdx.x, P, N);
    RoundFold fold;     // bit 0: assigned
    for (long r0 = span.lo; r0 < span.hi; r0 += 256) {
        const long i = r0 + tid;
        bool finite = false;
        int col = -1;
        if (i < span.hi) {
            finite = point_finite(x, i, D);
            const int lab = label_in[i];
            if (finite && lab >= 0 && lab < k) col = lab;
        }
        scol[tid] = col;
        __syncthreads();
        const long n = span.hi - r0 < 256 ? span.hi - r0 : 256;
        for (long q = tid; q < n * k; q += 256) {
            const int r = (int)(q / k);
            resp[r0 * k + q] = scol[r] == (int)(q - (long)r * k) ? 1.0 : 0.0;
        }
        fold.add(0.0, finite ? 1 : 0);      // its barriers keep the next round's scol from this round's readers
    }
    if (tid == 64) w.assigned[blockIdx.x] = fold.n0;
}

// Accumulate: one workgroup per chunk, a thread per (component, t) pair with t in 0..D walking the chunk's points in index
// order: S1 and S2 about the incoming mean for t < D, R for t == D.  A zero responsibility is skipped: for a finite point that
// adds +-0 and changes nothing, and the all-zero row of an unassigned point keeps its coordinates out.  `frozen`: the step's
// snapshot of converged_at; once it is set the tail uses none of this.
__global__ __launch_bounds__(256) void gmm_accumulate_kernel(const float* __restrict__ x, long N, int D, int k, long P,
                                                             const double* __restrict__ mean, const double* __restrict__ resp,
                                                             const long long* __restrict__ frozen, GmmWs w) {
#pragma clang fp contract(off)
    if (frozen && *frozen != 0) return;
    const ChunkSpan span(blockIdx.x, P, N);
    const int width = 2 * D + 1;
    for (int p = threadIdx.x; p < k * (D + 1); p += 256) {
        const int j = p / (D + 1), t = p - j * (D + 1);
        double* out = w.part + ((long)blockIdx.x * k + j) * width;
        if (t == D) {
            double R = 0.0;
            for (long i = span.lo; i < span.hi; ++i) {
                const double r = resp[i * k + j];
                if (r == 0.0) continue;
                R += r;
            }
            out[2 * D] = R;
        } else {
            const double mu = mean[(long)j * D + t];
            double s1 = 0.0, s2 = 0.0;
            for (long i = span.lo; i < span.hi; ++i) {
                const double r = resp[i * k + j];
                if (r == 0.0) continue;
                const double d = (double)x[i * D + t] - mu;
                s1 += r * d;
                s2 += r * (d * d);
            }
            out[t] = s1;
            out[D + t] = s2;
        }
    }
}

enum { kGmmLabelOnly = 0, kGmmStep = 1, kGmmInit = 2 };

// Tail: the chunks added in index order.  Every workgroup takes the same decision from the snapshot and the summed loglik;
// where the M part is applied thread g < k (D + 1) writes its coordinate of mean and var, or (t == D) its weight.  Workgroup 0
// also writes the record.
__global__ __launch_bounds__(256) void gmm_tail_kernel(int D, int k, int chunks, int mode, double reg, double tol,
                                                       double* __restrict__ weight, double* __restrict__ mean, double* __restrict__ var,
                                                       svae_gmm_record* __restrict__ rec, GmmWs w) {
#pragma clang fp contract(off)
    __shared__ double s_ll;
    const int tid = threadIdx.x;
    const long g = (long)blockIdx.x * 256 + tid;
    const int width = 2 * D + 1;
    long long n = 0;
    for (int c = tid; c < chunks; c += 256) n += w.assigned[c];
    if (tid == 0) s_ll = mode != kGmmInit ? chunk_total(w.ll, chunks, 1, 0) : 0.0;
    const long long assigned = block_sum(n);        // its barriers publish s_ll too
    const double ll = s_ll;
    long long conv = 0, it = 0;
    bool apply = mode == kGmmInit;
    if (mode == kGmmStep) {
        conv = w.snap[0];
        it = w.snap[1];
        const double prev = __longlong_as_double(w.snap[2]);
        if (conv == 0) {
            if (it >= 1 && ll - prev <= tol * fabs(ll)) conv = it;
            else apply = true;
        }
    }
    if (apply && g < (long)k * (D + 1)) {
        const int j = (int)(g / (D + 1)), t = (int)(g - (long)j * (D + 1));
        const long stride = (long)k * width, at = (long)j * width;
        const double R = chunk_total(w.part, chunks, stride, at + 2 * D);
        if (t == D) weight[j] = R > 0.0 ? R / (double)assigned : 0.0;
        else if (R > 0.0) {
            const double delta = chunk_total(w.part, chunks, stride, at + t) / R;
            const double v = chunk_total(w.part, chunks, stride, at + D + t) / R - delta * delta;
            mean[(long)j * D + t] = mean[(long)j * D + t] + delta;
            var[(long)j * D + t] = (v > 0.0 ? v : 0.0) + reg;
        }
    }
    if (blockIdx.x != 0) return;
    long long dead = 0;
    for (int j = tid; j < k; j += 256) {
        if (apply) dead += !(chunk_total(w.part, chunks, (long)k * width, (long)j * width + 2 * D) > 0.0);
        else dead += !(weight[j] > 0.0);
    }
    dead = block_sum(dead);
    if (tid != 0) return;
    if (mode == kGmmInit) {
        rec->iterations = 0;
        rec->converged_at = 0;
        rec->loglik = 0.0;
        rec->previous = 0.0;
    } else {
        rec->loglik = ll;
    }
    rec->assigned = assigned;
    rec->dead = dead;
    if (mode == kGmmStep) {
        if (apply) {
            rec->iterations = it + 1;
            rec->previous = ll;
        } else {
            rec->converged_at = conv;
        }
    }
}

}  // namespace svae
