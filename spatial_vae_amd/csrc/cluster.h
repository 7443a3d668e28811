// k-means over (N, D) float points with (k, D) double centres (include/svae_cluster.h): k-means++ seeding and Lloyd steps.
// The distance, the tie rule and the two-level order of every sum are stated in the header; tests/kmeans_ref.py is the float64
// restatement the kernels are held to, bit for bit.  Doubles with contraction off, no atomics, no scratch: a point's
// coordinates sit in registers (loops unrolled to the template bound DMAX and predicated on D), the centres in LDS.  The
// chunks, the point and the order of the sums are latent_core.h's, shared with gmm.h and pca.h.
#pragma once
#include "latent_core.h"

namespace svae {

constexpr int kKmeansMaxD = 64;
constexpr int kKmeansMaxK = 1024;

// where the pieces of the workspace start, in 8-byte words
struct KmeansWs {
    double* dmin;        // (N) running minimum distances of the seeding
    double* inertia;     // (chunks) per-chunk sums: the winning distances of a step, the dmin of a seeding round
    long long* changed;  // (chunks)
    long long* assigned; // (chunks)
    long long* count;    // (chunks, k) members per chunk
    double* part;        // (chunks, k, D) coordinate sums per chunk
};

__host__ __device__ inline size_t kmeans_ws_words(long N, int D, int k) {
    const size_t C = LatentChunks(N).n;
    return (size_t)N + 3 * C + C * k + C * k * D;
}

inline KmeansWs kmeans_ws(void* ws, long N, int D, int k) {
    const long C = LatentChunks(N).n;
    KmeansWs w;
    w.dmin = static_cast<double*>(ws);
    w.inertia = w.dmin + N;
    w.changed = reinterpret_cast<long long*>(w.inertia + C);
    w.assigned = w.changed + C;
    w.count = w.assigned + C;
    w.part = reinterpret_cast<double*>(w.count + C * k);
    return w;
}

// d2 of the header against the D doubles at c (LDS: every lane reads the same address, a broadcast)
template <int DMAX>
__device__ __forceinline__ double kmeans_d2(const float (&xr)[DMAX], const double* c, int D) {
#pragma clang fp contract(off)
    double acc = 0.0;
#pragma unroll
    for (int t = 0; t < DMAX; ++t)
        if (t < D) {
            const double d = (double)xr[t] - c[t];
            acc += d * d;
        }
    return acc;
}

// the index the seeding falls back to: min(floor(u N), N - 1), and 0 for a u that is no number in [0, 1)
__device__ __forceinline__ long kmeans_fallback(double u, long N) {
    const double v = floor(u * (double)N);
    if (!(v >= 0.0)) return 0;
    return v >= (double)(N - 1) ? N - 1 : (long)v;
}

// Assign: one workgroup per chunk, 256 points per round, one thread per point.  The labels go out, and per chunk the in-order
// sum of the winning distances and the changed / assigned counts (RoundFold).
template <int DMAX>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ x, long N, int D, int k, long P,
                                                            const double* __restrict__ centres, int* __restrict__ label,
                                                            const long long* __restrict__ iterations, KmeansWs w) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const ChunkSpan span(blockIdx.x, P, N);
    const bool first = *iterations == 0;
    RoundFold fold;     // sum: inertia; bit 0: assigned, bit 1: changed
    for (long r0 = span.lo; r0 < span.hi; r0 += 256) {
        const long i = r0 + tid;
        const bool live = i < span.hi;
        float xr[DMAX];
        const bool finite = point_load<DMAX>(x, i, live, D, xr);
        double best = 0.0;
        int bj = 0;
        slab_walk(
            k, D, finite, [&](int j, int t) { return centres[(long)j * D + t]; },
            [&](int j, const double* c) {
                const double d = kmeans_d2<DMAX>(xr, c, D);
                if (j == 0 || d < best) {
                    best = d;
                    bj = j;
                }
            });
        int flag = 0;
        if (live) {
            const int lab = finite ? bj : -1;
            const bool ch = first ? finite : label[i] != lab;
            label[i] = lab;
            flag = (finite ? 1 : 0) | (ch ? 2 : 0);
        }
        fold.add(best, flag);       // + 0 where no point won: exact, the values are >= 0
    }
    if (tid == 0) w.inertia[blockIdx.x] = fold.sum;
    if (tid == 64) {
        w.changed[blockIdx.x] = fold.n1;
        w.assigned[blockIdx.x] = fold.n0;
    }
}

// Accumulate: one workgroup per chunk; with `update` a thread per (centre, coordinate) pair walks the chunk's labels in index
// order and adds the coordinates of its centre's points (the pattern of class_sums_update_kernel), and the pair of coordinate
// 0 counts them; without, a thread per centre only counts.
__global__ __launch_bounds__(256) void kmeans_accumulate_kernel(const float* __restrict__ x, long N, int D, int k, long P, int update,
                                                                const int* __restrict__ label, KmeansWs w) {
#pragma clang fp contract(off)
    const ChunkSpan span(blockIdx.x, P, N);
    const int pairs = update ? k * D : k;
    for (int p = threadIdx.x; p < pairs; p += 256) {
        const int j = update ? p / D : p;
        const int t = update ? p - j * D : 0;
        double acc = 0.0;
        long long n = 0;
        for (long i = span.lo; i < span.hi; ++i) {
            if (label[i] != j) continue;
            if (update) acc += (double)x[i * D + t];
            n += 1;
        }
        if (update) w.part[((long)blockIdx.x * k + j) * D + t] = acc;
        if (t == 0) w.count[(long)blockIdx.x * k + j] = n;
    }
}

// Tail: the chunks added in index order.  Thread g < k writes members[g]; with `update` thread g < k D writes its coordinate of
// the centres; workgroup 0 also writes the record.
__global__ __launch_bounds__(256) void kmeans_tail_kernel(int D, int k, int chunks, int update, double* __restrict__ centres,
                                                          long long* __restrict__ members, svae_kmeans_record* __restrict__ rec,
                                                          KmeansWs w) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const long g = (long)blockIdx.x * 256 + tid;
    if (g < k) members[g] = chunk_total(w.count, chunks, k, g);
    if (update && g < (long)k * D) {
        const long long n = chunk_total(w.count, chunks, k, g / D);
        const double s = chunk_total(w.part, chunks, (long)k * D, g);
        if (n > 0) centres[g] = s / (double)n;
    }
    if (blockIdx.x != 0) return;
    long long empty = 0, changed = 0, assigned = 0;
    for (int j = tid; j < k; j += 256) empty += chunk_total(w.count, chunks, k, j) == 0;
    for (int c = tid; c < chunks; c += 256) {
        changed += w.changed[c];
        assigned += w.assigned[c];
    }
    empty = block_sum(empty);
    changed = block_sum(changed);
    assigned = block_sum(assigned);
    if (tid != 0) return;
    rec->changed = changed;
    rec->assigned = assigned;
    rec->empty = empty;
    rec->inertia = chunk_total(w.inertia, chunks, 1, 0);
    if (update) {
        const long long it = rec->iterations + 1;
        rec->iterations = it;
        if (rec->converged_at == 0 && changed == 0) rec->converged_at = it;
    }
}

// Seeding, distances: one workgroup per chunk.  dmin[i] = d2 to the seed chosen last (centres row `last`), or the smaller of
// that and what it held (`first` == 0); 0 for an unassigned point.  The chunk's in-order sum of dmin goes to w.inertia.
template <int DMAX>
__global__ __launch_bounds__(256) void kmeans_seed_dist_kernel(const float* __restrict__ x, long N, int D, long P,
                                                               const double* __restrict__ centres, int last, int first, KmeansWs w) {
#pragma clang fp contract(off)
    __shared__ double sc[kKmeansMaxD];
    const int tid = threadIdx.x;
    const ChunkSpan span(blockIdx.x, P, N);
    if (tid < D) sc[tid] = centres[(long)last * D + tid];
    __syncthreads();
    RoundFold fold;
    for (long r0 = span.lo; r0 < span.hi; r0 += 256) {
        const long i = r0 + tid;
        const bool live = i < span.hi;
        float xr[DMAX];
        double m = 0.0;
        if (point_load<DMAX>(x, i, live, D, xr)) {
            m = kmeans_d2<DMAX>(xr, sc, D);
            if (!first) {
                const double old = w.dmin[i];
                m = old < m ? old : m;
            }
        }
        if (live) w.dmin[i] = m;
        fold.add(m, 0);
    }
    if (tid == 0) w.inertia[blockIdx.x] = fold.sum;
}

// Seeding, the pick of centre j: one workgroup.  Thread 0 adds the chunk totals in order, finds the first chunk whose
// inclusive prefix exceeds u[j] T, then walks that chunk's dmin (staged 256 at a time) for the first point whose does.
__global__ __launch_bounds__(256) void kmeans_seed_pick_kernel(const float* __restrict__ x, long N, int D, long P, int chunks, int j,
                                                               const double* __restrict__ u, double* __restrict__ centres,
                                                               int* __restrict__ seed_index, KmeansWs w) {
#pragma clang fp contract(off)
    __shared__ double sd[256];
    __shared__ long s_pick, s_chunk;
    __shared__ double s_pre, s_target;
    __shared__ int s_done;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_pick = kmeans_fallback(u[j], N);
        s_chunk = -1;
        s_done = 0;
        if (j > 0) {
            const double T = chunk_total(w.inertia, chunks, 1, 0);
            if (T > 0.0 && isfinite(T)) {
                const double target = u[j] * T;
                double pre = 0.0;
                for (int c = 0; c < chunks; ++c) {
                    const double next = pre + w.inertia[c];
                    if (next > target) {
                        s_chunk = c;
                        s_pre = pre;
                        s_target = target;
                        break;
                    }
                    pre = next;
                }
            }
        }
    }
    __syncthreads();
    if (s_chunk >= 0) {         // uniform: every thread reads the same LDS word
        const ChunkSpan span(s_chunk, P, N);
        double run = 0.0;       // thread 0's running sum inside the chunk
        for (long r0 = span.lo; r0 < span.hi; r0 += 256) {
            const long i = r0 + tid;
            sd[tid] = i < span.hi ? w.dmin[i] : 0.0;
            __syncthreads();
            if (tid == 0) {
                const int n = span.hi - r0 < 256 ? (int)(span.hi - r0) : 256;
                for (int q = 0; q < n; ++q) {
                    run += sd[q];
                    if (s_pre + run > s_target) {
                        s_pick = r0 + q;
                        s_done = 1;
                        break;
                    }
                }
            }
            __syncthreads();
            if (s_done) break;
        }
    }
    const long pick = s_pick;
    if (tid < D) centres[(long)j * D + tid] = (double)x[pick * D + tid];
    if (tid == 0) seed_index[j] = (int)pick;
}

}  // namespace svae
