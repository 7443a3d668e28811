// What the statistics over the content latents share (cluster.h, gmm.h, pca.h): the chunk rule, a point in registers, and the
// order of every sum over points -- 256 points a round added in index order, the rounds of a chunk in order, the chunks in
// order.  The float64 references of the three state that order; it is written here once.  Every kernel runs 256 threads.
#pragma once
#include "common.h"

namespace svae {

constexpr int kLatentSlab = 4096;       // doubles of per-class parameters staged in LDS at a time (32 KiB)

// The chunks of every reduction over N points: P points each, 256 doubled until at most 1024 chunks are left
// (svae_grad_guard_norm's rule on N), so the order of a sum depends on N only.
struct LatentChunks {
    long P;     // points per chunk
    int n;      // chunks
    __host__ __device__ explicit LatentChunks(long N) : P(256) {
        while ((N + P - 1) / P > 1024) P *= 2;
        n = (int)((N + P - 1) / P);
    }
};
// chunk c's points [lo, hi): a workgroup's share, the last one cut at N
struct ChunkSpan {
    long lo, hi;
    __device__ __forceinline__ ChunkSpan(long c, long P, long N) : lo(c * P), hi(lo + P < N ? lo + P : N) {}
};

// whether point i's D coordinates are all finite
__device__ __forceinline__ bool point_finite(const float* __restrict__ x, long i, int D) {
    bool finite = true;
    for (int t = 0; t < D; ++t) finite = finite && isfinite(x[i * D + t]);
    return finite;
}

// Point i into registers, zero beyond D; returns whether it is live and finite.  A dead lane (one past its chunk's end) reads
// nothing and holds zeros, so that it can walk the slabs with the others.
template <int DMAX>
__device__ __forceinline__ bool point_load(const float* __restrict__ x, long i, bool live, int D, float (&xr)[DMAX]) {
    bool finite = live;
#pragma unroll
    for (int t = 0; t < DMAX; ++t) xr[t] = 0.0f;
    if (live) {     // one branch around the loads, so that each stays predicated on the uniform t < D alone
#pragma unroll
        for (int t = 0; t < DMAX; ++t)
            if (t < D) {
                xr[t] = x[i * D + t];
                finite = finite && isfinite(xr[t]);
            }
    }
    return finite;
}

// The fold of the rounds of a chunk, 256 points a round and a thread each.  add() is called by all threads once a round:
// thread 0 adds the round's 256 values to its `sum` in index order, thread 64 counts bits 0 and 1 of the 256 flags into its
// n0 and n1 -- two threads because they sit in different waves, so the two walks overlap.  The other threads' members stay 0,
// and the walk of a member no caller reads is compiled away (its 1 or 2 KiB of LDS stay).  Both barriers are add()'s own: on
// return every LDS write made before the call is visible to all threads and the fold's buffers are free, so a caller needs no
// barrier of its own around it and never leans on a neighbour's.
struct RoundFold {
    double sum = 0.0;
    long long n0 = 0, n1 = 0;
    __device__ __forceinline__ void add(double v, int flags) {
#pragma clang fp contract(off)
        __shared__ double sd[256];
        __shared__ int sf[256];
        const int tid = threadIdx.x;
        sd[tid] = v;
        sf[tid] = flags;
        __syncthreads();
        if (tid == 0) {
            for (int q = 0; q < 256; ++q) sum += sd[q];
        } else if (tid == 64) {
            for (int q = 0; q < 256; ++q) {
                n0 += sf[q] & 1;
                n1 += (sf[q] >> 1) & 1;
            }
        }
        __syncthreads();
    }
};

// The walk of k rows of `width` doubles through the LDS slab, as many whole rows at a time as fit.  All 256 threads call it
// and stage together: stage(j, u) gives entry u of row j.  Then a thread with `active` calls row(j, its `width` doubles in LDS)
// for each staged row, in index order; every lane reads the same address, a broadcast.  The first barrier frees the slab of
// its earlier readers, the second publishes it; the walk may be called again at once.
template <class Stage, class Row>
__device__ __forceinline__ void slab_walk(int k, int width, bool active, Stage stage, Row row) {
    __shared__ double sc[kLatentSlab];
    const int per = kLatentSlab / width;
    for (int j0 = 0; j0 < k; j0 += per) {
        const int nj = k - j0 < per ? k - j0 : per;
        __syncthreads();
        for (int q = threadIdx.x; q < nj * width; q += 256) {
            const int j = q / width, u = q - j * width;
            sc[q] = stage(j0 + j, u);
        }
        __syncthreads();
        if (active)
            for (int j = 0; j < nj; ++j) row(j0 + j, sc + j * width);
    }
}

// the chunks' partial sums base[c * stride + at] added in index order
template <class T>
__device__ __forceinline__ T chunk_total(const T* __restrict__ base, int chunks, long stride, long at) {
#pragma clang fp contract(off)
    T s = 0;
    for (int c = 0; c < chunks; ++c) s += base[c * stride + at];
    return s;
}

// The sum of the 256 threads' n, returned to all of them (integers: any order gives the same number).  Called by all threads;
// its two barriers also make every earlier LDS write visible, and it may be called again at once.
__device__ __forceinline__ long long block_sum(long long n) {
    __shared__ long long red[256];
    __shared__ long long total;
    red[threadIdx.x] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long s = 0;
        for (int q = 0; q < 256; ++q) s += red[q];
        total = s;
    }
    __syncthreads();
    return total;
}

}  // namespace svae
