// Latent-space neighbour averages (include/svae_neighbours.h): the exact K-nearest-neighbour search over the content latents and
// the gather-average of the neighbours' aligned images.  The arithmetic, the total order and the order of every sum are stated
// in the header; tests/neighbours_ref.py is the float64 restatement the kernels are held to.  Plain fp64 vector kernels: doubles
// with contraction off, no atomics, no matrix instruction, no scratch.
#pragma once
#include "common.h"

namespace svae {

constexpr int kNbrMaxK = 256;
constexpr int kNbrMaxD = 512;
constexpr int kNbrMaxT = kNbrMaxK + 1;
constexpr int kNbrQueries = 4;                  // queries of one workgroup: one per wave
constexpr int kNbrTile = 256;                   // candidates staged at a time: four per lane
constexpr int kNbrChunk = 16;                   // coordinates of them staged at a time
constexpr int kNbrPitch = kNbrChunk + 1;        // odd: lane l reads row l, and 32 rows fall on 32 different bank pairs

// (d, i) comes strictly before (e, j) in the header's total order
__device__ __forceinline__ bool nbr_before(double d, long long i, double e, long long j) { return d < e || (d == e && i < j); }

// One workgroup per kNbrQueries queries, one wave per query; all four waves stage every tile of candidates and read it once.
// A wave's list lives in LDS.  Per tile a lane forms d2 for its four candidates, in the header's order whatever the chunking
// (the accumulators outlive the chunks); what is not below the list's last entry is dropped, the survivors are compacted by
// ballot and prefix count and merged by rank: every element of list and survivors counts the elements that precede it (list
// before survivor and earlier survivor before later one where the keys are equal) and writes itself there if that is below K.
// Every barrier is reached by all four waves: the loops around them run on M, D and a flag read after a barrier, never on a
// wave's own data, and a wave without a query or without survivors walks through them empty-handed.
__global__ __launch_bounds__(256) void nbr_search_kernel(const double* __restrict__ query, int B, long long query_base,
                                                         const double* __restrict__ cand, int M, long long cand_base, int D, int K,
                                                         double* best_d2, long long* best_index) {
#pragma clang fp contract(off)
    __shared__ double s_tile[kNbrTile * kNbrPitch];
    __shared__ double s_query[kNbrQueries * kNbrChunk];
    __shared__ double s_list_d[kNbrQueries * kNbrMaxK];
    __shared__ long long s_list_i[kNbrQueries * kNbrMaxK];
    __shared__ double s_surv_d[kNbrQueries * kNbrTile];
    __shared__ int s_surv_c[kNbrQueries * kNbrTile];
    __shared__ int s_any[kNbrQueries];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int first = blockIdx.x * kNbrQueries;
    const int b = first + wave;
    const bool live = b < B;
    const long long self = query_base + b;
    const double inf = __builtin_huge_val();
    double* list_d = s_list_d + wave * kNbrMaxK;
    long long* list_i = s_list_i + wave * kNbrMaxK;
    double* surv_d = s_surv_d + wave * kNbrTile;
    int* surv_c = s_surv_c + wave * kNbrTile;

    int L = 0;      // the list's non-empty entries: the same number in every lane of the wave
    for (int p0 = 0; p0 < K; p0 += 64) {
        const int p = p0 + lane;
        bool has = false;
        if (live && p < K) {
            const long long i = best_index[(long)b * K + p];
            list_d[p] = best_d2[(long)b * K + p];
            list_i[p] = i;
            has = i >= 0;
        }
        L += __popcll(__ballot(has));
    }
    __syncthreads();    // the lists are in LDS

    for (long c0 = 0; c0 < M; c0 += kNbrTile) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < D; j0 += kNbrChunk) {
            const int dc = D - j0 < kNbrChunk ? D - j0 : kNbrChunk;
            __syncthreads();    // the last chunk has been read
            for (int e = tid; e < kNbrTile * dc; e += 256) {
                const int c = e / dc, j = e - c * dc;
                const long cc = c0 + c;
                s_tile[c * kNbrPitch + j] = cc < M ? cand[cc * D + j0 + j] : 0.0;
            }
            if (tid < kNbrQueries * dc) {
                const int w = tid / dc, j = tid - w * dc;
                s_query[w * kNbrChunk + j] = first + w < B ? query[(long)(first + w) * D + j0 + j] : 0.0;
            }
            __syncthreads();    // this chunk is staged
            for (int j = 0; j < dc; ++j) {
                const double qj = s_query[wave * kNbrChunk + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double t = qj - s_tile[(i * 64 + lane) * kNbrPitch + j];
                    acc[i] += t * t;
                }
            }
        }

        // the survivors of this tile, compacted in candidate order
        const bool full = L == K;
        const double last_d = full ? list_d[K - 1] : inf;
        const long long last_i = full ? list_i[K - 1] : -1;
        int S = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = i * 64 + lane;
            const long long id = cand_base + c0 + c;
            const bool pass = live && c0 + c < M && id != self && acc[i] < inf && (!full || nbr_before(acc[i], id, last_d, last_i));
            const unsigned long long mask = __ballot(pass);
            if (pass) {
                const int at = S + __popcll(mask & ((1ull << lane) - 1ull));
                surv_d[at] = acc[i];
                surv_c[at] = c;
            }
            S += __popcll(mask);
        }
        if (lane == 0) s_any[wave] = S;
        __syncthreads();    // the survivors and the four counts are written
        if ((s_any[0] | s_any[1] | s_any[2] | s_any[3]) == 0) continue;    // the same decision in every thread: the common case

        // the merge by rank: every element first finds its place, held in registers, ...
        double md[8];
        long long mi[8];
        int mr[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = u * 64 + lane;
            mr[u] = kNbrMaxK;
            md[u] = 0.0;
            mi[u] = 0;
            if (S > 0 && p < L) {
                const double d = list_d[p];
                const long long id = list_i[p];
                int r = p;
                for (int s = 0; s < S; ++s) r += nbr_before(surv_d[s], cand_base + c0 + surv_c[s], d, id) ? 1 : 0;
                md[u] = d, mi[u] = id, mr[u] = r;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = u * 64 + lane;
            mr[4 + u] = kNbrMaxK;
            md[4 + u] = 0.0;
            mi[4 + u] = 0;
            if (s < S) {
                const double d = surv_d[s];
                const long long id = cand_base + c0 + surv_c[s];
                int r = 0;
                for (int p = 0; p < L; ++p) r += nbr_before(d, id, list_d[p], list_i[p]) ? 0 : 1;
                for (int o = 0; o < S; ++o) {
                    const double e = surv_d[o];
                    const long long oid = cand_base + c0 + surv_c[o];
                    r += (nbr_before(e, oid, d, id) || (e == d && oid == id && o < s)) ? 1 : 0;
                }
                md[4 + u] = d, mi[4 + u] = id, mr[4 + u] = r;
            }
        }
        __syncthreads();    // ... and, once every element has been read, writes itself there
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (mr[u] < K) {
                list_d[mr[u]] = md[u];
                list_i[mr[u]] = mi[u];
            }
        L = L + S < K ? L + S : K;
        __syncthreads();    // the lists are whole again
    }

    __syncthreads();
    if (live)
        for (int p = lane; p < K; p += 64) {
            best_d2[(long)b * K + p] = list_d[p];
            best_index[(long)b * K + p] = list_i[p];
        }
}

// One workgroup per output image: its T slots go to LDS once, then the threads stride over the N C values, so that every
// neighbour's row is read coalesced; a thread walks the slots of its value in index order.
__global__ __launch_bounds__(256) void nbr_average_kernel(const float* __restrict__ stack, const uint8_t* __restrict__ cover,
                                                          long long images, int N, int C, const long long* __restrict__ index,
                                                          const double* __restrict__ weight, int T, float* __restrict__ average,
                                                          double* __restrict__ support) {
#pragma clang fp contract(off)
    __shared__ long long s_index[kNbrMaxT];
    __shared__ double s_weight[kNbrMaxT];
    const long b = blockIdx.x;
    for (int t = threadIdx.x; t < T; t += 256) {
        const long long i = index[b * T + t];
        s_index[t] = i >= 0 && i < images ? i : -1;
        s_weight[t] = weight ? weight[b * T + t] : 1.0;
    }
    __syncthreads();    // the slots are in LDS
    const long D = (long)N * C;
    for (long e = threadIdx.x; e < D; e += 256) {
        const long j = e / C;
        double num = 0.0, den = 0.0;
        for (int t = 0; t < T; ++t) {
            const long long i = s_index[t];
            if (i < 0) continue;
            if (cover && cover[i * N + j] == 0) continue;
            const double w = s_weight[t];
            num += w * (double)stack[i * D + e];
            den += w;
        }
        average[b * D + e] = den > 0.0 ? (float)(num / den) : 0.0f;
        if (support && e == j * C) support[b * N + j] = den;
    }
}

}  // namespace svae
