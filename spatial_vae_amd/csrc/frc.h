// Fourier ring correlation and the filter by per-ring weights (include/svae_frc.h).  The DFT is ctfcorr.h's construction:
// separable, doubles with contraction off, twiddles from the sincospi table indexed by k*v mod len, every sum in index order.
// frc_kernel runs the two forward passes only, on the complex plane z = w (a + i b); the spectra of a and b are separated from
// Z(u,v) and Z(-u,-v), their three products staged per frequency in the planes the passes have freed, and one thread per ring
// walks the frequencies upwards: no atomics, so two runs give the same bits.  frc_filter_kernel is dft_filter_plane with a
// filter that looks the ring up.  tests/frc_ref.py is the float64 restatement (np.fft) both are held to.
#pragma once
#include "ctfcorr.h"

namespace svae {

// the ring of frequency (u, v) of an n x m plane, L = min(n, m): the largest r >= 1 with (2r-1)^2 (n m)^2 <= 4 ((ku L m)^2 +
// (kv L n)^2), 0 where there is none.  The double estimate is within one of it and the integer comparisons decide; with
// n, m <= 1024 the largest product is 2.3e18.
__device__ __forceinline__ int frc_ring(int u, int v, int n, int m, int L) {
    const long ku = u <= (n - 1) / 2 ? u : u - n;
    const long kv = v <= (m - 1) / 2 ? v : v - m;
    const long A = ku * L * m, B = kv * L * n;
    const long S = 4 * (A * A + B * B);
    const long nm = (long)n * m, T = nm * nm;
    long r = (long)((sqrt((double)S / (double)T) + 1.0) * 0.5);
    while ((2 * r + 1) * (2 * r + 1) * T <= S) ++r;
    while (r > 0 && (2 * r - 1) * (2 * r - 1) * T > S) --r;
    return (int)r;
}

// the soft circular mask at row a, column b; radius == 0: none
__device__ __forceinline__ double frc_mask(int a, int b, int n, int m, double radius, double edge) {
#pragma clang fp contract(off)
    if (radius == 0.0) return 1.0;
    const double dy = (double)a - 0.5 * (n - 1), dx = (double)b - 0.5 * (m - 1);
    const double d = sqrt(dx * dx + dy * dy);
    if (d <= radius) return 1.0;
    if (d >= radius + edge) return 0.0;
    return 0.5 * (1.0 + cospi((d - radius) / edge));
}

// dft_twiddles with entry len - k the exact conjugate of entry k (both from sincospi at min(k, len - k)).  With it a real plane
// transforms to Z(-u,-v) = conj Z(u,v) bit for bit, so a half that is exactly 0 separates to FB = 0 and pb = 0 exactly, which
// is what makes its FRC 0 and not a quotient of rounding errors.  The caller synchronises before the first use.
__device__ __forceinline__ void frc_twiddles(double2* wm, double2* wn, int n, int m) {
    for (int k = threadIdx.x; k < m; k += 256) {
        const bool low = 2 * k <= m;
        double sn, cn;
        sincospi(2.0 * (low ? k : m - k) / m, &sn, &cn);
        wm[k] = make_double2(cn, low ? sn : -sn);
    }
    for (int k = threadIdx.x; k < n; k += 256) {
        const bool low = 2 * k <= n;
        double sn, cn;
        sincospi(2.0 * (low ? k : n - k) / n, &sn, &cn);
        wn[k] = make_double2(cn, low ? sn : -sn);
    }
}

// One workgroup per plane (SCRATCH: the grid strides over the planes).  Passes: z = w (a + i b) into Q; rows forward Q -> P;
// columns forward P -> Q, which now holds Z; per pair of frequencies e <= e' = (-u, -v), by one thread, which alone touches
// the two entries: P[e] = P[e'] = (num, pa), Q[e] = Q[e'] = (pb, ring or -1); then thread r walks e upwards for ring r.
template <bool SCRATCH>
__global__ void __launch_bounds__(256) frc_kernel(const double* __restrict__ a, const double* __restrict__ b, int planes, int n,
                                                   int m, double radius, double edge, double* __restrict__ sums,
                                                   double* __restrict__ frc, int* __restrict__ ring_count,
                                                   double* __restrict__ scratch) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_ctfcorr[];
    const DftPlanes<SCRATCH> pl(lds_ctfcorr, scratch, n, m);
    double2* P = pl.P;
    double2* Q = pl.Q;
    const double2* wm = pl.wm;
    const double2* wn = pl.wn;
    const int N = n * m;
    const int L = n < m ? n : m, R = L / 2 + 1;
    frc_twiddles(pl.wm, pl.wn, n, m);
    for (int p = blockIdx.x; p < planes; p += gridDim.x) {
        const double* pa_src = a + (long)p * N;
        const double* pb_src = b + (long)p * N;
        for (int e = threadIdx.x; e < N; e += 256) {
            const int r = e / m, c = e - r * m;
            const double w = frc_mask(r, c, n, m, radius, edge);
            Q[e] = make_double2(w * pa_src[e], w * pb_src[e]);
        }
        __syncthreads();   // the input and the twiddles are in place
        for (int e = threadIdx.x; e < N; e += 256) {  // P[r][v] = sum_c Q[r][c] e^{-2 pi i c v / m}
            const int r = e / m, v = e - r * m;
            double re = 0.0, im = 0.0;
            int k = 0;
            for (int c = 0; c < m; ++c) {
                const double2 t = Q[r * m + c];
                const double2 w = wm[k];
                re += t.x * w.x + t.y * w.y;
                im += t.y * w.x - t.x * w.y;
                k += v;
                if (k >= m) k -= m;
            }
            P[e] = make_double2(re, im);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < N; e += 256) {  // Q[u][v] = sum_r P[r][v] e^{-2 pi i r u / n}
            const int u = e / m, v = e - u * m;
            double re = 0.0, im = 0.0;
            int k = 0;
            for (int r = 0; r < n; ++r) {
                const double2 t = P[r * m + v];
                const double2 w = wn[k];
                re += t.x * w.x + t.y * w.y;
                im += t.y * w.x - t.x * w.y;
                k += u;
                if (k >= n) k -= n;
            }
            Q[e] = make_double2(re, im);
        }
        __syncthreads();
        for (int e = threadIdx.x; e < N; e += 256) {
            const int u = e / m, v = e - u * m;
            const int e2 = (u ? n - u : 0) * m + (v ? m - v : 0);
            if (e2 < e) continue;   // the partner's thread does both
            const double2 z1 = Q[e], z2 = Q[e2];
            const double ax = 0.5 * (z1.x + z2.x), ay = 0.5 * (z1.y - z2.y);    // FA = (Z + conj Z') / 2
            const double bx = 0.5 * (z1.y + z2.y), by = -0.5 * (z1.x - z2.x);   // FB = (Z - conj Z') / (2i)
            const int ring = frc_ring(u, v, n, m, L);
            const double2 first = make_double2(ax * bx + ay * by, ax * ax + ay * ay);
            const double2 second = make_double2(bx * bx + by * by, ring < R ? (double)ring : -1.0);
            P[e] = first;
            P[e2] = first;
            Q[e] = second;
            Q[e2] = second;
        }
        __syncthreads();
        for (int r = threadIdx.x; r < R; r += 256) {
            const double want = (double)r;
            double num = 0.0, sa = 0.0, sb = 0.0;
            int count = 0;
            for (int e = 0; e < N; ++e) {
                const double2 q = Q[e];
                if (q.y != want) continue;
                const double2 t = P[e];
                num += t.x;
                sa += t.y;
                sb += q.x;
                ++count;
            }
            double* s = sums + ((long)p * R + r) * 3;
            s[0] = num;
            s[1] = sa;
            s[2] = sb;
            const double pp = sa * sb;
            frc[(long)p * R + r] = pp == 0.0 ? 0.0 : num / sqrt(pp);
            if (p == 0) ring_count[r] = count;
        }
        __syncthreads();   // the walk has finished with P and Q before the next plane is loaded
    }
}

// One workgroup per plane (SCRATCH: the grid strides over the planes): out[p] = Re IDFT( weight[p, ring] DFT(x[p]) ), a
// frequency in no ring contributing 0.
template <bool SCRATCH>
__global__ void __launch_bounds__(256) frc_filter_kernel(const double* __restrict__ x, const double* __restrict__ weight,
                                                          int planes, int n, int m, float* __restrict__ out,
                                                          double* __restrict__ scratch) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_ctfcorr[];
    const DftPlanes<SCRATCH> pl(lds_ctfcorr, scratch, n, m);
    const int N = n * m;
    const int L = n < m ? n : m, R = L / 2 + 1;
    dft_twiddles(pl.wm, pl.wn, n, m);
    for (int p = blockIdx.x; p < planes; p += gridDim.x) {
        const double* src = x + (long)p * N;
        const double* wp = weight + (long)p * R;
        double* in = reinterpret_cast<double*>(pl.Q);   // free: the previous plane's last pass reads P only
        for (int e = threadIdx.x; e < N; e += 256) in[e] = src[e];
        __syncthreads();
        dft_filter_plane(pl.P, pl.Q, pl.wm, pl.wn, n, m,
                         [&](int, int u, int v, double re, double im) {
                             const int ring = frc_ring(u, v, n, m, L);
                             if (ring >= R) return make_double2(0.0, 0.0);
                             const double w = wp[ring];
                             return make_double2(re * w, im * w);
                         },
                         out + (long)p * N);
    }
}

}  // namespace svae
