// CTF correction in Fourier space (include/svae_ctfcorr.h): each observed particle multiplied by the sign of its own transfer
// function (phase flipping) or by the transfer function itself, the per-class sums of the squared transfer functions, and the
// Wiener quotient of a class sum by them.  The closed form is the one ctf_filter_kernel evaluates (elementwise.h; restated here
// so that svae_ctf_filter's code, and with it its bits, stay what they were), on the image's own n x m frequency grid.  The 2-D
// DFT is ctf_filter_kernel's construction run forwards and back: separable, doubles with contraction off, twiddles from a
// sincospi table indexed by k*v mod len, every sum in index order, one rounding to float on the way out; no atomics.
// tests/ctfcorr_ref.py is the float64 restatement (np.fft) the kernels are held to.
#pragma once
#include "common.h"

namespace svae {

// what the closed form needs of one row of the parameter table [defocus um, cs mm, voltage kV, apix A, bfactor, ampcont %,
// dfdiff, dfang deg].  Both defoci are defocus*10000 (ctf.py:47-48), so ctf_filter_kernel's df = 0.5*(dfu + dfv + (dfu - dfv)*cos(..))
// is dfu exactly, whatever the angle: neither dfdiff nor dfang enters.
struct CtfRow {
    double apix, df, lam, cs, w, amp, bfactor;
};

__device__ __forceinline__ CtfRow ctf_row(const double* __restrict__ p, double scale) {
#pragma clang fp contract(off)
    CtfRow r;
    r.apix = p[3] * scale;
    r.df = p[0] * 10000.0;
    const double volt = p[2] * 1000.0;
    r.cs = p[1] * 1e7;
    r.w = p[5] / 100.0;
    r.bfactor = p[4];
    r.lam = 12.2639 / sqrt(volt + 0.97845e-6 * volt * volt);
    r.amp = sqrt(1.0 - r.w * r.w);
    return r;
}

// c(a, b), the CTF with its B-factor envelope at the fftfreq indices a of n (rows) and b of m (columns); *u is c without the
// envelope, whose sign is c's wherever the envelope has not underflowed.  H = -c (the minus sign of ctf.py:54).
__device__ __forceinline__ double ctf_at(const CtfRow& r, int a, int b, int n, int m, double* u) {
#pragma clang fp contract(off)
    const double fx = (double)(a <= (n - 1) / 2 ? a : a - n) / n / r.apix;
    const double fy = (double)(b <= (m - 1) / 2 ? b : b - m) / m / r.apix;
    const double s2 = fx * fx + fy * fy;
    const double gamma = 2.0 * M_PI * (-0.5 * r.df * r.lam * s2 + 0.25 * r.cs * r.lam * r.lam * r.lam * s2 * s2);
    const double osc = r.amp * sin(gamma) - r.w * cos(gamma);
    *u = osc;
    return osc * exp(-r.bfactor / 4.0 * s2);
}

// wm[k] = e^{2 pi i k / m}, wn[k] = e^{2 pi i k / n}; the caller synchronises before the first use
__device__ __forceinline__ void dft_twiddles(double2* wm, double2* wn, int n, int m) {
    for (int k = threadIdx.x; k < m; k += 256) {
        double sn, cn;
        sincospi(2.0 * k / m, &sn, &cn);
        wm[k] = make_double2(cn, sn);
    }
    for (int k = threadIdx.x; k < n; k += 256) {
        double sn, cn;
        sincospi(2.0 * k / n, &sn, &cn);
        wn[k] = make_double2(cn, sn);
    }
}

// out = Re IDFT( filter( DFT(plane) ) ) / (n m) for one n x m plane, by the 256 threads of a workgroup.  P and Q are two
// complex planes of n*m double2 each; on entry the real input sits in the first n*m doubles of Q, and every thread has passed
// a barrier since it was written.  filter(e, u, v, re, im) gives the filtered coefficient at the frequency indices (u, v),
// e = u*m + v.  Passes: rows forward Q -> P, columns forward P -> Q (filtered as it is stored), columns back Q -> P, rows
// back P -> out (real part only).  On return P may still be read by other threads and Q is free.
template <class Filter>
__device__ __forceinline__ void dft_filter_plane(double2* P, double2* Q, const double2* wm, const double2* wn, int n, int m,
                                                 Filter filter, float* __restrict__ out) {
#pragma clang fp contract(off)
    const double* y = reinterpret_cast<const double*>(Q);
    const int N = n * m;
    for (int e = threadIdx.x; e < N; e += 256) {  // P[a][v] = sum_b y[a][b] e^{-2 pi i b v / m}
        const int a = e / m, v = e - a * m;
        double re = 0.0, im = 0.0;
        int k = 0;
        for (int b = 0; b < m; ++b) {
            const double yv = y[a * m + b];
            re += yv * wm[k].x;
            im += yv * wm[k].y;
            k += v;
            if (k >= m) k -= m;
        }
        P[e] = make_double2(re, -im);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < N; e += 256) {  // Q[u][v] = filter( sum_a P[a][v] e^{-2 pi i a u / n} )
        const int u = e / m, v = e - u * m;
        double re = 0.0, im = 0.0;
        int k = 0;
        for (int a = 0; a < n; ++a) {
            const double2 t = P[a * m + v];
            const double2 w = wn[k];
            re += t.x * w.x + t.y * w.y;
            im += t.y * w.x - t.x * w.y;
            k += u;
            if (k >= n) k -= n;
        }
        Q[e] = filter(e, u, v, re, im);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < N; e += 256) {  // P[a][v] = sum_u Q[u][v] e^{+2 pi i u a / n}
        const int a = e / m, v = e - a * m;
        double re = 0.0, im = 0.0;
        int k = 0;
        for (int u = 0; u < n; ++u) {
            const double2 g = Q[u * m + v];
            const double2 w = wn[k];
            re += g.x * w.x - g.y * w.y;
            im += g.x * w.y + g.y * w.x;
            k += a;
            if (k >= n) k -= n;
        }
        P[e] = make_double2(re, im);
    }
    __syncthreads();
    const double inv = 1.0 / ((double)n * m);
    for (int e = threadIdx.x; e < N; e += 256) {  // out[a][b] = Re sum_v P[a][v] e^{+2 pi i v b / m} / (n m)
        const int a = e / m, b = e - a * m;
        double re = 0.0;
        int k = 0;
        for (int v = 0; v < m; ++v) {
            const double2 t = P[a * m + v];
            re += t.x * wm[k].x - t.y * wm[k].y;
            k += b;
            if (k >= m) k -= m;
        }
        out[e] = (float)(re * inv);
    }
}

// The two complex planes and the twiddles of a workgroup.  LDS: P | Q | wm | wn (32 n m + 16 (n + m) bytes, up to 71 x 71 in
// the 160 KiB of a CU).  SCRATCH = true: P and Q are the workgroup's slice of a caller-provided global area, only the
// twiddles stay in LDS, and the grid strides over the planes; the same arithmetic in the same order, so the same bits.
template <bool SCRATCH>
struct DftPlanes {
    double2 *P, *Q, *wm, *wn;
    __device__ __forceinline__ DftPlanes(double* lds, double* scratch, int n, int m) {
        const long N = (long)n * m;
        P = reinterpret_cast<double2*>(SCRATCH ? scratch + (long)blockIdx.x * 4 * N : lds);
        Q = P + N;
        wm = SCRATCH ? reinterpret_cast<double2*>(lds) : Q + N;
        wn = wm + m;
    }
};

// One workgroup per image (SCRATCH: the grid strides over the images).  mode 0: the coefficient times s = (u <= 0 ? +1 : -1),
// the sign of H = -c taken from the oscillating part; mode 1: times H.
template <bool SCRATCH>
__global__ void __launch_bounds__(256) ctf_apply_kernel(const float* __restrict__ y, const double* __restrict__ params, int B,
                                                         int n, int m, double scale, int mode, float* __restrict__ out,
                                                         double* __restrict__ scratch) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_ctfcorr[];
    const DftPlanes<SCRATCH> pl(lds_ctfcorr, scratch, n, m);
    const int N = n * m;
    dft_twiddles(pl.wm, pl.wn, n, m);
    for (int img = blockIdx.x; img < B; img += gridDim.x) {
        const CtfRow row = ctf_row(params + (long)img * 8, scale);
        const float* src = y + (long)img * N;
        double* in = reinterpret_cast<double*>(pl.Q);   // free: the previous image's last pass reads P only
        for (int e = threadIdx.x; e < N; e += 256) in[e] = (double)src[e];
        __syncthreads();   // the input and the twiddles are in place, and the previous image's last pass has finished with P
        dft_filter_plane(pl.P, pl.Q, pl.wm, pl.wn, n, m,
                         [&](int, int u, int v, double re, double im) {
                             double osc;
                             const double c = ctf_at(row, u, v, n, m, &osc);
                             const double h = mode == 0 ? (osc <= 0.0 ? 1.0 : -1.0) : -c;
                             return make_double2(re * h, im * h);
                         },
                         out + (long)img * N);
    }
}

// One thread per (class k, frequency e): walks the call's B labels in index order and adds H_b(e)^2 of the images of its
// class into den[k, e]; the closed form is evaluated only where the label matches.
__global__ void ctf_power_update_kernel(const double* __restrict__ params, const int* __restrict__ label, int B, int n, int m,
                                        double scale, int n_classes, double* __restrict__ den) {
#pragma clang fp contract(off)
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int N = n * m;
    if (t >= (long)n_classes * N) return;
    const int k = (int)(t / N);
    const int e = (int)(t - (long)k * N);
    const int a = e / m, b = e - a * m;
    double acc = den[t];
    for (int i = 0; i < B; ++i) {
        if (label[i] != k) continue;
        const CtfRow row = ctf_row(params + (long)i * 8, scale);
        double osc;
        const double c = ctf_at(row, a, b, n, m, &osc);
        acc += c * c;
    }
    den[t] = acc;
}

// One workgroup per class (SCRATCH: the grid strides over the classes): average[k] = Re IDFT( DFT(sum[k]) / (den[k] + lambda) ),
// a frequency whose den + lambda is 0 contributing 0.
template <bool SCRATCH>
__global__ void __launch_bounds__(256) wiener_finish_kernel(const double* __restrict__ sum, const double* __restrict__ den,
                                                             double lambda, int n_classes, int n, int m,
                                                             float* __restrict__ average, double* __restrict__ scratch) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) double lds_ctfcorr[];
    const DftPlanes<SCRATCH> pl(lds_ctfcorr, scratch, n, m);
    const int N = n * m;
    dft_twiddles(pl.wm, pl.wn, n, m);
    for (int k = blockIdx.x; k < n_classes; k += gridDim.x) {
        const double* src = sum + (long)k * N;
        const double* dk = den + (long)k * N;
        double* in = reinterpret_cast<double*>(pl.Q);
        for (int e = threadIdx.x; e < N; e += 256) in[e] = src[e];
        __syncthreads();
        dft_filter_plane(pl.P, pl.Q, pl.wm, pl.wn, n, m,
                         [&](int e, int, int, double re, double im) {
                             const double d = dk[e] + lambda;
                             return d == 0.0 ? make_double2(0.0, 0.0) : make_double2(re / d, im / d);
                         },
                         average + (long)k * N);
    }
}

}  // namespace svae
