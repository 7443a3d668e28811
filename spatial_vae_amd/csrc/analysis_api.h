// The entry points of the analysis headers (include/svae_align.h, svae_ctfcorr.h, svae_frc.h, svae_refine.h, svae_classify.h,
// svae_cluster.h, svae_gmm.h, svae_pca.h, svae_expect.h, svae_eigen.h, svae_neighbours.h) and svae.h's svae_ctf_filter, which takes the
// same LDS / workspace form.  Not a header of its own: api.hip includes it once, at namespace scope, below the kernels and its own fail(), Scope,
// launch_status() and blocks_for().  The rules the entry points share are stated once, here at the top.

namespace {

// ---- planes in LDS, or in a workspace slice per workgroup ----
const size_t kLdsMax = 160 * 1024;  // the LDS of one CU
const int kScratchGroups = 512;     // workgroups of the workspace form (two per CU); each strides over the images or planes
int scratch_groups(int count) { return count < kScratchGroups ? count : kScratchGroups; }
size_t roundup32(size_t v) { return (v + 31) & ~size_t(31); }

// Where one workgroup keeps its doubles.  `fixed` of them stay in LDS in either form; the `planes` stay there too while both
// fit kLdsMax (one workgroup per item), and else move to a slice of the workspace, over which kScratchGroups workgroups stride.
struct PlaneForm {
    bool scratch;      // the workspace form
    size_t lds_bytes;  // dynamic LDS of the launch
    int groups;        // its grid
    size_t slice;      // doubles between two workgroups' slices of the workspace: a multiple of 256 bytes
    double* at(void* ws) const { return scratch ? static_cast<double*>(ws) : nullptr; }  // the kernels' scratch argument
};
PlaneForm plane_form(size_t fixed, size_t planes, int count) {
    const bool scratch = (fixed + planes) * sizeof(double) > kLdsMax;
    return {scratch, (fixed + (scratch ? 0 : planes)) * sizeof(double), scratch ? scratch_groups(count) : count, roundup32(planes)};
}

// Launch the kernel of form `f`, its LDS- or its workspace-form instantiation, with `args`; `first()` launches what comes
// before it in the same profile scope.  More than 64 KiB of dynamic LDS have to be asked for.
template <class First, class K, class... Args>
int launch_form_after(const char* who, First first, K lds_kernel, K ws_kernel, const PlaneForm& f, hipStream_t st, Args... args) {
    K kernel = f.scratch ? ws_kernel : lds_kernel;
    if (f.lds_bytes > 64 * 1024 && hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)f.lds_bytes) != hipSuccess)
        return fail(SVAE_E_LAUNCH, "%s: cannot reserve %zu bytes of LDS", who, f.lds_bytes);
    Scope prof(K_AUGMENT, st);
    first();
    hipLaunchKernelGGL(kernel, dim3(f.groups), dim3(256), f.lds_bytes, st, args...);
    return launch_status(who);
}
template <class K, class... Args>
int launch_form(const char* who, K lds_kernel, K ws_kernel, const PlaneForm& f, hipStream_t st, Args... args) {
    return launch_form_after(who, [] {}, lds_kernel, ws_kernel, f, st, args...);
}

// `ws` must be there, 256-byte aligned and `need` bytes long; 0 or `code`, the message naming what needs it (a printf format)
int check_workspace(const char* who, int code, const void* ws, size_t ws_bytes, size_t need, const char* what, ...) {
    if (ws && ws_bytes >= need && !(reinterpret_cast<uintptr_t>(ws) & 255)) return SVAE_OK;
    char subject[192];
    va_list ap;
    va_start(ap, what);
    vsnprintf(subject, sizeof(subject), what, ap);
    va_end(ap);
    return fail(code, "%s: %s need a workspace of %zu bytes, 256-byte aligned (got %zu)", who, subject, need, ws_bytes);
}

inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }
inline bool bytes_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + qn && b < a + pn;
}

// ---- the plane transforms: ctf_filter (3 planes of n x m doubles), ctfcorr and frc (4) ----
size_t dft_twiddles(int n, int m) { return 2 * ((size_t)n + m); }  // doubles; they stay in LDS in either form
PlaneForm dft_form(int count, int n, int m, int planes = 4) { return plane_form(dft_twiddles(n, m), (size_t)n * m * planes, count); }
size_t dft_workspace_bytes(int count, int n, int m, int planes = 4) {
    if (count < 1 || n < 1 || m < 1) return 0;
    const PlaneForm f = dft_form(count, n, m, planes);
    return f.scratch ? (size_t)f.groups * n * m * planes * sizeof(double) : 0;  // these kernels' slices are not rounded
}

// the plane-size and workspace rules svae_ctf_apply, svae_wiener_finish and the two ring calls share; 0 or the refusal
int dft_check(const char* who, int count, int n, int m, const void* ws, size_t ws_bytes) {
    if (n < 2 || m < 2) return fail(SVAE_E_INVALID, "%s: planes must be at least 2 x 2 (got %d x %d)", who, n, m);
    if (dft_twiddles(n, m) * sizeof(double) > kLdsMax)
        return fail(SVAE_E_INVALID, "%s: %d x %d planes are not supported (n + m must not exceed %zu)", who, n, m,
                    kLdsMax / (2 * sizeof(double)));
    if ((long)count * n * m > 0x7fffffffL) return fail(SVAE_E_INVALID, "%s: %d planes of %d x %d are too many", who, count, n, m);
    if (!dft_form(count, n, m).scratch) return SVAE_OK;
    return check_workspace(who, SVAE_E_INVALID, ws, ws_bytes, dft_workspace_bytes(count, n, m), "%d x %d planes", n, m);
}

// ---- the pose calls: svae_pose_search, svae_pose_classify, svae_pose_expect ----
bool refine_sizes_ok(int B, int rows, int cols, int C, int A, int S) {
    return B >= 1 && rows >= 2 && rows <= 1024 && cols >= 2 && cols <= 1024 && C >= 1 && C <= SVAE_MAX_OUT && A >= 0 && A <= 32 &&
           S >= 0 && S <= 8;
}
// 0, or which size rule fails: 1 = a size outside its range, 2 = a product past 2^31 - 1.  An image has M slots (1..max_M) of
// `slot` output elements each; svae_pose_search has neither (M = max_M = 1, slot = 0).
int pose_sizes(int B, int n_ref, int M, int max_M, int rows, int cols, int C, int A, int S, long slot) {
    if (!refine_sizes_ok(B, rows, cols, C, A, S) || n_ref < 1 || M < 1 || M > max_M) return 1;
    const long plane = (long)rows * cols * C;
    return (B * plane > 0x7fffffffL || n_ref * plane > 0x7fffffffL || (long)B * M * slot > 0x7fffffffL) ? 2 : 0;
}
// the sizes, "too many", step and interp rules of the three calls, in that order; `slots` names what B x M counts; 0 or the refusal
int pose_check(const char* who, int B, int n_ref, int M, int max_M, int rows, int cols, int C, int A, double step, int S, int interp,
               long slot, const char* slots) {
    char m_is[24] = "", m_in[32] = "", or_slots[64] = "";
    if (max_M > 1) {
        snprintf(m_is, sizeof(m_is), "M=%d ", M);
        snprintf(m_in, sizeof(m_in), "M in 1..%d, ", max_M);
        snprintf(or_slots, sizeof(or_slots), ", or %d x %d %s,", B, M, slots);
    }
    const int bad = pose_sizes(B, n_ref, M, max_M, rows, cols, C, A, S, slot);
    if (bad == 1)
        return fail(SVAE_E_INVALID, "%s: bad sizes B=%d n_ref=%d %srows=%d cols=%d C=%d A=%d S=%d (%srows, cols in 2..1024, C in 1..%d, "
                    "A in 0..32, S in 0..8)", who, B, n_ref, m_is, rows, cols, C, A, S, m_in, SVAE_MAX_OUT);
    if (bad == 2)
        return fail(SVAE_E_INVALID, "%s: %d images or %d references of %d x %d x %d%s are too many", who, B, n_ref, rows, cols, C, or_slots);
    if (A > 0 && (!(step > 0.0) || isinf(step))) return fail(SVAE_E_INVALID, "%s: step must be finite and > 0 where A > 0", who);
    if (interp != SVAE_ALIGN_BILINEAR && interp != SVAE_ALIGN_BICUBIC)
        return fail(SVAE_E_INVALID, "%s: unknown interpolation %d", who, interp);
    return SVAE_OK;
}

// one of a pose kernel's four <CUBIC, SCRATCH> instantiations (a function template cannot be handed over: hence the macro)
template <class K>
K pose_kernel(int interp, bool scratch, K cubic_ws, K linear_ws, K cubic_lds, K linear_lds) {
    const bool cubic = interp == SVAE_ALIGN_BICUBIC;
    return scratch ? (cubic ? cubic_ws : linear_ws) : (cubic ? cubic_lds : linear_lds);
}
#define POSE_KERNEL(kernel, interp, scratch) \
    pose_kernel(interp, scratch, kernel<true, true>, kernel<false, true>, kernel<true, false>, kernel<false, false>)

// What each pose kernel moves to the workspace above the limit: the resampled plane and the image's score volume (search), the
// M running maxima (classify), or the plane's coverage and the M log-weight volumes (expect).  The block sums stay in LDS.
size_t pose_volume(int A, int S) { return (size_t)(2 * A + 1) * (2 * S + 1) * (2 * S + 1); }
PlaneForm refine_form(int B, int rows, int cols, int C, int A, int S) {
    return plane_form(8, (size_t)rows * cols * C + pose_volume(A, S), B);
}
PlaneForm classify_form(int B, int M, int rows, int cols, int C) { return plane_form(8, (size_t)rows * cols * C + (size_t)M, B); }
PlaneForm expect_form(int B, int M, int rows, int cols, int C, int A, int S) {
    return plane_form(kExpectFixed, (size_t)rows * cols * C + (size_t)rows * cols + (size_t)M * pose_volume(A, S), B);
}
// the workspace of svae_pose_classify and svae_pose_expect, in bytes: the references' norms, then the slices
size_t norms_and_slices_bytes(int n_ref, const PlaneForm& f) {
    return (roundup32((size_t)n_ref) + (f.scratch ? (size_t)f.groups * f.slice : 0)) * sizeof(double);
}

// ---- the statistics of the content latents: k-means, the mixture, the principal axes ----
bool latent_sizes_ok(int64_t N, int32_t D, int32_t k) {
    return D >= 1 && D <= kKmeansMaxD && k >= 1 && k <= kKmeansMaxK && N >= k && N <= 0x7fffffffLL;
}
// f(std::integral_constant<int, DMAX>) for the kernels' DMAX of D coordinates in registers
template <class F>
void by_dim(int D, F f) {
    if (D <= 4) f(std::integral_constant<int, 4>{});
    else if (D <= 16) f(std::integral_constant<int, 16>{});
    else f(std::integral_constant<int, 64>{});
}
// the geometry and workspace rules the k-means and mixture calls share; 0 or the refusal
int latent_check(const char* who, int64_t N, int32_t D, int32_t k, size_t (*ws_words)(long, int, int), const void* ws, size_t ws_bytes) {
    if (!latent_sizes_ok(N, D, k))
        return fail(SVAE_E_INVALID, "%s: bad sizes N=%lld D=%d k=%d (1 <= D <= %d, 1 <= k <= %d, k <= N < 2^31)", who, (long long)N, D, k,
                    kKmeansMaxD, kKmeansMaxK);
    return check_workspace(who, SVAE_E_WORKSPACE, ws, ws_bytes, ws_words((long)N, D, k) * 8, "N=%lld points with D=%d, k=%d", (long long)N,
                           D, k);
}

}  // namespace

extern "C" {

// ---- alignment into the canonical frame and class sums (include/svae_align.h) ----
int svae_align_images(const float* y, const float* theta, const float* dx, int32_t B, int32_t rows, int32_t cols, int32_t C,
                      int32_t interp, float* aligned, uint8_t* cover, svae_stream_t stream) {
    if (B < 1 || rows < 2 || cols < 2 || C < 1 || C > SVAE_MAX_OUT || (long)B * rows * cols * C > 0x7fffffffL)
        return fail(SVAE_E_INVALID, "svae_align_images: bad sizes B=%d rows=%d cols=%d C=%d", B, rows, cols, C);
    if (interp != SVAE_ALIGN_BILINEAR && interp != SVAE_ALIGN_BICUBIC)
        return fail(SVAE_E_INVALID, "svae_align_images: unknown interpolation %d", interp);
    const long total = (long)B * rows * cols * C;
    if (!y || !aligned || (y < aligned + total && aligned < y + total))
        return fail(SVAE_E_INVALID, "svae_align_images: y and aligned must be two buffers that do not overlap");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    const AlignGeo g{B, rows, cols, C};
    if (interp == SVAE_ALIGN_BICUBIC)
        hipLaunchKernelGGL(align_images_kernel<true>, dim3(blocks_for(total)), dim3(256), 0, st, y, theta, dx, aligned, cover, g);
    else
        hipLaunchKernelGGL(align_images_kernel<false>, dim3(blocks_for(total)), dim3(256), 0, st, y, theta, dx, aligned, cover, g);
    return launch_status("svae_align_images");
}

int svae_class_sums_update(const float* aligned, const uint8_t* cover, const int32_t* label, int32_t B, int32_t N, int32_t C,
                           int32_t n_classes, double* sum, double* count, svae_stream_t stream) {
    if (B < 1 || N < 1 || C < 1 || C > SVAE_MAX_OUT || n_classes < 1 || n_classes > 4096 || (long)B * N * C > 0x7fffffffL ||
        (long)n_classes * N * C > 0x7fffffffL)
        return fail(SVAE_E_INVALID, "svae_class_sums_update: bad sizes B=%d N=%d C=%d n_classes=%d", B, N, C, n_classes);
    if (!aligned || !label || !sum || !count) return fail(SVAE_E_INVALID, "svae_class_sums_update: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(class_sums_update_kernel, dim3(blocks_for((long)n_classes * N)), dim3(256), 0, st, aligned, cover, label, B, N,
                       C, n_classes, sum, count);
    return launch_status("svae_class_sums_update");
}

// ---- the CTF filter bank (include/svae.h) ----
size_t svae_ctf_filter_workspace_bytes(int32_t count, int32_t n, int32_t m) { return dft_workspace_bytes(count, n, m, 3); }

int svae_ctf_filter(const double* params, float* filters, int32_t count, int32_t n, int32_t m, double scale, void* ws,
                    size_t ws_bytes, svae_stream_t stream) {
    if (!params || !filters || count < 1 || n < 1 || m < 1) return fail(SVAE_E_INVALID, "svae_ctf_filter: bad arguments");
    if (dft_twiddles(n, m) * sizeof(double) > kLdsMax)
        return fail(SVAE_E_INVALID, "svae_ctf_filter: %d x %d filters are not supported (n + m must not exceed %zu)", n, m,
                    kLdsMax / (2 * sizeof(double)));
    if (!(scale > 0.0)) return fail(SVAE_E_INVALID, "svae_ctf_filter: scale must be positive");
    const PlaneForm f = dft_form(count, n, m, 3);
    if (f.scratch)
        if (const int rc = check_workspace("svae_ctf_filter", SVAE_E_WORKSPACE, ws, ws_bytes, dft_workspace_bytes(count, n, m, 3),
                                           "the scratch planes of %d x %d filters", n, m))
            return rc;
    return launch_form("svae_ctf_filter", ctf_filter_kernel<false>, ctf_filter_kernel<true>, f, static_cast<hipStream_t>(stream), params,
                       filters, count, n, m, scale, f.at(ws));
}

// ---- CTF correction in Fourier space (include/svae_ctfcorr.h) ----
size_t svae_ctf_apply_workspace_bytes(int32_t B, int32_t n, int32_t m) { return dft_workspace_bytes(B, n, m); }

int svae_ctf_apply(const float* y, const double* params, int32_t B, int32_t n, int32_t m, double scale, int32_t mode, float* out,
                   void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (B < 1) return fail(SVAE_E_INVALID, "svae_ctf_apply: B must be positive (got %d)", B);
    if (mode != SVAE_CTF_FLIP && mode != SVAE_CTF_MULTIPLY) return fail(SVAE_E_INVALID, "svae_ctf_apply: unknown mode %d", mode);
    if (!(scale > 0.0)) return fail(SVAE_E_INVALID, "svae_ctf_apply: scale must be positive");
    if (const int rc = dft_check("svae_ctf_apply", B, n, m, ws, ws_bytes)) return rc;
    const long total = (long)B * n * m;
    if (!y || !out || !params) return fail(SVAE_E_INVALID, "svae_ctf_apply: null y, out or params");
    if (y < out + total && out < y + total)
        return fail(SVAE_E_INVALID, "svae_ctf_apply: y and out must be two buffers that do not overlap");
    const PlaneForm f = dft_form(B, n, m);
    return launch_form("svae_ctf_apply", ctf_apply_kernel<false>, ctf_apply_kernel<true>, f, static_cast<hipStream_t>(stream), y, params,
                       (int)B, (int)n, (int)m, scale, (int)mode, out, f.at(ws));
}

int svae_ctf_power_update(const double* params, const int32_t* label, int32_t B, int32_t n, int32_t m, double scale,
                          int32_t n_classes, double* den, svae_stream_t stream) {
    if (B < 1 || n < 2 || m < 2 || n_classes < 1 || n_classes > 4096 || (long)n * m > 0x7fffffffL ||
        (long)n_classes * n * m > 0x7fffffffL)
        return fail(SVAE_E_INVALID, "svae_ctf_power_update: bad sizes B=%d n=%d m=%d n_classes=%d", B, n, m, n_classes);
    if (!(scale > 0.0)) return fail(SVAE_E_INVALID, "svae_ctf_power_update: scale must be positive");
    if (!params || !label || !den) return fail(SVAE_E_INVALID, "svae_ctf_power_update: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(ctf_power_update_kernel, dim3(blocks_for((long)n_classes * n * m)), dim3(256), 0, st, params, label, B, n, m,
                       scale, n_classes, den);
    return launch_status("svae_ctf_power_update");
}

size_t svae_wiener_finish_workspace_bytes(int32_t n_classes, int32_t n, int32_t m) { return dft_workspace_bytes(n_classes, n, m); }

int svae_wiener_finish(const double* sum, const double* den, double lambda, int32_t n_classes, int32_t n, int32_t m, float* average,
                       void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (n_classes < 1 || n_classes > 4096)
        return fail(SVAE_E_INVALID, "svae_wiener_finish: n_classes %d outside 1..4096", n_classes);
    if (!(lambda >= 0.0) || isinf(lambda)) return fail(SVAE_E_INVALID, "svae_wiener_finish: lambda must be finite and >= 0");
    if (const int rc = dft_check("svae_wiener_finish", n_classes, n, m, ws, ws_bytes)) return rc;
    if (!sum || !den || !average) return fail(SVAE_E_INVALID, "svae_wiener_finish: null sum, den or average");
    const PlaneForm f = dft_form(n_classes, n, m);
    return launch_form("svae_wiener_finish", wiener_finish_kernel<false>, wiener_finish_kernel<true>, f, static_cast<hipStream_t>(stream),
                       sum, den, lambda, (int)n_classes, (int)n, (int)m, average, f.at(ws));
}

// ---- Fourier ring correlation (include/svae_frc.h) ----
namespace {
// the size rules the two ring calls share, then ctfcorr's plane and workspace rules; 0 or the refusal
int frc_check(const char* who, int planes, int n, int m, const void* ws, size_t ws_bytes) {
    if (n < 2 || m < 2 || n > 1024 || m > 1024) return fail(SVAE_E_INVALID, "%s: n and m must be in 2..1024 (got %d x %d)", who, n, m);
    if (planes < 1) return fail(SVAE_E_INVALID, "%s: planes must be positive (got %d)", who, planes);
    return dft_check(who, planes, n, m, ws, ws_bytes);
}
}  // namespace

size_t svae_frc_workspace_bytes(int32_t planes, int32_t n, int32_t m) { return dft_workspace_bytes(planes, n, m); }

int svae_frc(const double* a, const double* b, int32_t planes, int32_t n, int32_t m, double mask_radius, double mask_edge,
             double* sums, double* frc, int32_t* ring_count, void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = frc_check("svae_frc", planes, n, m, ws, ws_bytes)) return rc;
    if (!(mask_radius >= 0.0) || isinf(mask_radius)) return fail(SVAE_E_INVALID, "svae_frc: mask_radius must be finite and >= 0");
    if (mask_radius > 0.0 && (!(mask_edge > 0.0) || isinf(mask_edge)))
        return fail(SVAE_E_INVALID, "svae_frc: mask_edge must be finite and > 0 where mask_radius > 0");
    if (!a || !b || !sums || !frc || !ring_count) return fail(SVAE_E_INVALID, "svae_frc: null a, b, sums, frc or ring_count");
    const size_t R = (size_t)((n < m ? n : m) / 2 + 1);
    const size_t in_bytes = (size_t)planes * n * m * sizeof(double);
    const void* outs[3] = {sums, frc, ring_count};
    const size_t out_bytes[3] = {(size_t)planes * R * 3 * sizeof(double), (size_t)planes * R * sizeof(double), R * sizeof(int32_t)};
    for (int i = 0; i < 3; ++i)
        if (bytes_overlap(a, in_bytes, outs[i], out_bytes[i]) || bytes_overlap(b, in_bytes, outs[i], out_bytes[i]))
            return fail(SVAE_E_INVALID, "svae_frc: a and b must not overlap sums, frc or ring_count");
    const PlaneForm f = dft_form(planes, n, m);
    return launch_form("svae_frc", frc_kernel<false>, frc_kernel<true>, f, static_cast<hipStream_t>(stream), a, b, (int)planes, (int)n,
                       (int)m, mask_radius, mask_edge, sums, frc, reinterpret_cast<int*>(ring_count), f.at(ws));
}

size_t svae_frc_filter_workspace_bytes(int32_t planes, int32_t n, int32_t m) { return dft_workspace_bytes(planes, n, m); }

int svae_frc_filter(const double* x, const double* weight, int32_t planes, int32_t n, int32_t m, float* out, void* ws,
                    size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = frc_check("svae_frc_filter", planes, n, m, ws, ws_bytes)) return rc;
    if (!x || !weight || !out) return fail(SVAE_E_INVALID, "svae_frc_filter: null x, weight or out");
    const size_t R = (size_t)((n < m ? n : m) / 2 + 1);
    const size_t total = (size_t)planes * n * m;
    if (bytes_overlap(x, total * sizeof(double), out, total * sizeof(float)) ||
        bytes_overlap(weight, (size_t)planes * R * sizeof(double), out, total * sizeof(float)))
        return fail(SVAE_E_INVALID, "svae_frc_filter: x and weight must not overlap out");
    const PlaneForm f = dft_form(planes, n, m);
    return launch_form("svae_frc_filter", frc_filter_kernel<false>, frc_filter_kernel<true>, f, static_cast<hipStream_t>(stream), x, weight,
                       (int)planes, (int)n, (int)m, out, f.at(ws));
}

// ---- reference-based pose search (include/svae_refine.h) ----
size_t svae_pose_search_workspace_bytes(int32_t B, int32_t rows, int32_t cols, int32_t C, int32_t A, int32_t S) {
    if (!refine_sizes_ok(B, rows, cols, C, A, S)) return 0;
    const PlaneForm f = refine_form(B, rows, cols, C, A, S);
    return f.scratch ? (size_t)f.groups * f.slice * sizeof(double) : 0;
}

int svae_pose_search(const float* y, const double* ref, const double* weight, const int32_t* ref_index, const float* pose_in,
                     int32_t B, int32_t n_ref, int32_t rows, int32_t cols, int32_t C, int32_t A, double step, int32_t S,
                     int32_t interp, float* pose_out, double* score, int32_t* offset, double* scores, void* ws, size_t ws_bytes,
                     svae_stream_t stream) {
    if (const int rc = pose_check("svae_pose_search", B, n_ref, 1, 1, rows, cols, C, A, step, S, interp, 0, nullptr)) return rc;
    if (!y || !ref || !ref_index || !pose_in || !pose_out || !score || !offset)
        return fail(SVAE_E_INVALID, "svae_pose_search: null y, ref, ref_index, pose_in, pose_out, score or offset");
    const PlaneForm f = refine_form(B, rows, cols, C, A, S);
    if (f.scratch)
        if (const int rc = check_workspace("svae_pose_search", SVAE_E_INVALID, ws, ws_bytes,
                                           svae_pose_search_workspace_bytes(B, rows, cols, C, A, S),
                                           "%d x %d x %d images with A=%d, S=%d", rows, cols, C, A, S))
            return rc;
    const PoseGeo g{B, n_ref, 1, rows, cols, C, A, S, A > 0 ? step : 0.0, 0.0};
    return launch_form("svae_pose_search", POSE_KERNEL(pose_search_kernel, interp, false), POSE_KERNEL(pose_search_kernel, interp, true), f,
                       static_cast<hipStream_t>(stream), y, ref, weight, reinterpret_cast<const int*>(ref_index), pose_in, g, pose_out, score,
                       reinterpret_cast<int*>(offset), scores, f.at(ws), (long)f.slice);
}

// ---- multi-reference alignment (include/svae_classify.h) ----
size_t svae_pose_classify_workspace_bytes(int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C) {
    if (pose_sizes(B, n_ref, M, 4096, rows, cols, C, 0, 0, 1)) return 0;
    return norms_and_slices_bytes(n_ref, classify_form(B, M, rows, cols, C));
}

int svae_pose_classify(const float* y, const double* ref, const double* weight, const int32_t* cand, const float* pose_in,
                       int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A, double step,
                       int32_t S, int32_t interp, int32_t* choice, int32_t* ref_chosen, double* cand_score, double* margin,
                       void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = pose_check("svae_pose_classify", B, n_ref, M, 4096, rows, cols, C, A, step, S, interp, 1, "candidates")) return rc;
    if (!y || !ref || !cand || !pose_in || !choice || !ref_chosen || !cand_score)
        return fail(SVAE_E_INVALID, "svae_pose_classify: null y, ref, cand, pose_in, choice, ref_chosen or cand_score");
    const PlaneForm f = classify_form(B, M, rows, cols, C);
    if (const int rc = check_workspace("svae_pose_classify", SVAE_E_INVALID, ws, ws_bytes, norms_and_slices_bytes(n_ref, f),
                                       "%d references and %d x %d x %d images with M=%d", n_ref, rows, cols, C, M))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PoseGeo g{B, n_ref, M, rows, cols, C, A, S, A > 0 ? step : 0.0, 0.0};
    double* norms = static_cast<double*>(ws);
    const auto first = [&] {
        hipLaunchKernelGGL(pose_norms_kernel<true>, dim3(n_ref), dim3(256), 0, st, ref, weight, rows * cols * C, C, norms);
    };
    return launch_form_after("svae_pose_classify", first, POSE_KERNEL(pose_classify_kernel, interp, false),
                             POSE_KERNEL(pose_classify_kernel, interp, true), f, st, y, ref, weight, reinterpret_cast<const int*>(cand),
                             pose_in, g, static_cast<const double*>(norms), reinterpret_cast<int*>(choice),
                             reinterpret_cast<int*>(ref_chosen), cand_score, margin, f.at(norms + roundup32((size_t)n_ref)), (long)f.slice);
}

// ---- k-means over the content latents (include/svae_cluster.h) ----
size_t svae_kmeans_workspace_bytes(int64_t N, int32_t D, int32_t k) {
    return latent_sizes_ok(N, D, k) ? kmeans_ws_words((long)N, D, k) * 8 : 0;
}

int svae_kmeans_seed(const float* x, int64_t N, int32_t D, int32_t k, const double* u, double* centres, int32_t* seed_index,
                     void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (!x || !u || !centres || !seed_index) return fail(SVAE_E_INVALID, "svae_kmeans_seed: null x, u, centres or seed_index");
    if (misaligned8(u) || misaligned8(centres)) return fail(SVAE_E_INVALID, "svae_kmeans_seed: u and centres must be 8-byte aligned");
    if (const int rc = latent_check("svae_kmeans_seed", N, D, k, kmeans_ws_words, ws, ws_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LatentChunks ch((long)N);
    const KmeansWs w = kmeans_ws(ws, (long)N, D, k);
    Scope prof(K_AUGMENT, st);
    for (int j = 0; j < k; ++j) {
        if (j > 0) {
            const int first = j == 1 ? 1 : 0;
            by_dim(D, [&](auto d) {
                hipLaunchKernelGGL(kmeans_seed_dist_kernel<decltype(d)::value>, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, ch.P, centres,
                                   j - 1, first, w);
            });
        }
        hipLaunchKernelGGL(kmeans_seed_pick_kernel, dim3(1), dim3(256), 0, st, x, (long)N, D, ch.P, ch.n, j, u, centres, seed_index, w);
    }
    return launch_status("svae_kmeans_seed");
}

int svae_kmeans_step(const float* x, int64_t N, int32_t D, int32_t k, int32_t update, double* centres, int32_t* label,
                     int64_t* members, svae_kmeans_record* rec, void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (!x || !centres || !label || !members || !rec) return fail(SVAE_E_INVALID, "svae_kmeans_step: null x, centres, label, members or rec");
    if (misaligned8(centres) || misaligned8(members) || misaligned8(rec))
        return fail(SVAE_E_INVALID, "svae_kmeans_step: centres, members and rec must be 8-byte aligned");
    if (const int rc = latent_check("svae_kmeans_step", N, D, k, kmeans_ws_words, ws, ws_bytes)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LatentChunks ch((long)N);
    const KmeansWs w = kmeans_ws(ws, (long)N, D, k);
    const int up = update ? 1 : 0;
    const long long* iterations = reinterpret_cast<const long long*>(&rec->iterations);
    long long* mem = reinterpret_cast<long long*>(members);
    Scope prof(K_AUGMENT, st);
    by_dim(D, [&](auto d) {
        hipLaunchKernelGGL(kmeans_assign_kernel<decltype(d)::value>, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P, centres, label,
                           iterations, w);
    });
    hipLaunchKernelGGL(kmeans_accumulate_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P, up, label, w);
    hipLaunchKernelGGL(kmeans_tail_kernel, dim3(blocks_for(up ? (long)k * D : (long)k)), dim3(256), 0, st, D, k, ch.n, up, centres, mem,
                       rec, w);
    return launch_status("svae_kmeans_step");
}

// ---- the Gaussian mixture over the content latents (include/svae_gmm.h) ----
namespace {
// the pointer, range, geometry and workspace rules the two mixture calls share; 0 or the refusal
int gmm_check(const char* who, const void* x, int64_t N, int32_t D, int32_t k, const void* labels, double reg, double tol,
              const void* weight, const void* mean, const void* var, const void* resp, const void* loglik_point, const void* rec,
              const void* ws, size_t ws_bytes) {
    if (!x || !labels || !weight || !mean || !var || !resp || !rec)
        return fail(SVAE_E_INVALID, "%s: null x, labels, weight, mean, var, resp or rec", who);
    if (misaligned8(weight) || misaligned8(mean) || misaligned8(var) || misaligned8(resp) || misaligned8(rec) || misaligned8(loglik_point))
        return fail(SVAE_E_INVALID, "%s: weight, mean, var, resp, loglik_point and rec must be 8-byte aligned", who);
    if (!(reg > 0.0) || !std::isfinite(reg)) return fail(SVAE_E_INVALID, "%s: reg = %g must be a finite number > 0", who, reg);
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(SVAE_E_INVALID, "%s: tol = %g must be a finite number >= 0", who, tol);
    return latent_check(who, N, D, k, gmm_ws_words, ws, ws_bytes);
}
}  // namespace

size_t svae_gmm_workspace_bytes(int64_t N, int32_t D, int32_t k) { return latent_sizes_ok(N, D, k) ? gmm_ws_words((long)N, D, k) * 8 : 0; }

int svae_gmm_init(const float* x, int64_t N, int32_t D, int32_t k, const int32_t* label_in, double reg, double* weight, double* mean,
                  double* var, double* resp, svae_gmm_record* rec, void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = gmm_check("svae_gmm_init", x, N, D, k, label_in, reg, 0.0, weight, mean, var, resp, nullptr, rec, ws, ws_bytes))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LatentChunks ch((long)N);
    const GmmWs w = gmm_ws(ws, (long)N, D, k);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(gmm_onehot_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P, reinterpret_cast<const int*>(label_in), resp,
                       w);
    hipLaunchKernelGGL(gmm_accumulate_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P, static_cast<const double*>(mean),
                       static_cast<const double*>(resp), static_cast<const long long*>(nullptr), w);
    hipLaunchKernelGGL(gmm_tail_kernel, dim3(blocks_for((long)k * (D + 1))), dim3(256), 0, st, D, k, ch.n, (int)kGmmInit, reg, 0.0, weight,
                       mean, var, rec, w);
    return launch_status("svae_gmm_init");
}

int svae_gmm_step(const float* x, int64_t N, int32_t D, int32_t k, int32_t update, double reg, double tol, double* weight,
                  double* mean, double* var, double* resp, int32_t* label, double* loglik_point, svae_gmm_record* rec, void* ws,
                  size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = gmm_check("svae_gmm_step", x, N, D, k, label, reg, tol, weight, mean, var, resp, loglik_point, rec, ws, ws_bytes))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LatentChunks ch((long)N);
    const GmmWs w = gmm_ws(ws, (long)N, D, k);
    int* lab = reinterpret_cast<int*>(label);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(gmm_prologue_kernel, dim3(blocks_for((long)k)), dim3(256), 0, st, D, k, static_cast<const double*>(weight),
                       static_cast<const double*>(var), static_cast<const svae_gmm_record*>(rec), w);
    by_dim(D, [&](auto d) {
        hipLaunchKernelGGL(gmm_e_kernel<decltype(d)::value>, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P,
                           static_cast<const double*>(mean), resp, lab, loglik_point, w);
    });
    if (update)
        hipLaunchKernelGGL(gmm_accumulate_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, k, ch.P, static_cast<const double*>(mean),
                           static_cast<const double*>(resp), static_cast<const long long*>(w.snap), w);
    hipLaunchKernelGGL(gmm_tail_kernel, dim3(update ? blocks_for((long)k * (D + 1)) : 1), dim3(256), 0, st, D, k, ch.n,
                       update ? (int)kGmmStep : (int)kGmmLabelOnly, reg, tol, weight, mean, var, rec, w);
    return launch_status("svae_gmm_step");
}

// ---- principal axes of the content latents (include/svae_pca.h) ----
size_t svae_pca_workspace_bytes(int64_t N, int32_t D, int32_t G) { return pca_sizes_ok(N, D, G) ? pca_ws_words((long)N, D, G) * 8 : 0; }

int svae_pca_moments(const float* x, int64_t N, int32_t D, int32_t G, const int32_t* group, int64_t* count, double* mean,
                     double* cov, void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (!x || !count || !mean || !cov) return fail(SVAE_E_INVALID, "svae_pca_moments: null x, count, mean or cov");
    if (misaligned8(count) || misaligned8(mean) || misaligned8(cov))
        return fail(SVAE_E_INVALID, "svae_pca_moments: count, mean and cov must be 8-byte aligned");
    if (!pca_sizes_ok(N, D, G))
        return fail(SVAE_E_INVALID, "svae_pca_moments: bad sizes N=%lld D=%d G=%d (1 <= D <= %d, 1 <= G <= %d, G D (D + 1) / 2 <= %d, "
                    "1 <= N < 2^31)", (long long)N, D, G, kKmeansMaxD, kPcaMaxG, kPcaMaxPartials);
    if (!group && G != 1) return fail(SVAE_E_INVALID, "svae_pca_moments: a null group needs G == 1 (got %d)", G);
    if (const int rc = check_workspace("svae_pca_moments", SVAE_E_WORKSPACE, ws, ws_bytes, pca_ws_words((long)N, D, G) * 8,
                                       "N=%lld points with D=%d, G=%d", (long long)N, D, G))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const LatentChunks ch((long)N);
    const PcaWs w = pca_ws(ws, (long)N, D, G);
    long long* cnt = reinterpret_cast<long long*>(count);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(pca_sums_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, G, ch.P, reinterpret_cast<const int*>(group), w);
    hipLaunchKernelGGL(pca_mean_kernel, dim3(blocks_for((long)G * (D + 1))), dim3(256), 0, st, D, G, ch.n, cnt, mean, w);
    hipLaunchKernelGGL(pca_products_kernel, dim3(ch.n), dim3(256), 0, st, x, (long)N, D, G, ch.P, static_cast<const double*>(mean), w);
    hipLaunchKernelGGL(pca_cov_kernel, dim3(blocks_for((long)G * (D * (D + 1) / 2))), dim3(256), 0, st, D, G, ch.n,
                       static_cast<const long long*>(cnt), cov, w);
    return launch_status("svae_pca_moments");
}

int svae_pca_eigen(const double* cov, int32_t D, int32_t G, double* eigenvalues, double* components, int32_t* sweeps,
                   double* off_norm, svae_stream_t stream) {
    if (!cov || !eigenvalues || !components || !sweeps || !off_norm)
        return fail(SVAE_E_INVALID, "svae_pca_eigen: null cov, eigenvalues, components, sweeps or off_norm");
    if (misaligned8(cov) || misaligned8(eigenvalues) || misaligned8(components) || misaligned8(off_norm))
        return fail(SVAE_E_INVALID, "svae_pca_eigen: cov, eigenvalues, components and off_norm must be 8-byte aligned");
    if (!pca_sizes_ok(1, D, G))
        return fail(SVAE_E_INVALID, "svae_pca_eigen: bad sizes D=%d G=%d (1 <= D <= %d, 1 <= G <= %d, G D (D + 1) / 2 <= %d)", D, G,
                    kKmeansMaxD, kPcaMaxG, kPcaMaxPartials);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(pca_eigen_kernel, dim3(G), dim3(256), 0, st, cov, D, eigenvalues, components, reinterpret_cast<int*>(sweeps), off_norm);
    return launch_status("svae_pca_eigen");
}

int svae_pca_project(const float* x, int64_t N, int32_t D, int32_t G, int32_t P, const int32_t* group, const int64_t* count,
                     const double* mean, const double* components, double* proj, svae_stream_t stream) {
    if (!x || !count || !mean || !components || !proj) return fail(SVAE_E_INVALID, "svae_pca_project: null x, count, mean, components or proj");
    if (misaligned8(count) || misaligned8(mean) || misaligned8(components) || misaligned8(proj))
        return fail(SVAE_E_INVALID, "svae_pca_project: count, mean, components and proj must be 8-byte aligned");
    if (!pca_sizes_ok(N, D, G))
        return fail(SVAE_E_INVALID, "svae_pca_project: bad sizes N=%lld D=%d G=%d (1 <= D <= %d, 1 <= G <= %d, G D (D + 1) / 2 <= %d, "
                    "1 <= N < 2^31)", (long long)N, D, G, kKmeansMaxD, kPcaMaxG, kPcaMaxPartials);
    if (P < 1 || P > D) return fail(SVAE_E_INVALID, "svae_pca_project: P = %d must be in 1..D = %d", P, D);
    if (!group && G != 1) return fail(SVAE_E_INVALID, "svae_pca_project: a null group needs G == 1 (got %d)", G);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(pca_project_kernel, dim3(blocks_for((long)N * P)), dim3(256), 0, st, x, (long)N, D, G, P,
                       reinterpret_cast<const int*>(group), reinterpret_cast<const long long*>(count), mean, components, proj);
    return launch_status("svae_pca_project");
}

// ---- maximum-likelihood class averages (include/svae_expect.h) ----
size_t svae_pose_expect_workspace_bytes(int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A,
                                        int32_t S) {
    if (pose_sizes(B, n_ref, M, kExpectMaxSlots, rows, cols, C, A, S, (long)rows * cols * C)) return 0;
    return norms_and_slices_bytes(n_ref, expect_form(B, M, rows, cols, C, A, S));
}

int svae_pose_expect(const float* y, const double* ref, const double* weight, const double* log_prior, const int32_t* cand,
                     const float* pose_in, int32_t B, int32_t n_ref, int32_t M, int32_t rows, int32_t cols, int32_t C, int32_t A,
                     double step, int32_t S, int32_t interp, double inv_sigma2, double* contrib, double* cover_w,
                     double* class_post, double* log_evidence, int32_t* best, void* ws, size_t ws_bytes, svae_stream_t stream) {
    if (const int rc = pose_check("svae_pose_expect", B, n_ref, M, kExpectMaxSlots, rows, cols, C, A, step, S, interp,
                                  (long)rows * cols * C, "contribution rows"))
        return rc;
    if (!(inv_sigma2 >= 0.0) || !std::isfinite(inv_sigma2))
        return fail(SVAE_E_INVALID, "svae_pose_expect: inv_sigma2 = %g must be a finite number >= 0", inv_sigma2);
    if (!y || !ref || !cand || !pose_in || !contrib || !cover_w || !class_post || !log_evidence || !best)
        return fail(SVAE_E_INVALID, "svae_pose_expect: null y, ref, cand, pose_in, contrib, cover_w, class_post, log_evidence or best");
    const PlaneForm f = expect_form(B, M, rows, cols, C, A, S);
    if (const int rc = check_workspace("svae_pose_expect", SVAE_E_INVALID, ws, ws_bytes, norms_and_slices_bytes(n_ref, f),
                                       "%d references and %d x %d x %d images with M=%d, A=%d, S=%d", n_ref, rows, cols, C, M, A, S))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PoseGeo g{B, n_ref, M, rows, cols, C, A, S, A > 0 ? step : 0.0, inv_sigma2};
    double* hn = static_cast<double*>(ws);
    const auto first = [&] {
        hipLaunchKernelGGL(pose_norms_kernel<false>, dim3(n_ref), dim3(256), 0, st, ref, weight, rows * cols * C, C, hn);
    };
    return launch_form_after("svae_pose_expect", first, POSE_KERNEL(pose_expect_kernel, interp, false),
                             POSE_KERNEL(pose_expect_kernel, interp, true), f, st, y, ref, weight, log_prior,
                             reinterpret_cast<const int*>(cand), pose_in, g, static_cast<const double*>(hn), contrib, cover_w, class_post,
                             log_evidence, reinterpret_cast<int*>(best), f.at(hn + roundup32((size_t)n_ref)), (long)f.slice);
}

int svae_expect_sums_update(const double* contrib, const double* cover_w, const int32_t* cand, const int32_t* target, int32_t B,
                            int32_t M, int32_t N, int32_t C, int32_t n_ref, int32_t n_classes, double* sum, double* count,
                            svae_stream_t stream) {
    if (B < 1 || N < 1 || C < 1 || C > SVAE_MAX_OUT || n_classes < 1 || n_classes > 4096 || n_ref < 1 || M < 1 || M > kExpectMaxSlots ||
        (long)B * N * C > 0x7fffffffL || (long)n_classes * N * C > 0x7fffffffL || (long)B * M * N * C > 0x7fffffffL)
        return fail(SVAE_E_INVALID, "svae_expect_sums_update: bad sizes B=%d M=%d N=%d C=%d n_ref=%d n_classes=%d (M in 1..%d)", B, M, N, C,
                    n_ref, n_classes, kExpectMaxSlots);
    if (!contrib || !cover_w || !cand || !sum || !count) return fail(SVAE_E_INVALID, "svae_expect_sums_update: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(expect_sums_update_kernel, dim3(blocks_for((long)n_classes * N)), dim3(256), 0, st, contrib, cover_w,
                       reinterpret_cast<const int*>(cand), reinterpret_cast<const int*>(target), B, M, N, C, n_ref, n_classes, sum, count);
    return launch_status("svae_expect_sums_update");
}

// ---- per-class eigenimages of aligned images (include/svae_eigen.h) ----
namespace {
// the size rules the calls on a basis share; 0 or the refusal
int eig_basis_check(const char* who, int32_t K, int64_t D, int32_t R) {
    if (K < 1 || K > kEigMaxK || R < 1 || R > kEigMaxR || D < 1 || D > kEigMaxBasis || (int64_t)K * D * R > kEigMaxBasis)
        return fail(SVAE_E_INVALID, "%s: bad sizes K=%d D=%lld R=%d (1 <= K <= %d, 1 <= R <= %d, 1 <= D, K D R <= 2^28)", who, K,
                    (long long)D, R, kEigMaxK, kEigMaxR);
    return SVAE_OK;
}
// the rules svae_eig_project and svae_eig_accumulate share: the sizes, then the images' pointers; 0 or the refusal
int eig_images_check(const char* who, const void* aligned, const void* label, const void* mean, int32_t B, int32_t N, int32_t C,
                     int32_t K, int32_t R) {
    if (B < 1 || N < 1 || C < 1 || C > SVAE_MAX_OUT || (int64_t)B * N * C > 0x7fffffffLL)
        return fail(SVAE_E_INVALID, "%s: bad sizes B=%d N=%d C=%d (C in 1..%d, B N C < 2^31)", who, B, N, C, SVAE_MAX_OUT);
    if (const int rc = eig_basis_check(who, K, (int64_t)N * C, R)) return rc;
    if (!aligned || !label || !mean) return fail(SVAE_E_INVALID, "%s: null aligned, label or mean", who);
    if (misaligned8(mean)) return fail(SVAE_E_INVALID, "%s: mean must be 8-byte aligned", who);
    return SVAE_OK;
}
// 0, or the refusal where the output `out` overlaps one of the inputs
struct EigSpan {
    const void* p;
    size_t bytes;
};
int eig_overlap_check(const char* who, const char* what, const void* out, size_t out_bytes, std::initializer_list<EigSpan> inputs) {
    for (const EigSpan& in : inputs)
        if (in.p && bytes_overlap(in.p, in.bytes, out, out_bytes)) return fail(SVAE_E_INVALID, "%s: %s overlaps an input of the call", who, what);
    return SVAE_OK;
}
}  // namespace

int svae_eig_project(const float* aligned, const uint8_t* cover, const int32_t* label, const double* mean, const double* Q,
                     int32_t B, int32_t N, int32_t C, int32_t K, int32_t R, double* T, svae_stream_t stream) {
    const char* who = "svae_eig_project";
    if (const int rc = eig_images_check(who, aligned, label, mean, B, N, C, K, R)) return rc;
    if (!Q || !T) return fail(SVAE_E_INVALID, "%s: null Q or T", who);
    if (misaligned8(Q) || misaligned8(T)) return fail(SVAE_E_INVALID, "%s: Q and T must be 8-byte aligned", who);
    const size_t D = (size_t)N * C;
    const std::initializer_list<EigSpan> inputs = {{aligned, (size_t)B * D * 4}, {cover, (size_t)B * N}, {label, (size_t)B * 4},
                                                   {mean, (size_t)K * D * 8}, {Q, (size_t)K * D * R * 8}};
    if (const int rc = eig_overlap_check(who, "T", T, (size_t)B * R * 8, inputs)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const EigGeo g{B, N, C, K, R, (long)D};
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_project_kernel, dim3(B), dim3(256), 0, st, aligned, cover, reinterpret_cast<const int*>(label), mean, Q, g, T);
    return launch_status(who);
}

int svae_eig_accumulate(const float* aligned, const uint8_t* cover, const int32_t* label, const double* mean, const double* T,
                        int32_t B, int32_t N, int32_t C, int32_t K, int32_t R, double* Y, double* ssq, svae_stream_t stream) {
    const char* who = "svae_eig_accumulate";
    if (const int rc = eig_images_check(who, aligned, label, mean, B, N, C, K, R)) return rc;
    if (!T || !Y) return fail(SVAE_E_INVALID, "%s: null T or Y", who);
    if (misaligned8(T) || misaligned8(Y) || misaligned8(ssq)) return fail(SVAE_E_INVALID, "%s: T, Y and ssq must be 8-byte aligned", who);
    const size_t D = (size_t)N * C;
    const std::initializer_list<EigSpan> inputs = {{aligned, (size_t)B * D * 4}, {cover, (size_t)B * N}, {label, (size_t)B * 4},
                                                   {mean, (size_t)K * D * 8}, {T, (size_t)B * R * 8}};
    if (const int rc = eig_overlap_check(who, "Y", Y, (size_t)K * D * R * 8, inputs)) return rc;
    if (ssq) {
        if (const int rc = eig_overlap_check(who, "ssq", ssq, (size_t)K * D * 8, inputs)) return rc;
        if (bytes_overlap(ssq, (size_t)K * D * 8, Y, (size_t)K * D * R * 8)) return fail(SVAE_E_INVALID, "%s: ssq overlaps Y", who);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const EigGeo g{B, N, C, K, R, (long)D};
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_accumulate_kernel, dim3(blocks_for((long)K * D * R)), dim3(256), 0, st, aligned, cover,
                       reinterpret_cast<const int*>(label), mean, T, g, Y, ssq);
    return launch_status(who);
}

int svae_eig_orthonormalise(const double* Y, int32_t K, int64_t D, int32_t R, double* Q, svae_stream_t stream) {
    const char* who = "svae_eig_orthonormalise";
    if (const int rc = eig_basis_check(who, K, D, R)) return rc;
    if (!Y || !Q) return fail(SVAE_E_INVALID, "%s: null Y or Q", who);
    if (misaligned8(Y) || misaligned8(Q)) return fail(SVAE_E_INVALID, "%s: Y and Q must be 8-byte aligned", who);
    const size_t basis = (size_t)K * D * R * 8;
    if (const int rc = eig_overlap_check(who, "Q", Q, basis, {{Y, basis}})) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_orthonormalise_kernel, dim3(K), dim3(256), 0, st, Y, (long)D, R, Q);
    return launch_status(who);
}

int svae_eig_gram(const double* Q, const double* Y, const int64_t* members, int32_t K, int64_t D, int32_t R, double* G,
                  svae_stream_t stream) {
    const char* who = "svae_eig_gram";
    if (const int rc = eig_basis_check(who, K, D, R)) return rc;
    if (!Q || !Y || !members || !G) return fail(SVAE_E_INVALID, "%s: null Q, Y, members or G", who);
    if (misaligned8(Q) || misaligned8(Y) || misaligned8(members) || misaligned8(G))
        return fail(SVAE_E_INVALID, "%s: Q, Y, members and G must be 8-byte aligned", who);
    const size_t basis = (size_t)K * D * R * 8;
    if (const int rc = eig_overlap_check(who, "G", G, (size_t)K * R * R * 8, {{Q, basis}, {Y, basis}, {members, (size_t)K * 8}})) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_gram_kernel, dim3(K * R), dim3(256), 0, st, Q, Y, reinterpret_cast<const long long*>(members), (long)D, R, G);
    return launch_status(who);
}

int svae_eig_rotate(const double* Q, const double* Y, const double* W, const double* lambda, const int64_t* members, int32_t K,
                    int64_t D, int32_t R, int32_t P, double* eigenimages, double* residual, double* rot, svae_stream_t stream) {
    const char* who = "svae_eig_rotate";
    if (const int rc = eig_basis_check(who, K, D, R)) return rc;
    if (P < 1 || P > R) return fail(SVAE_E_INVALID, "%s: P = %d must be in 1..R = %d", who, P, R);
    if (!Q || !Y || !W || !lambda || !members || !eigenimages || !residual || !rot)
        return fail(SVAE_E_INVALID, "%s: null Q, Y, W, lambda, members, eigenimages, residual or rot", who);
    if (misaligned8(Q) || misaligned8(Y) || misaligned8(W) || misaligned8(lambda) || misaligned8(members) || misaligned8(eigenimages) ||
        misaligned8(residual) || misaligned8(rot))
        return fail(SVAE_E_INVALID, "%s: every buffer must be 8-byte aligned", who);
    const size_t basis = (size_t)K * D * R * 8;
    const std::initializer_list<EigSpan> inputs = {{Q, basis}, {Y, basis}, {W, (size_t)K * R * R * 8}, {lambda, (size_t)K * R * 8},
                                                   {members, (size_t)K * 8}};
    const EigSpan outs[3] = {{eigenimages, (size_t)K * P * D * 8}, {residual, (size_t)K * P * 8}, {rot, (size_t)K * P * R * 8}};
    const char* names[3] = {"eigenimages", "residual", "rot"};
    for (int i = 0; i < 3; ++i) {
        if (const int rc = eig_overlap_check(who, names[i], outs[i].p, outs[i].bytes, inputs)) return rc;
        for (int j = 0; j < i; ++j)
            if (bytes_overlap(outs[i].p, outs[i].bytes, outs[j].p, outs[j].bytes))
                return fail(SVAE_E_INVALID, "%s: %s overlaps %s", who, names[i], names[j]);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_rotate_kernel, dim3(K * P), dim3(256), 0, st, Q, Y, W, lambda, reinterpret_cast<const long long*>(members),
                       (long)D, R, P, eigenimages, residual, rot);
    return launch_status(who);
}

int svae_eig_coords(const double* T, const int32_t* label, const double* rot, int32_t B, int32_t K, int32_t R, int32_t P,
                    double* coords, svae_stream_t stream) {
    const char* who = "svae_eig_coords";
    if (B < 1 || K < 1 || K > kEigMaxK || R < 1 || R > kEigMaxR || P < 1 || P > R)
        return fail(SVAE_E_INVALID, "%s: bad sizes B=%d K=%d R=%d P=%d (1 <= K <= %d, 1 <= P <= R <= %d)", who, B, K, R, P, kEigMaxK, kEigMaxR);
    if (!T || !label || !rot || !coords) return fail(SVAE_E_INVALID, "%s: null T, label, rot or coords", who);
    if (misaligned8(T) || misaligned8(rot) || misaligned8(coords)) return fail(SVAE_E_INVALID, "%s: T, rot and coords must be 8-byte aligned", who);
    if (const int rc = eig_overlap_check(who, "coords", coords, (size_t)B * P * 8,
                                         {{T, (size_t)B * R * 8}, {label, (size_t)B * 4}, {rot, (size_t)K * P * R * 8}}))
        return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(eig_coords_kernel, dim3(blocks_for((long)B * P)), dim3(256), 0, st, T, reinterpret_cast<const int*>(label), rot, B, K,
                       R, P, coords);
    return launch_status(who);
}

// ---- latent-space neighbour averages (include/svae_neighbours.h) ----
int svae_nbr_search(const double* query, int32_t B, int64_t query_base, const double* cand, int32_t M, int64_t cand_base, int32_t D,
                    int32_t K, double* best_d2, int64_t* best_index, svae_stream_t stream) {
    const char* who = "svae_nbr_search";
    if (B < 1 || M < 1 || D < 1 || D > kNbrMaxD || K < 1 || K > kNbrMaxK || query_base < 0 || cand_base < 0)
        return fail(SVAE_E_INVALID, "%s: bad sizes B=%d M=%d D=%d K=%d query_base=%lld cand_base=%lld (1 <= D <= %d, 1 <= K <= %d, "
                    "1 <= B, 1 <= M, bases >= 0)", who, B, M, D, K, (long long)query_base, (long long)cand_base, kNbrMaxD, kNbrMaxK);
    if (!query || !cand || !best_d2 || !best_index) return fail(SVAE_E_INVALID, "%s: null query, cand, best_d2 or best_index", who);
    if (misaligned8(query) || misaligned8(cand) || misaligned8(best_d2) || misaligned8(best_index))
        return fail(SVAE_E_INVALID, "%s: every buffer must be 8-byte aligned", who);
    const size_t lists = (size_t)B * K * 8;
    const std::initializer_list<EigSpan> inputs = {{query, (size_t)B * D * 8}, {cand, (size_t)M * D * 8}};
    if (const int rc = eig_overlap_check(who, "best_d2", best_d2, lists, inputs)) return rc;
    if (const int rc = eig_overlap_check(who, "best_index", best_index, lists, inputs)) return rc;
    if (bytes_overlap(best_d2, lists, best_index, lists)) return fail(SVAE_E_INVALID, "%s: best_d2 overlaps best_index", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(nbr_search_kernel, dim3((B + kNbrQueries - 1) / kNbrQueries), dim3(256), 0, st, query, B, (long long)query_base, cand,
                       M, (long long)cand_base, D, K, best_d2, reinterpret_cast<long long*>(best_index));
    return launch_status(who);
}

int svae_nbr_average(const float* stack, const uint8_t* cover, int64_t images, int32_t N, int32_t C, const int64_t* index,
                     const double* weight, int32_t B, int32_t T, float* average, double* support, svae_stream_t stream) {
    const char* who = "svae_nbr_average";
    if (images < 1 || images > 0x7fffffffLL || N < 1 || C < 1 || C > SVAE_MAX_OUT || (int64_t)N * C > 0x7fffffffLL || B < 1 || T < 1 ||
        T > kNbrMaxT)
        return fail(SVAE_E_INVALID, "%s: bad sizes images=%lld N=%d C=%d B=%d T=%d (1 <= images < 2^31, C in 1..%d, N C < 2^31, 1 <= B, "
                    "T in 1..%d)", who, (long long)images, N, C, B, T, SVAE_MAX_OUT, kNbrMaxT);
    if (!stack || !index || !average) return fail(SVAE_E_INVALID, "%s: null stack, index or average", who);
    if (misaligned8(index) || misaligned8(weight) || misaligned8(support))
        return fail(SVAE_E_INVALID, "%s: index, weight and support must be 8-byte aligned", who);
    const size_t D = (size_t)N * C, slots = (size_t)B * T * 8;
    const std::initializer_list<EigSpan> inputs = {{stack, (size_t)images * D * 4}, {cover, (size_t)images * N}, {index, slots},
                                                   {weight, slots}};
    if (const int rc = eig_overlap_check(who, "average", average, (size_t)B * D * 4, inputs)) return rc;
    if (support) {
        if (const int rc = eig_overlap_check(who, "support", support, (size_t)B * N * 8, inputs)) return rc;
        if (bytes_overlap(support, (size_t)B * N * 8, average, (size_t)B * D * 4)) return fail(SVAE_E_INVALID, "%s: support overlaps average", who);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Scope prof(K_AUGMENT, st);
    hipLaunchKernelGGL(nbr_average_kernel, dim3(B), dim3(256), 0, st, stack, cover, (long long)images, N, C,
                       reinterpret_cast<const long long*>(index), weight, T, average, support);
    return launch_status(who);
}

#undef POSE_KERNEL

}  // extern "C"
