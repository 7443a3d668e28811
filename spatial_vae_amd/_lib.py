"""ctypes binding of include/svae.h.  Loading fails loudly: there is no fallback path."""
import ctypes
import os

# torch ships its own libamdhip64.so.7; it must be in the process first so that this library's
# NEEDED entry of the same soname binds to THAT runtime (two HIP runtimes in one process do not
# share a device context: launches then fail with "no ROCm-capable device").
import torch  # noqa: F401

from .build import library_path

# ---- the constants of include/svae.h (SVAE_ prefix dropped) ----
# Every upper-case integer of this module is one of the header's #defines or enumerators and nothing else is:
# tests/test_binding_cpu.py compares the two sets and their values.
ABI_VERSION = 2
MAX_HIDDEN = 7
MAX_OUT = 4
IW_MAX_SAMPLES = 1024
LINEAR_ACT_NONE = -1
PROF_KINDS = 20             # length of the arrays svae_profile_read writes
PATH_KINDS = 16             # length of the array svae_path_counts writes
OK, E_INVALID, E_WORKSPACE, E_LAUNCH = 0, -1, -2, -3
ACT_TANH, ACT_LEAKYRELU, ACT_RELU, ACT_SIGMOID = 0, 1, 2, 3
FLAG_RESID, FLAG_BILINEAR, FLAG_SOFTPLUS = 1, 2, 4
GEMM_FP32, GEMM_FP16X3 = 0, 1

ACT = {"tanh": ACT_TANH, "leakyrelu": ACT_LEAKYRELU, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID}
GEMM_MODE = {"fp32": GEMM_FP32, "fp16x3": GEMM_FP16X3}

vp, sz, cint, cstr = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_char_p
i32, i64, f32, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_double
ptr = ctypes.POINTER


# ---- the structs of include/svae.h (device pointers are c_void_p: the callers hold addresses, not ctypes objects) ----
class Desc(ctypes.Structure):
    _fields_ = [(n, i32) for n in ("B", "N", "H", "L", "Zd", "C", "in_dim", "act", "flags")]


class Params(ctypes.Structure):
    _fields_ = [("coord_w", vp), ("coord_b", vp), ("latent_w", vp), ("bilinear_w", vp), ("hidden_w", vp * MAX_HIDDEN),
                ("hidden_b", vp * MAX_HIDDEN), ("out_w", vp), ("out_b", vp)]


Grads = Params      # svae_grads: svae_params' fields without the const (the test holds the header to that)


class Pose(ctypes.Structure):
    _fields_ = [("coords", vp), ("grid", vp), ("theta", vp), ("dx", vp)]


class PoseGrads(ctypes.Structure):
    _fields_ = [("dcoords", vp), ("dtheta", vp), ("ddx", vp)]


class LatentDesc(ctypes.Structure):
    _fields_ = [("B", i32), ("inf_dim", i32), ("rotate", i32), ("translate", i32), ("mu_penalty", i32), ("dx_scale", f32),
                ("z_scale", f32), ("theta_prior", f32)]


class GuardControl(ctypes.Structure):
    """svae_guard_control: all zero bytes = a fresh record; the statistics are the bytes from `steps` to the end."""
    _fields_ = [("t", i64), ("total", f32), ("coef", f32), ("step_size", f32), ("sqrt_bc2", f32), ("apply", i32),
                ("finite", i32), ("steps", i64), ("clipped", i64), ("skipped", i64), ("norm_sum", f64), ("norm_max", f32),
                ("reserved", f32)]


# ---- every function include/svae.h declares: name -> (return type, argument types) ----
# The one declaration of the binding: lib() applies it, EXPORTS is its keys, and tests/test_binding_cpu.py parses the header's
# prototypes and holds each row to them, type by type (the header is documentation: importing the package must not need it).
SIGNATURES = {
    "svae_abi_version": (cint, []),
    "svae_last_error": (cstr, []),
    "svae_saved_bytes": (sz, [ptr(Desc)]),
    "svae_workspace_bytes": (sz, [ptr(Desc)]),
    "svae_decoder_forward": (cint, [ptr(Desc), ptr(Params), ptr(Pose), vp, vp, vp, vp, vp, sz, vp]),
    "svae_decoder_forward_bce": (cint, [ptr(Desc), ptr(Params), ptr(Pose), vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
    "svae_decoder_backward": (cint, [ptr(Desc), ptr(Params), ptr(Pose), vp, vp, vp, vp, vp, ptr(Grads), vp, ptr(PoseGrads),
                                     vp, sz, vp]),
    "svae_bce_loglik": (cint, [i32, i32, vp, vp, vp, vp, vp]),
    "svae_gaussian_workspace_bytes": (sz, [i32, i32]),
    "svae_gaussian_loglik": (cint, [i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, sz, vp]),
    "svae_latent_forward": (cint, [ptr(LatentDesc), vp, vp, vp, vp, vp, vp, vp]),
    "svae_latent_backward": (cint, [ptr(LatentDesc), vp, vp, vp, vp, vp, vp, vp, vp]),
    "svae_elbo_head_forward": (cint, [vp, vp, i32, vp, vp]),
    "svae_elbo_head_backward": (cint, [vp, vp, vp, i32, vp, vp, vp]),
    "svae_latent_iw_forward": (cint, [ptr(LatentDesc), i32, vp, vp, vp, vp, vp, vp, vp]),
    "svae_latent_iw_backward": (cint, [ptr(LatentDesc), i32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "svae_iw_head_forward": (cint, [vp, vp, i32, i32, vp, vp, vp]),
    "svae_iw_head_backward": (cint, [vp, vp, vp, vp, i32, i32, vp, vp, vp]),
    "svae_colsum": (cint, [vp, i32, i32, vp, vp]),
    "svae_linear_forward": (cint, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "svae_linear_backward": (cint, [vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
    "svae_adam_step": (cint, [vp, vp, vp, vp, i64, f32, f32, f32, f32, i64, i32, vp]),
    "svae_grad_guard_control_bytes": (sz, []),
    "svae_grad_guard_workspace_bytes": (sz, [i64]),
    "svae_grad_guard_norm": (cint, [vp, i64, f32, f32, f32, f32, vp, vp, sz, vp]),
    "svae_adam_step_guarded": (cint, [vp, vp, vp, vp, i64, f32, f32, f32, i32, vp, vp]),
    "svae_rotate_bicubic": (cint, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
    "svae_ctf_filter_workspace_bytes": (sz, [i32, i32, i32]),
    "svae_ctf_filter": (cint, [vp, vp, i32, i32, i32, f64, vp, sz, vp]),
    "svae_gemm_mode_set": (cint, [cint]),
    "svae_gemm_mode_get": (cint, []),
    "svae_profile_enable": (cint, [cint]),
    "svae_profile_read": (cint, [ptr(f64), ptr(i64)]),
    "svae_profile_kind_name": (cstr, [cint]),
    "svae_path_counts": (cint, [ptr(i64), cint]),
    "svae_path_name": (cstr, [cint]),
}
EXPORTS = tuple(SIGNATURES)

# ---- include/svae_stream.h: the streaming K-sample scorer, an addition with a header and a table of its own ----
# Same rules as above (tests/test_stream_binding_cpu.py holds these rows to that header's prototypes); `state` is the address
# of a record in device memory.  The header's one macro is iw_stream_cols below.
STREAM_SIGNATURES = {
    "svae_iw_stream_state_bytes": (sz, [i32, i32]),
    "svae_iw_stream_reset": (cint, [vp, i32, i32, vp]),
    "svae_iw_stream_update": (cint, [vp, ptr(LatentDesc), i32, vp, vp, vp, vp, vp, vp]),
    "svae_iw_stream_finish": (cint, [vp, ptr(LatentDesc), vp, vp, vp]),
}


def iw_stream_cols(inf_dim):
    """SVAE_IW_STREAM_COLS(inf_dim): floats per image in svae_iw_stream_finish's per_image."""
    return 6 + 2 * int(inf_dim)


# ---- include/svae_align.h: alignment into the canonical frame and class sums, a third header with a table of its own ----
# Same rules again (tests/test_align_cpu.py holds these rows to that header's prototypes).  The header's two constants are the
# values of ALIGN_INTERP, under SVAE_ALIGN_<NAME>: a name table like ACT, because the upper-case integers of this module are
# svae.h's constants and nothing else.
ALIGN_SIGNATURES = {
    "svae_align_images": (cint, [vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "svae_class_sums_update": (cint, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]),
}
ALIGN_INTERP = {"bilinear": 0, "bicubic": 1}


# ---- include/svae_ctfcorr.h: CTF correction in Fourier space, a fourth header with a table of its own ----
# Same rules once more (tests/test_ctfcorr_cpu.py holds these rows to that header's prototypes).  The header's two constants are
# the values of CTF_MODE, under SVAE_CTF_<NAME>.
CTFCORR_SIGNATURES = {
    "svae_ctf_apply_workspace_bytes": (sz, [i32, i32, i32]),
    "svae_ctf_apply": (cint, [vp, vp, i32, i32, i32, f64, i32, vp, vp, sz, vp]),
    "svae_ctf_power_update": (cint, [vp, vp, i32, i32, i32, f64, i32, vp, vp]),
    "svae_wiener_finish_workspace_bytes": (sz, [i32, i32, i32]),
    "svae_wiener_finish": (cint, [vp, vp, f64, i32, i32, i32, vp, vp, sz, vp]),
}
CTF_MODE = {"flip": 0, "multiply": 1}


# ---- include/svae_cluster.h: k-means over the content latents, a fifth header with a table of its own ----
# Same rules (tests/test_cluster_cpu.py holds these rows, and the mirror of the header's one struct, to that header).  `rec` is
# the address of a record in device memory, like svae_grad_guard_norm's `control`.  The header adds no constant.
class KMeansRecord(ctypes.Structure):
    """svae_kmeans_record: all zero bytes = a fresh record."""
    _fields_ = [("iterations", i64), ("changed", i64), ("converged_at", i64), ("assigned", i64), ("empty", i64), ("inertia", f64)]


CLUSTER_SIGNATURES = {
    "svae_kmeans_workspace_bytes": (sz, [i64, i32, i32]),
    "svae_kmeans_seed": (cint, [vp, i64, i32, i32, vp, vp, vp, vp, sz, vp]),
    "svae_kmeans_step": (cint, [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
}


# ---- include/svae_frc.h: Fourier ring correlation and the filter by per-ring weights, a sixth header with a table of its own ----
# Same rules (tests/test_frc_cpu.py holds these rows to that header's prototypes).  The header adds no constant.
FRC_SIGNATURES = {
    "svae_frc_workspace_bytes": (sz, [i32, i32, i32]),
    "svae_frc": (cint, [vp, vp, i32, i32, i32, f64, f64, vp, vp, vp, vp, sz, vp]),
    "svae_frc_filter_workspace_bytes": (sz, [i32, i32, i32]),
    "svae_frc_filter": (cint, [vp, vp, i32, i32, i32, vp, vp, sz, vp]),
}


# ---- include/svae_refine.h: the reference-based pose search, a seventh header with a table of its own ----
# Same rules (tests/test_refine_cpu.py holds these rows to that header's prototypes).  The header adds no constant: `interp` takes
# the values of ALIGN_INTERP.
REFINE_SIGNATURES = {
    "svae_pose_search_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "svae_pose_search": (cint, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, f64, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
}


# ---- include/svae_classify.h: multi-reference alignment, an eighth header with a table of its own ----
# Same rules (tests/test_classify_cpu.py holds these rows to that header's prototypes).  The header adds no constant: `interp`
# takes the values of ALIGN_INTERP.
CLASSIFY_SIGNATURES = {
    "svae_pose_classify_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32]),
    "svae_pose_classify": (cint, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f64, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
}


# ---- include/svae_gmm.h: the diagonal-covariance Gaussian mixture, a ninth header with a table of its own ----
# Same rules (tests/test_gmm_cpu.py holds these rows, and the mirror of the header's one struct, to that header).  `rec` is the
# address of a record in device memory.  The header adds no constant.
class GmmRecord(ctypes.Structure):
    """svae_gmm_record: all zero bytes = a fresh record."""
    _fields_ = [("iterations", i64), ("converged_at", i64), ("assigned", i64), ("dead", i64), ("loglik", f64), ("previous", f64)]


GMM_SIGNATURES = {
    "svae_gmm_workspace_bytes": (sz, [i64, i32, i32]),
    "svae_gmm_init": (cint, [vp, i64, i32, i32, vp, f64, vp, vp, vp, vp, vp, vp, sz, vp]),
    "svae_gmm_step": (cint, [vp, i64, i32, i32, i32, f64, f64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]),
}


# ---- include/svae_expect.h: maximum-likelihood class averages, a tenth header with a table of its own ----
# Same rules (tests/test_expect_cpu.py holds these rows to that header's prototypes).  The header adds no constant: `interp`
# takes the values of ALIGN_INTERP.
EXPECT_SIGNATURES = {
    "svae_pose_expect_workspace_bytes": (sz, [i32, i32, i32, i32, i32, i32, i32, i32]),
    "svae_pose_expect": (cint, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, f64, i32, i32, f64, vp, vp, vp, vp, vp,
                                vp, sz, vp]),
    "svae_expect_sums_update": (cint, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
}


# ---- include/svae_pca.h: principal axes of the content latents, an eleventh header with a table of its own ----
# Same rules (tests/test_pca_cpu.py holds these rows to that header's prototypes).  The header adds no constant and no struct.
PCA_SIGNATURES = {
    "svae_pca_workspace_bytes": (sz, [i64, i32, i32]),
    "svae_pca_moments": (cint, [vp, i64, i32, i32, vp, vp, vp, vp, vp, sz, vp]),
    "svae_pca_eigen": (cint, [vp, i32, i32, vp, vp, vp, vp, vp]),
    "svae_pca_project": (cint, [vp, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
}


# ---- include/svae_eigen.h: per-class eigenimages of aligned images, a twelfth header with a table of its own ----
# Same rules (tests/test_eigen_cpu.py holds these rows to that header's prototypes).  The header's two constants are the values
# of EIGEN_LIMITS, under SVAE_EIG_<NAME>.
EIGEN_SIGNATURES = {
    "svae_eig_project": (cint, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp]),
    "svae_eig_accumulate": (cint, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp]),
    "svae_eig_orthonormalise": (cint, [vp, i32, i64, i32, vp, vp]),
    "svae_eig_gram": (cint, [vp, vp, vp, i32, i64, i32, vp, vp]),
    "svae_eig_rotate": (cint, [vp, vp, vp, vp, vp, i32, i64, i32, i32, vp, vp, vp, vp]),
    "svae_eig_coords": (cint, [vp, vp, vp, i32, i32, i32, i32, vp, vp]),
}
EIGEN_LIMITS = {"max_r": 64, "dead_log2": -26}


# ---- include/svae_neighbours.h: latent-space neighbour averages, a thirteenth header with a table of its own ----
# Same rules (tests/test_neighbours_cpu.py holds these rows to that header's prototypes).  The header's one constant is the
# value of NEIGHBOUR_LIMITS, under SVAE_NBR_<NAME>.
NEIGHBOUR_SIGNATURES = {
    "svae_nbr_search": (cint, [vp, i32, i64, vp, i32, i64, i32, i32, vp, vp, vp]),
    "svae_nbr_average": (cint, [vp, vp, i64, i32, i32, vp, vp, i32, i32, vp, vp, vp]),
}
NEIGHBOUR_LIMITS = {"max_k": 256}


# ---- the one list of the headers of include/, in the order they were added: header -> its table above ----
# lib(), ops._POINTER_ARGS, build.dependencies() and __graft_entry__.build() walk it; a fourteenth header is one more row.
# tests/test_binding_cpu.py holds every row to its header's prototypes by one rule (the test files named above: what is a
# header's own), and every function here that takes a stream has a row in the tests' shared stream table.
HEADERS = {
    "svae.h": SIGNATURES, "svae_stream.h": STREAM_SIGNATURES, "svae_align.h": ALIGN_SIGNATURES,
    "svae_ctfcorr.h": CTFCORR_SIGNATURES, "svae_cluster.h": CLUSTER_SIGNATURES, "svae_frc.h": FRC_SIGNATURES,
    "svae_refine.h": REFINE_SIGNATURES, "svae_classify.h": CLASSIFY_SIGNATURES, "svae_gmm.h": GMM_SIGNATURES,
    "svae_expect.h": EXPECT_SIGNATURES, "svae_pca.h": PCA_SIGNATURES, "svae_eigen.h": EIGEN_SIGNATURES,
    "svae_neighbours.h": NEIGHBOUR_SIGNATURES,
}
ALL_SIGNATURES = {name: row for table in HEADERS.values() for name, row in table.items()}


def declared_in_header(header=None):
    """The function names include/svae.h (or another header of include/) declares (used by build() and the tests, never at
    import)."""
    import re
    header = header or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "svae.h")
    with open(header) as f:
        return tuple(sorted(set(re.findall(r"\b(svae_[a-z0-9_]+)\s*\(", f.read()))))


_lib = None


def lib():
    """The loaded library.  Raises if it was never built: the product path has no other backend."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise RuntimeError("spatial_vae_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(or spatial_vae_amd.build()); there is no fallback implementation" % path)
    L = ctypes.CDLL(path)
    for name, (restype, argtypes) in ALL_SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    if L.svae_abi_version() != ABI_VERSION:
        raise RuntimeError("spatial_vae_amd: %s has ABI version %d, this binding needs %d -- rebuild it"
                           % (path, L.svae_abi_version(), ABI_VERSION))
    if L.svae_grad_guard_control_bytes() != ctypes.sizeof(GuardControl):
        raise RuntimeError("spatial_vae_amd: %s lays out svae_guard_control in %d bytes, this binding in %d -- rebuild it"
                           % (path, L.svae_grad_guard_control_bytes(), ctypes.sizeof(GuardControl)))
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RuntimeError("svae: %s (code %d)" % (lib().svae_last_error().decode(), rc))


def set_gemm_mode(name):
    """'fp32' (fp32 MFMA) or 'fp16x3' (split-operand f16 MFMA, fp32-accurate).  Call before any decoder call of the process:
    buffer sizes depend on it."""
    check(lib().svae_gemm_mode_set(GEMM_MODE[name]))


def gemm_mode():
    mode = lib().svae_gemm_mode_get()
    return next(name for name, code in GEMM_MODE.items() if code == mode)


def profile_enable(level):
    """0 = off, 1 = the three MFMA GEMM kernels only (cheap enough for a timed region), 2 = every kernel."""
    check(lib().svae_profile_enable(int(level)))


def profile_read():
    """{kernel kind: (total ms, launches)} since the last read; synchronises the recorded events."""
    L = lib()
    ms = (ctypes.c_double * PROF_KINDS)()
    cnt = (ctypes.c_int64 * PROF_KINDS)()
    check(L.svae_profile_read(ms, cnt))
    return {L.svae_profile_kind_name(k).decode(): (ms[k], cnt[k]) for k in range(PROF_KINDS) if cnt[k]}


def path_counts(reset=False):
    """{kernel family: launches} dispatched by this process (svae_path_counts): tells a run of the fp16x3 split kernels, the
    rank-1 output-layer backward etc. from a fallback to the plain fp32 kernels."""
    L = lib()
    arr = (ctypes.c_int64 * PATH_KINDS)()
    check(L.svae_path_counts(arr, 1 if reset else 0))
    return {L.svae_path_name(i).decode(): int(arr[i]) for i in range(PATH_KINDS) if L.svae_path_name(i)}
