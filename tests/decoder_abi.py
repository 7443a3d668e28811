"""Helper of tests/test_gpu_decoder_abi.py and tests/test_decoder_abi_cpu.py (not collected): the case table, the float64 /
float32 CPU references and a caller of svae_decoder_forward / _forward_bce / _backward that goes through ctypes alone.

Unlike ops._Decoder the caller here owns every buffer: each one the library writes sits 256-byte aligned inside a larger
allocation with GUARD bytes of 0xA5 on both sides, `saved` is exactly svae_saved_bytes and the workspace exactly
svae_workspace_bytes long, the two calls can be given different workspaces, and every gradient sink, `saved`, `logits`,
`dy_scale`, `dz` and `pg` can be NULL on its own."""
import ctypes
import functools
import zlib
import numpy as np
import torch

from oracle import torch_cpu_step as T

GUARD = 4096
GUARD_BYTE = 0xA5
SENTINEL = -12345.5
U = 2.0 ** -24
FLAGS = {"resid": 1, "bilinear": 2, "softplus": 4}

# name, N, B, H, L, C, Zd, in_dim, activation, flags, pose form: the smallest shapes at which each branch of the plan can go
# wrong (32-row tiles, Hp = H rounded up to 32, four-tile row groups, 16 image lanes, kZChunk = 8 latent coordinates)
CASES = [
    ("one_image_subtile", 15, 1, 7, 1, 1, 0, 2, "tanh", (), "grid+theta"),
    ("L1_c4_softplus", 33, 3, 33, 1, 4, 2, 2, "sigmoid", ("softplus",), "grid+theta+dx"),
    ("rank1_tanh", 25, 4, 64, 2, 1, 2, 2, "tanh", (), "grid+theta+dx"),
    ("rank1_sigmoid_rag", 33, 5, 100, 2, 1, 3, 2, "sigmoid", (), "grid+theta+dx"),
    ("stream_c2_L3", 64, 3, 96, 3, 2, 9, 2, "tanh", (), "grid+dx"),
    ("relu_c3_coords", 40, 17, 64, 2, 3, 1, 2, "relu", (), "coords"),
    ("leaky_resid_L4", 25, 4, 65, 4, 2, 2, 2, "leakyrelu", ("resid",), "grid+theta+dx"),
    ("expand_bilinear", 49, 4, 48, 3, 1, 4, 5, "tanh", ("bilinear",), "coords"),
    ("deepest_c4", 36, 2, 36, 8, 4, 2, 2, "tanh", (), "grid"),
    ("resid_tanh_w64", 36, 3, 64, 4, 1, 2, 2, "tanh", ("resid",), "grid+theta+dx"),
    ("many_images", 9, 65, 32, 2, 1, 2, 2, "tanh", (), "grid+theta+dx"),
    ("z0_sigmoid_w128", 35, 3, 128, 3, 2, 0, 2, "sigmoid", (), "grid+theta"),
]
# rank1_tanh with 1280 padded rows (ten four-tile groups = three sets): room for a half-width tail launch of dense4
VARIANTS = [("rank1_tanh_b20", 64, 20, 64, 2, 1, 2, 2, "tanh", (), "grid+theta+dx")]
FIELDS = ("name", "N", "B", "H", "L", "C", "Zd", "in_dim", "act", "flags", "pose")
BY_NAME = {c[0]: dict(zip(FIELDS, c)) for c in CASES + VARIANTS}
NAMES = [c[0] for c in CASES]

# What the plan (api.hip) derives for each case, written out so that editing a shape cannot silently drop a branch:
# Hp, padded rows Mp, rank1_out (one channel, tanh / sigmoid, no residual, L >= 2), dense4 legal (whole four-tile row groups,
# no residual), ntile even (the fp16x3 kernels' condition), fused first-layer backward (in_dim == 2 and L >= 2)
EXPECT = {
    "one_image_subtile": dict(Hp=32, Mp=32, rank1=False, dense4=False, ntile_even=False, fused_first=False),
    "L1_c4_softplus": dict(Hp=64, Mp=192, rank1=False, dense4=False, ntile_even=True, fused_first=False),
    "rank1_tanh": dict(Hp=64, Mp=128, rank1=True, dense4=True, ntile_even=True, fused_first=True),
    "rank1_sigmoid_rag": dict(Hp=128, Mp=320, rank1=True, dense4=False, ntile_even=True, fused_first=True),
    "stream_c2_L3": dict(Hp=96, Mp=192, rank1=False, dense4=False, ntile_even=False, fused_first=True),
    "relu_c3_coords": dict(Hp=64, Mp=1088, rank1=False, dense4=False, ntile_even=True, fused_first=True),
    "leaky_resid_L4": dict(Hp=96, Mp=128, rank1=False, dense4=False, ntile_even=False, fused_first=True),
    "expand_bilinear": dict(Hp=64, Mp=256, rank1=True, dense4=True, ntile_even=True, fused_first=False),
    "deepest_c4": dict(Hp=64, Mp=128, rank1=False, dense4=True, ntile_even=True, fused_first=True),
    "resid_tanh_w64": dict(Hp=64, Mp=192, rank1=False, dense4=False, ntile_even=True, fused_first=True),
    "many_images": dict(Hp=32, Mp=2080, rank1=True, dense4=False, ntile_even=False, fused_first=True),
    "z0_sigmoid_w128": dict(Hp=128, Mp=192, rank1=False, dense4=False, ntile_even=True, fused_first=True),
    "rank1_tanh_b20": dict(Hp=64, Mp=1280, rank1=True, dense4=True, ntile_even=True, fused_first=True),
}


def case(name):
    return BY_NAME[name] if isinstance(name, str) else name


def predicates(c):
    """The plan's predicates restated from the descriptor (make_geo, rank1_out, use_dense4, split_active, fused_first)."""
    c = case(c)
    npad = (c["N"] + 31) // 32 * 32
    hp = (c["H"] + 31) // 32 * 32
    mp = c["B"] * npad
    bounded = c["act"] in ("tanh", "sigmoid")
    resid = "resid" in c["flags"]
    return dict(Hp=hp, Mp=mp, rank1=c["C"] == 1 and c["L"] >= 2 and not resid and bounded,
                dense4=(mp // 32) % 4 == 0 and not resid, ntile_even=(hp // 32) % 2 == 0,
                fused_first=c["in_dim"] == 2 and c["L"] >= 2)


def split_eligible(c):
    """fp16x3 mode takes the f16 kernels: bounded activation, an even number of 32-column tiles, at least one hidden GEMM."""
    c = case(c)
    return c["act"] in ("tanh", "sigmoid") and predicates(c)["ntile_even"] and c["L"] >= 2


def sink_names(c):
    """Every output the backward call can write for this case, in a fixed order."""
    c = case(c)
    out = ["coord_w", "coord_b"]
    if c["Zd"] > 0:
        out.append("latent_w")
    if "bilinear" in c["flags"]:
        out.append("bilinear_w")
    for i in range(c["L"] - 1):
        out += ["hidden_w%d" % i, "hidden_b%d" % i]
    out += ["out_w", "out_b"]
    if c["Zd"] > 0:
        out.append("dz")
    if c["pose"] == "coords":
        out.append("dcoords")
    if "theta" in c["pose"]:
        out.append("dtheta")
    if "dx" in c["pose"]:
        out.append("ddx")
    return out


POSE_SINKS = ("dcoords", "dtheta", "ddx")
PER_IMAGE = ("dz",) + POSE_SINKS


# ---------------------------------------------------------------------------------------------------------------------
# inputs and references
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs(name, seed=0):
    """float32 numpy inputs of a case, seeded by its name (and `seed`: 0 is the set every reference here is computed on, another
    value draws a second set of the same shapes): parameters as nn.Linear / nn.Bilinear draw them
    (uniform(+-1/sqrt(fan_in))), z ~ normal, theta ~ uniform(-3, 3), dx ~ 0.1 normal, coordinates uniform(-1, 1),
    dy ~ normal / N, Bernoulli targets k / 255."""
    c = case(name)
    rs = np.random.RandomState((zlib.crc32(c["name"].encode()) + 7919 * int(seed)) & 0x7FFFFFFF)
    N, B, H, L, C, Zd, ind = (c[k] for k in ("N", "B", "H", "L", "C", "Zd", "in_dim"))

    def uni(fan_in, *shape):
        k = 1.0 / np.sqrt(fan_in)
        return rs.uniform(-k, k, size=shape).astype(np.float32)

    p = {"coord_w": uni(ind, H, ind), "coord_b": uni(ind, H)}
    if Zd > 0:
        p["latent_w"] = uni(Zd, H, Zd)
    if "bilinear" in c["flags"]:
        p["bilinear_w"] = uni(ind, H, ind, Zd)
    for i in range(L - 1):
        p["hidden_w%d" % i] = uni(H, H, H)
        p["hidden_b%d" % i] = uni(H, H)
    p["out_w"], p["out_b"] = uni(H, C, H), uni(H, C)
    d = {"z": rs.normal(size=(B, Zd)).astype(np.float32)}
    if c["pose"] == "coords":
        d["coords"] = rs.uniform(-1, 1, size=(B, N, 2)).astype(np.float32)
    else:
        d["grid"] = rs.uniform(-1, 1, size=(N, 2)).astype(np.float32)
        if "theta" in c["pose"]:
            d["theta"] = rs.uniform(-3, 3, size=B).astype(np.float32)
        if "dx" in c["pose"]:
            d["dx"] = (0.1 * rs.normal(size=(B, 2))).astype(np.float32)
    d["dy"] = (rs.normal(size=(B, N, C)) / N).astype(np.float32)
    d["target"] = (np.floor(rs.uniform(size=(B, N, C)) * 255) / 255).astype(np.float32)
    return p, d


def _state_dict(p, L, dtype):
    """The parameter dict oracle.torch_cpu_step.decoder reads, as leaves that require a gradient."""
    leaf = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in p.items()}
    pp = {"coord_linear.weight": leaf["coord_w"], "coord_linear.bias": leaf["coord_b"]}
    if "latent_w" in leaf:
        pp["latent_linear.weight"] = leaf["latent_w"]
    if "bilinear_w" in leaf:
        pp["bilinear.weight"] = leaf["bilinear_w"]
    for i in range(L - 1):
        pp["layers.%d.weight" % i], pp["layers.%d.bias" % i] = leaf["hidden_w%d" % i], leaf["hidden_b%d" % i]
    pp["layers.%d.weight" % (L - 1)], pp["layers.%d.bias" % (L - 1)] = leaf["out_w"], leaf["out_b"]
    return leaf, pp


_REFS = {}


def reference(name, dtype, dy_scale=None):
    """oracle.torch_cpu_step.decoder on the CPU in `dtype`, the pose applied in torch in the same dtype
    (x'' = grid @ [[cos t, sin t], [-sin t, cos t]] + dx), and autograd of sum(y * dy * dy_scale[b]): a dict of numpy arrays
    y, logits and every name of sink_names(case).  float64 is the reference, float32 the yardstick."""
    c = case(name)
    key = (c["name"], dtype, None if dy_scale is None else np.asarray(dy_scale, np.float32).tobytes())
    if key in _REFS:
        return _REFS[key]
    p, d = inputs(c["name"])
    leaf, pp = _state_dict(p, c["L"], dtype)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in d.items()}
    z = t["z"].requires_grad_(True)
    if c["pose"] == "coords":
        x = t["coords"].requires_grad_(True)
        leaf["dcoords"] = x
    else:
        x = t["grid"].unsqueeze(0).expand(c["B"], c["N"], 2)
        if "theta" in t:
            th = t["theta"].requires_grad_(True)
            leaf["dtheta"] = th
            rot = torch.stack([torch.stack([torch.cos(th), torch.sin(th)], 1),
                               torch.stack([-torch.sin(th), torch.cos(th)], 1)], 1)
            x = torch.bmm(x, rot)
        if "dx" in t:
            dx = t["dx"].requires_grad_(True)
            leaf["ddx"] = dx
            x = x + dx.unsqueeze(1)
        x = x.contiguous()
    leaf["dz"] = z
    linear_outputs = []

    def recording_linear(*a, **k):                  # the decoder's last F.linear call is the output layer: its logits
        linear_outputs.append(torch.nn.functional.linear(*a, **k))
        return linear_outputs[-1]

    class Functional(object):                        # torch.nn.functional with that one function replaced
        linear = staticmethod(recording_linear)

        def __getattr__(self, attr):
            return getattr(torch.nn.functional, attr)

    kept, T.F = T.F, Functional()
    try:
        y = T.decoder(pp, x, z, c["act"], resid="resid" in c["flags"], softplus="softplus" in c["flags"],
                      expand_coords=c["in_dim"] == 5)
    finally:
        T.F = kept
    dy = t["dy"]
    if dy_scale is not None:
        dy = dy * torch.from_numpy(np.asarray(dy_scale, np.float32)).to(dtype).view(-1, 1, 1)
    (y * dy).sum().backward()
    out = {"y": y.detach().numpy(), "logits": linear_outputs[-1].detach().view(c["B"], c["N"], c["C"]).numpy()}
    for nm in sink_names(c):
        out[nm] = leaf[nm].grad.numpy()
    _REFS[key] = out
    return out


def bce64(y, target):
    """Per-image Bernoulli log-likelihood of the returned fp32 y, in float64 with torch's clamps at -100."""
    y, tg = y.astype(np.float64), target.astype(np.float64)
    with np.errstate(divide="ignore"):
        ll = tg * np.maximum(np.log(y), -100.0) + (1.0 - tg) * np.maximum(np.log1p(-y), -100.0)
    return ll.reshape(y.shape[0], -1).sum(1)


# ---------------------------------------------------------------------------------------------------------------------
# guarded device buffers
# ---------------------------------------------------------------------------------------------------------------------
class Guarded(object):
    """`nbytes` of device memory, 256-byte aligned, with GUARD bytes of 0xA5 in front and behind inside one allocation."""

    def __init__(self, nbytes, dev):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD + 256,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.off = GUARD + (-(self.buf.data_ptr() + GUARD)) % 256
        self.ptr = self.buf.data_ptr() + self.off
        assert self.ptr % 256 == 0

    def fill_byte(self, byte):
        self.buf[self.off:self.off + self.nbytes].fill_(byte)
        return self

    def fill_float(self, value):
        assert self.nbytes % 4 == 0
        self.buf[self.off:self.off + self.nbytes].view(torch.float32).fill_(value)
        return self

    def read(self, shape=None):
        """(payload as float32 numpy [reshaped], guards intact?) -- one copy of the whole allocation."""
        a = self.buf.cpu().numpy()
        intact = bool((a[:self.off] == GUARD_BYTE).all() and (a[self.off + self.nbytes:] == GUARD_BYTE).all())
        pay = a[self.off:self.off + self.nbytes].copy()
        return (pay.view(np.float32).reshape(shape) if shape is not None else pay), intact


def _dev():
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def make_desc(c):
    from spatial_vae_amd import _lib
    c = case(c)
    flags = sum(FLAGS[f] for f in c["flags"])
    return _lib.Desc(c["B"], c["N"], c["H"], c["L"], c["Zd"], c["C"], c["in_dim"], _lib.ACT[c["act"]], flags)


def _shape(c, name):
    B, N, H, C, Zd, ind = (c[k] for k in ("B", "N", "H", "C", "Zd", "in_dim"))
    if name.startswith("hidden_w"):
        return (H, H)
    if name.startswith("hidden_b"):
        return (H,)
    return {"coord_w": (H, ind), "coord_b": (H,), "latent_w": (H, Zd), "bilinear_w": (H, ind, Zd), "out_w": (C, H),
            "out_b": (C,), "dz": (B, Zd), "dcoords": (B, N, 2), "dtheta": (B,), "ddx": (B, 2), "y": (B, N, C),
            "logits": (B, N, C), "dll_dy": (B, N, C), "loglik": (B,)}[name]


class Forward(object):
    """One svae_decoder_forward[_bce] call on a case; backward() runs svae_decoder_backward from what it left.

    saved / logits: present or NULL; fill: the byte `saved` and the workspace are pre-filled with; bce: None (plain forward),
    "dll" or "nodll" (svae_decoder_forward_bce with / without dll_dy).  After the call: out (numpy, by name), paths
    (svae_path_counts of this call), bad_guards (names of buffers whose guard bytes changed)."""

    def __init__(self, name, saved=True, logits=True, fill=0x00, bce=None, seed=0, run=True):
        """Allocates every buffer of the call; run=False stops there (enqueue() and collect() are then the caller's)."""
        from spatial_vae_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.c = c = case(name)
        self.dev = dev = _dev()
        self.fill = fill
        self.bce = bce
        p, d = inputs(c["name"], seed)
        self.tens = {k: torch.from_numpy(v).to(dev) for k, v in list(p.items()) + list(d.items())}
        self.desc = make_desc(c)
        self.saved_bytes = self.L.svae_saved_bytes(ctypes.byref(self.desc))
        self.ws_bytes = self.L.svae_workspace_bytes(ctypes.byref(self.desc))
        assert self.saved_bytes > 0 and self.ws_bytes > 0
        self.params = self._param_struct(_lib.Params(), {k: self.tens[k].data_ptr() for k in p})
        self.pose = _lib.Pose()
        for k in ("coords", "grid", "theta", "dx"):
            setattr(self.pose, k, self.tens[k].data_ptr() if k in self.tens else None)
        self.z = self.tens["z"].data_ptr() if c["Zd"] > 0 else None
        self.saved = Guarded(self.saved_bytes, dev).fill_byte(fill) if saved else None
        self.ws = Guarded(self.ws_bytes, dev).fill_byte(fill)
        self.bufs = {"y": self._out("y")}
        if logits:
            self.bufs["logits"] = self._out("logits")
        if bce:
            self.bufs["loglik"] = self._out("loglik")
            if bce == "dll":
                self.bufs["dll_dy"] = self._out("dll_dy")
        self.bwd = None
        if not run:
            return
        _lib.path_counts(reset=True)
        with torch.cuda.device(dev):
            self.rc = self.enqueue(_stream())
        _lib.check(self.rc)
        torch.cuda.synchronize()
        self.paths = {k: v for k, v in _lib.path_counts(reset=True).items() if v}
        self.collect()

    def enqueue(self, stream):
        """The one svae_decoder_forward[_bce] call on `stream`; returns its status.  Nothing else: no allocation, copy or wait."""
        ptr = {k: (self.bufs[k].ptr if k in self.bufs else None) for k in ("y", "logits", "loglik", "dll_dy")}
        sv = self.saved.ptr if self.saved is not None else None
        if self.bce:
            return self.L.svae_decoder_forward_bce(ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.pose),
                                                   self.z, self.tens["target"].data_ptr(), ptr["y"], ptr["logits"], ptr["loglik"],
                                                   ptr["dll_dy"], sv, self.ws.ptr, self.ws_bytes, stream)
        return self.L.svae_decoder_forward(ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.pose), self.z,
                                           ptr["y"], ptr["logits"], sv, self.ws.ptr, self.ws_bytes, stream)

    def collect(self):
        """Read the forward's outputs back: out (numpy, by name) and bad_guards."""
        self.out, self.bad_guards = _collect(self.c, self.bufs)
        self.bad_guards += _guards_only(dict(ws=self.ws, saved=self.saved))
        return self.out, self.bad_guards

    def _out(self, name):
        return Guarded(4 * int(np.prod(_shape(self.c, name))), self.dev).fill_float(SENTINEL)

    def _param_struct(self, st, ptrs):
        hw, hb = [None] * self._lib.MAX_HIDDEN, [None] * self._lib.MAX_HIDDEN
        for k, v in ptrs.items():
            if k.startswith("hidden_w"):
                hw[int(k[8:])] = v
            elif k.startswith("hidden_b"):
                hb[int(k[8:])] = v
            else:
                setattr(st, k, v)
        st.hidden_w = (ctypes.c_void_p * self._lib.MAX_HIDDEN)(*hw)
        st.hidden_b = (ctypes.c_void_p * self._lib.MAX_HIDDEN)(*hb)
        return st

    def backward(self, sinks=None, dy_scale=None, separate_ws=False, null_pg=False, check=True):
        """One svae_decoder_backward call.  sinks: the outputs to request (default: all of sink_names); every other field is
        NULL, and with no pose sink at all `pg` itself is NULL when null_pg (else a struct of NULLs).  separate_ws: the
        forward's workspace is first overwritten with the fill byte and the call gets a fresh workspace, filled likewise.
        Returns (outputs by name, path counts of this call, names of buffers whose guards changed)."""
        _lib = self._lib
        self.alloc_backward(sinks=sinks, dy_scale=dy_scale, separate_ws=separate_ws, null_pg=null_pg)
        _lib.path_counts(reset=True)
        with torch.cuda.device(self.dev):
            rc = self.enqueue_backward(_stream())
        if check:
            _lib.check(rc)
        torch.cuda.synchronize()
        paths = {k: v for k, v in _lib.path_counts(reset=True).items() if v}
        out, bad = self.collect_backward()
        return out, paths, bad

    def alloc_backward(self, sinks=None, dy_scale=None, separate_ws=False, null_pg=False):
        """Every buffer and struct of the backward call (see backward); kept in self.bwd."""
        _lib, c, dev = self._lib, self.c, self.dev
        sinks = list(sink_names(c) if sinks is None else sinks)
        assert set(sinks) <= set(sink_names(c)), sinks
        assert self.saved is not None and "logits" in self.bufs
        bufs = {nm: Guarded(4 * int(np.prod(_shape(c, nm))), dev).fill_float(SENTINEL) for nm in sinks}
        grads = self._param_struct(_lib.Grads(), {k: b.ptr for k, b in bufs.items() if k not in PER_IMAGE})
        pg = _lib.PoseGrads()
        for k in POSE_SINKS:
            setattr(pg, k, bufs[k].ptr if k in bufs else None)
        has_pose = any(k in bufs for k in POSE_SINKS)
        ws = self.ws
        if separate_ws:
            self.ws.fill_byte(self.fill)
            ws = Guarded(self.ws_bytes, dev).fill_byte(self.fill)
        scale = None
        if dy_scale is not None:
            scale = torch.from_numpy(np.asarray(dy_scale, np.float32)).to(dev)
            assert scale.shape == (c["B"],)
        self.bwd = dict(bufs=bufs, grads=grads, pg=pg, pg_null=null_pg and not has_pose, ws=ws, scale=scale)
        return self.bwd

    def enqueue_backward(self, stream):
        """The one svae_decoder_backward call on `stream`; returns its status.  Nothing else."""
        w = self.bwd
        bufs = w["bufs"]
        return self.L.svae_decoder_backward(ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.pose), self.z,
                                            self.bufs["logits"].ptr, self.tens["dy"].data_ptr(),
                                            None if w["scale"] is None else w["scale"].data_ptr(), self.saved.ptr,
                                            ctypes.byref(w["grads"]), bufs["dz"].ptr if "dz" in bufs else None,
                                            None if w["pg_null"] else ctypes.byref(w["pg"]), w["ws"].ptr, self.ws_bytes, stream)

    def collect_backward(self):
        """(outputs by name, names of buffers whose guards changed) of the backward call."""
        out, bad = _collect(self.c, self.bwd["bufs"])
        bad += _guards_only(dict(ws_backward=self.bwd["ws"], ws_forward=self.ws, saved=self.saved, logits=self.bufs["logits"],
                                 y=self.bufs["y"]))
        return out, bad


def _collect(c, bufs):
    out, bad = {}, []
    for nm, b in bufs.items():
        out[nm], ok = b.read(_shape(c, nm))
        if not ok:
            bad.append(nm)
    return out, bad


def _guards_only(bufs):
    return [nm for nm, b in bufs.items() if b is not None and not b.read()[1]]


def run_abi(name, sinks=None, dy_scale=None, saved=True, logits=True, fill=0x00, separate_ws=False, bce=None, backward=True):
    """Forward (and, with `saved` and `logits`, backward) of one case through the C ABI; see Forward / Forward.backward for
    the options.  Returns dict(out=, paths=, bad_guards=): every output by name, svae_path_counts of the call pair (reset
    before it), and the buffers whose guard bytes changed."""
    f = Forward(name, saved=saved, logits=logits, fill=fill, bce=bce)
    res = dict(out=dict(f.out), paths=dict(f.paths), bad_guards=list(f.bad_guards))
    if backward and saved and logits:
        out, paths, bad = f.backward(sinks=sinks, dy_scale=dy_scale, separate_ws=separate_ws)
        res["out"].update(out)
        for k, v in paths.items():
            res["paths"][k] = res["paths"].get(k, 0) + v
        res["bad_guards"] = sorted(set(res["bad_guards"] + bad))
    return res


def sentinel_hits(a):
    """Entries of a float32 array that still hold the sentinel's bit pattern."""
    return int((np.asarray(a, np.float32).view(np.uint32) == np.float32(SENTINEL).view(np.uint32)).sum())
