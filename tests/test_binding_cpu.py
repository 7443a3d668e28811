"""CPU-only: spatial_vae_amd/_lib.py restates include/svae.h (constants, struct layouts, one signature per function) and
nothing at import time compares the two.  This file does: it parses the header with a few regexes and holds the binding to
every prototype, struct field and constant -- and holds the parser to altered copies of the header, so that a parser which
silently matches nothing cannot pass for agreement."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double, "uint8_t": ctypes.c_uint8}

# (function, parameter) pairs whose `svae_X*` is the address of a record in DEVICE memory: the binding hands over an integer
# address (c_void_p), not a pointer to its host-side mirror.  Everywhere else a struct pointer must be POINTER(mirror).
DEVICE_STRUCT_ARGS = {("svae_grad_guard_norm", "control"), ("svae_adam_step_guarded", "control")}


def _binding():
    from spatial_vae_amd import _lib
    return _lib


def _mirrors(B):
    return {"svae_desc": B.Desc, "svae_params": B.Params, "svae_grads": B.Grads, "svae_pose": B.Pose,
            "svae_pose_grads": B.PoseGrads, "svae_latent_desc": B.LatentDesc, "svae_guard_control": B.GuardControl}


def _declarator(text):
    """'const float* hidden_w[SVAE_MAX_HIDDEN]' -> ('float', True, 'hidden_w', 'SVAE_MAX_HIDDEN'): base type, is it a pointer,
    name ('' for a bare type), array length (None for a scalar).  const is dropped: ctypes has no notion of it."""
    m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w*)\s*(?:\[\s*(\w+)\s*\])?", text.strip())
    assert m, "cannot parse the declarator %r" % text
    return m.group(1), bool(m.group(2)), m.group(3), m.group(4)


def parse_header(text):
    """{'constants': {SVAE_X: int}, 'structs': {svae_x: [(base, pointer, name, length)]},
    'functions': {svae_x: ((base, pointer), [(base, pointer, name)])}} of the text of include/svae.h."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*#\s*define\s+(SVAE_\w+)\s+\(?\s*(-?\d+)\s*\)?\s*$", text, re.M)}
    for body in re.findall(r"\benum\s*\{(.*?)\}\s*;", text, re.S):
        for item in filter(None, (i.strip() for i in body.split(","))):
            name, value = (s.strip() for s in item.split("="))
            constants[name] = int(value)
    structs = {}
    for name, body in re.findall(r"\btypedef\s+struct\s+(svae_\w+)\s*\{(.*?)\}\s*\1\s*;", text, re.S):
        structs[name] = [_declarator(f) for f in body.split(";") if f.strip()]
    # what is left once preprocessor lines, enums, struct and plain typedefs and the extern "C" braces are gone is prototypes
    rest = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    rest = re.sub(r"\benum\s*\{.*?\}\s*;", " ", rest, flags=re.S)
    rest = re.sub(r"\btypedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", rest, flags=re.S)
    rest = re.sub(r"\btypedef\b[^;{}]*;", " ", rest)
    rest = re.sub(r'extern\s+"C"\s*\{|\}', " ", rest)
    functions = {}
    for stmt in filter(None, (s.strip() for s in rest.split(";"))):
        m = re.fullmatch(r"(.*?)\b(svae_\w+)\s*\((.*)\)", stmt, re.S)
        assert m, "include/svae.h: cannot parse the statement %r" % stmt
        args = [] if m.group(3).strip() == "void" else [_declarator(a)[:3] for a in m.group(3).split(",")]
        functions[m.group(2)] = (_declarator(m.group(1))[:2], args)
    return {"constants": constants, "structs": structs, "functions": functions}


def _allowed(base, pointer, B, device_record=False):
    """The ctypes types that may stand for the C type."""
    if base == "svae_stream_t" and not pointer:
        return [ctypes.c_void_p]
    if not pointer:
        return [SCALARS[base]]
    if base == "void":
        return [ctypes.c_void_p]
    if base == "char":
        return [ctypes.c_char_p]
    if base in SCALARS:
        return [ctypes.c_void_p, ctypes.POINTER(SCALARS[base])]
    return [ctypes.c_void_p] if device_record else [ctypes.POINTER(_mirrors(B)[base])]


def _name(t):
    return getattr(t, "__name__", repr(t))


def binding_constants(B):
    """The binding's constants block: every upper-case integer of the module, under its header name."""
    return {"SVAE_" + k: v for k, v in vars(B).items() if k.isupper() and type(v) is int}


def compare(header_text, B):
    """Every disagreement between the header and the binding, one line each, naming the function, struct or constant."""
    H = parse_header(header_text)
    out = []
    # constants, both ways
    mine = binding_constants(B)
    for name in sorted(set(H["constants"]) | set(mine)):
        if H["constants"].get(name) != mine.get(name):
            out.append("constant %s: header %s, binding %s" % (name, H["constants"].get(name), mine.get(name)))
    # functions, both ways, then type by type
    for name in sorted(set(H["functions"]) ^ set(B.SIGNATURES)):
        out.append("function %s: %s" % (name, "not in the binding's table" if name in H["functions"] else "not in the header"))
    for name in sorted(set(H["functions"]) & set(B.SIGNATURES)):
        (rbase, rptr), args = H["functions"][name]
        restype, argtypes = B.SIGNATURES[name]
        if restype not in _allowed(rbase, rptr, B):
            out.append("function %s: returns %s%s, binding %s" % (name, rbase, "*" * rptr, _name(restype)))
        if len(args) != len(argtypes):
            out.append("function %s: %d arguments, binding %d" % (name, len(args), len(argtypes)))
            continue
        for i, ((base, pointer, arg), have) in enumerate(zip(args, argtypes)):
            if have not in _allowed(base, pointer, B, (name, arg) in DEVICE_STRUCT_ARGS):
                out.append("function %s: argument %d (%s) is %s%s, binding %s" % (name, i, arg, base, "*" * pointer, _name(have)))
    # structs
    mirrors = _mirrors(B)
    for name in sorted(set(H["structs"]) ^ set(mirrors)):
        out.append("struct %s: %s" % (name, "no mirror in the binding" if name in H["structs"] else "not in the header"))
    for name in sorted(set(H["structs"]) & set(mirrors)):
        fields, have = H["structs"][name], mirrors[name]._fields_
        if [f[2] for f in fields] != [f[0] for f in have]:
            out.append("struct %s: fields %s, binding %s" % (name, [f[2] for f in fields], [f[0] for f in have]))
            continue
        for (base, pointer, field, length), (_, ctype) in zip(fields, have):
            if length is not None:
                n = int(length) if length.isdigit() else binding_constants(B).get(length)
                if not (issubclass(ctype, ctypes.Array) and ctype._length_ == n):
                    out.append("struct %s: %s is an array of %s, binding %s" % (name, field, length, _name(ctype)))
                    continue
                ctype = ctype._type_
            elif issubclass(ctype, ctypes.Array):
                out.append("struct %s: %s is no array, binding %s" % (name, field, _name(ctype)))
                continue
            if ctype not in _allowed(base, pointer, B):
                out.append("struct %s: %s is %s%s, binding %s" % (name, field, base, "*" * pointer, _name(ctype)))
    return out


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "svae.h")) as f:
        return f.read()


def test_parser_sees_the_whole_header(header):
    H = parse_header(header)
    assert len(H["functions"]) == 36 and len(H["structs"]) == 7
    assert set(H["functions"]) == set(_binding().declared_in_header())
    assert H["functions"]["svae_abi_version"] == (("int", False), [])
    assert H["functions"]["svae_last_error"] == (("char", True), [])
    assert H["functions"]["svae_colsum"] == (("int", False), [("float", True, "x"), ("int32_t", False, "rows"), ("int32_t", False, "cols"),
                                                              ("float", True, "out"), ("svae_stream_t", False, "stream")])
    assert len(H["functions"]["svae_decoder_backward"][1]) == 14
    assert H["structs"]["svae_params"][4] == ("float", True, "hidden_w", "SVAE_MAX_HIDDEN")
    assert H["structs"]["svae_guard_control"][-3] == ("double", False, "norm_sum", None)
    assert H["constants"]["SVAE_LINEAR_ACT_NONE"] == -1 and H["constants"]["SVAE_E_LAUNCH"] == -3
    assert "SVAE_H" not in H["constants"] and len(H["constants"]) == 20


def test_binding_matches_the_header(header):
    B = _binding()
    assert compare(header, B) == []
    assert B.EXPORTS == tuple(B.SIGNATURES) and len(B.EXPORTS) == 36
    # svae_grads is svae_params without the const, which is what lets one mirror serve both
    structs = parse_header(header)["structs"]
    assert structs["svae_grads"] == structs["svae_params"]
    assert [f[0] for f in B.Grads._fields_] == [f[2] for f in structs["svae_grads"]]
    # the name tables draw on the constants
    consts = binding_constants(B)
    assert B.ACT == {k[len("SVAE_ACT_"):].lower(): v for k, v in consts.items() if k.startswith("SVAE_ACT_")}
    assert B.GEMM_MODE == {k[len("SVAE_GEMM_"):].lower(): v for k, v in consts.items() if k.startswith("SVAE_GEMM_")}
    from spatial_vae_amd import ops
    assert ops.ENC_ACT == {None: B.LINEAR_ACT_NONE, **B.ACT}


def test_loaded_library_carries_the_table():
    B = _binding()
    L = B.lib()
    for name, (restype, argtypes) in B.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


# ---------------------------------------------------------------- the headers added since: one rule for all of them
THIRTEEN = ["svae.h", "svae_stream.h", "svae_align.h", "svae_ctfcorr.h", "svae_cluster.h", "svae_frc.h", "svae_refine.h",
            "svae_classify.h", "svae_gmm.h", "svae_expect.h", "svae_pca.h", "svae_eigen.h", "svae_neighbours.h"]
# the file of csrc/ that holds a header's kernels, where it is not the header's name without its prefix
CSRC = {"svae_stream.h": "iw_stream.h", "svae_eigen.h": "eigen_images.h"}


def parse_added_header(name):
    """(path, parse_header of include/<name> without its #include "svae.h")."""
    path = os.path.join(ROOT, "include", name)
    with open(path) as f:
        return path, parse_header(f.read().replace('#include "svae.h"', ""))


def test_headers_is_the_one_list_in_the_order_the_headers_were_added():
    B = _binding()
    assert list(B.HEADERS) == THIRTEEN
    assert list(B.ALL_SIGNATURES) == [name for table in B.HEADERS.values() for name in table] and len(B.ALL_SIGNATURES) == 76


@pytest.mark.parametrize("name", THIRTEEN[1:])
def test_added_header_binding_matches_its_header(name):
    """What every header added to svae.h is held to (svae.h itself: compare() above).  The header declares exactly the functions
    of its table in _lib.HEADERS, which no other table has; return type and arguments agree type by type under the rules used
    for svae.h, a pointer to a struct the header declares itself being the address of a record in device memory (c_void_p); an
    entry point that takes a stream calls it `stream`; the loaded library carries the table; ops._POINTER_ARGS knows every name;
    the header and its file of csrc/ are files the library is built from, so an edit of either makes it stale.  The per-header
    files hold what is a header's own: the number of functions, constants, struct mirrors, argument names, pointer positions."""
    import sys

    import stream_cases
    from spatial_vae_amd import ops
    B = _binding()
    build = sys.modules["spatial_vae_amd.build"]        # the module: the package's attribute of that name is its build()
    table = B.HEADERS[name]
    path, H = parse_added_header(name)
    assert set(H["functions"]) == set(table) == set(B.declared_in_header(path)) and table
    assert all(not set(t) & set(table) for h, t in B.HEADERS.items() if h != name)
    takes_stream = set(stream_cases.stream_entry_points())
    for fn, ((rbase, rptr), args) in H["functions"].items():
        restype, argtypes = table[fn]
        assert restype in _allowed(rbase, rptr, B), fn
        assert len(args) == len(argtypes), fn
        for (base, pointer, arg), have in zip(args, argtypes):
            assert have in _allowed(base, pointer, B, device_record=base in H["structs"]), (fn, arg)
        assert (args[-1][2] == "stream") == (fn in takes_stream) if args else fn not in takes_stream, fn
    L = B.lib()
    for fn, (restype, argtypes) in table.items():
        have = getattr(L, fn)
        assert have.restype is restype and list(have.argtypes) == list(argtypes), fn
    assert L.svae_abi_version() == B.ABI_VERSION == 2
    assert set(table) <= set(ops._POINTER_ARGS)
    deps = build.dependencies()
    assert all(os.path.isfile(d) for d in deps)
    for needed in (path, os.path.join(ROOT, "spatial_vae_amd", "csrc", CSRC.get(name, name[len("svae_"):]))):
        assert any(os.path.samefile(needed, d) for d in deps), needed


@pytest.mark.parametrize("what, alter, named", [
    ("two arguments swapped", lambda t: t.replace("float eps, int64_t step, int32_t zero_grad", "int64_t step, float eps, int32_t zero_grad"),
     "function svae_adam_step:"),
    ("an int32_t widened", lambda t: t.replace("int svae_colsum(const float* x, int32_t rows", "int svae_colsum(const float* x, int64_t rows"),
     "function svae_colsum:"),
    ("a struct field removed", lambda t: t.replace("    int32_t mu_penalty;\n", ""), "struct svae_latent_desc:"),
    ("a constant changed", lambda t: t.replace("#define SVAE_PROF_KINDS 20", "#define SVAE_PROF_KINDS 24"), "constant SVAE_PROF_KINDS:"),
    ("a function added", lambda t: t.replace("int svae_abi_version(void);", "int svae_abi_version(void);\nint svae_new_thing(int32_t n);"),
     "function svae_new_thing:"),
    ("an array bound changed", lambda t: t.replace("#define SVAE_MAX_HIDDEN 7", "#define SVAE_MAX_HIDDEN 8"), "constant SVAE_MAX_HIDDEN:"),
    ("a device record passed by host pointer elsewhere", lambda t: t.replace("size_t svae_saved_bytes(const svae_desc* d);",
                                                                            "size_t svae_saved_bytes(const svae_guard_control* d);"),
     "function svae_saved_bytes:"),
])
def test_altered_header_is_caught(header, what, alter, named):
    altered = alter(header)
    assert altered != header, "the alteration (%s) did not apply: the header's text has moved on" % what
    found = compare(altered, _binding())
    assert found and all(line.startswith(named) for line in found), (what, found)


def test_call_helper_refuses_a_strided_tensor():
    """ops._call hands data_ptr() over as the header's contiguous row-major array; a strided view would be read as one."""
    from spatial_vae_amd import ops
    x = torch.zeros(4, 6).t()
    with pytest.raises(RuntimeError, match=r"svae_colsum was handed a non-contiguous tensor of shape \(6, 4\)"):
        ops._call("svae_colsum", torch.device("cpu"), x, 6, 4, torch.zeros(4))
