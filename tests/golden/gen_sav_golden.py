#!/usr/bin/env python3
"""Generate whole-module `.sav` fixtures by letting the REFERENCE construct and save tiny networks on CPU.

Same pattern as gen_golden.py: runs only where the reference tree is present, loads it read-only with the two absent
third-party imports stubbed, and writes DATA only.  Each network is saved exactly as MiscTools.save_trained_models does
(src/misc_tools.py:94-99: net.eval().cpu(); torch.save(net, path)) to tests/golden/sav_<name>.sav, and beside it
sav_<name>.npz holds the constructor arguments (JSON), the state-dict tensors ("sd.<key>"), the sorted key set of the
pickled __dict__ and, for the generators, a seeded input (x, z) with the reference's forward output y_hat.

A `.sav` is torch's zip container: data.pkl names classes and holds no source text.  check_is_data() asserts that for every
file written -- only the container's own members, only short dotted identifiers as strings, only torch / collections /
spatial_vae.models globals -- so nothing that is program text can reach tests/golden/.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_sav_golden.py
"""
import contextlib
import io
import json
import os
import pickletools
import re
import sys
import types
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"

# the repo root also holds a package called spatial_vae; make sure the reference wins
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != os.path.abspath(os.path.join(HERE, "..", ".."))]
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

for name in ("torchvision", "torchvision.utils", "torchvision.datasets", "skimage", "skimage.transform"):
    if name not in sys.modules:
        sys.modules[name] = types.ModuleType(name)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

import spatial_vae.models as ref_models  # noqa: E402  (the reference's, see sys.path above)

assert os.path.abspath(ref_models.__file__).startswith(REF), ref_models.__file__

ACT = {"tanh": nn.Tanh, "leakyrelu": nn.LeakyReLU, "relu": nn.ReLU, "sigmoid": nn.Sigmoid}
H, PIXELS = 8, 16

# name -> (class, positional arguments, keyword arguments; "activation" by name)
VARIANTS = [
    ("gen_tanh_L2", "SpatialGenerator", [2, H], dict(num_layers=2, activation="tanh")),
    ("gen_leaky_resid_bilinear_expand_L3", "SpatialGenerator", [3, H],
     dict(num_layers=3, activation="leakyrelu", resid=True, bilinear=True, expand_coords=True)),
    ("gen_z0", "SpatialGenerator", [0, H], dict(num_layers=2, activation="tanh")),
    ("gen_softplus_nout2", "SpatialGenerator", [2, H], dict(n_out=2, num_layers=2, activation="tanh", softplus=True)),
    ("gen_relu", "SpatialGenerator", [2, H], dict(num_layers=2, activation="relu")),
    ("gen_sigmoid", "SpatialGenerator", [2, H], dict(num_layers=2, activation="sigmoid")),
    ("inf_plain", "InferenceNetwork", [PIXELS, 5, H], dict(num_layers=2, activation="tanh")),
    ("inf_resid", "InferenceNetwork", [PIXELS, 5, H], dict(num_layers=3, activation="leakyrelu", resid=True)),
    ("vanilla", "VanillaGenerator", [PIXELS, 2, H], dict(num_layers=2, activation="tanh")),
]

_MEMBER = re.compile(r"^[^/]+/(data\.pkl|data/\d+|version|byteorder|\.format_version|\.storage_alignment|\.data/serialization_id)$")
_IDENT = re.compile(r"^[A-Za-z0-9_. ]*$")
_GLOBAL_ROOTS = ("torch", "collections", "spatial_vae.models")
_GLOBAL_EXTRA = ("__builtin__ set",)        # nn.Module keeps a set (_non_persistent_buffers_set); protocol 2 spells it so


def check_is_data(path):
    """The file is torch's zip container and its pickle names classes only: no member but the container's own, no string
    longer than 64 characters or outside [A-Za-z0-9_. ], no global outside torch / collections / spatial_vae.models (and the
    builtin set)."""
    with zipfile.ZipFile(path) as z:
        names = z.namelist()
        assert all(_MEMBER.match(n) for n in names), names
        pkl = z.read([n for n in names if n.endswith("/data.pkl")][0])
    longest = 0
    for op, arg, _ in pickletools.genops(pkl):
        if isinstance(arg, bytes):
            arg = arg.decode("latin-1")
        if isinstance(arg, str):
            assert len(arg) <= 64 and _IDENT.match(arg), (path, op.name, arg)
            longest = max(longest, len(arg))
            if op.name in ("GLOBAL", "STACK_GLOBAL"):
                assert arg.split(" ")[0].startswith(_GLOBAL_ROOTS) or arg in _GLOBAL_EXTRA, (path, arg)
    return longest


def main():
    total = 0
    for seed, (name, cls, pos, kw) in enumerate(VARIANTS):
        torch.manual_seed(1000 + seed)
        ctor = dict(kw, activation=ACT[kw["activation"]])
        with contextlib.redirect_stdout(io.StringIO()):             # the constructors print(self)
            net = getattr(ref_models, cls)(*pos, **ctor)
        path = os.path.join(HERE, "sav_%s.sav" % name)
        net.eval().cpu()
        torch.save(net, path)
        out = {"ctor": np.array(json.dumps({"cls": cls, "args": pos, "kwargs": kw})),
               "dict_keys": np.array(sorted(net.__dict__))}
        for k, v in net.state_dict().items():
            out["sd." + k] = v.detach().numpy().copy()
        if cls != "InferenceNetwork":
            rs = np.random.RandomState(seed)
            x = rs.uniform(-1, 1, size=(3, PIXELS, 2)).astype(np.float32)
            z = rs.normal(size=(3, pos[1] if cls == "VanillaGenerator" else pos[0])).astype(np.float32)
            with torch.no_grad():
                y_hat = net(torch.from_numpy(x), torch.from_numpy(z))
            out.update(x=x, z=z, y_hat=y_hat.numpy())
        np.savez_compressed(os.path.join(HERE, "sav_%s.npz" % name), **out)
        longest = check_is_data(path)
        size = os.path.getsize(path)
        total += size + os.path.getsize(os.path.join(HERE, "sav_%s.npz" % name))
        print("%-40s %6d bytes, longest string in data.pkl %d" % (name, size, longest))
    print("total bytes:", total)


if __name__ == "__main__":
    main()
