"""Child process of tests/test_gpu_loss_head.py: SVAE_CTF_LDS is read once per process, so the global-memory form of the CTF
likelihood (gaussian_kernel with a filter) needs a process of its own at sizes the LDS form would otherwise take.

    SVAE_CTF_LDS=0 python tests/loss_head_child.py ctf OUT.npz

runs ops.gaussian_loglik, with the circular mask and with dll, on the random and the integer inputs of every (n, k) of
ref64.CTF_BOTH_FORMS and writes loglik / dll per case into OUT.npz (keys '<kind>_<n>_<k>_loglik' / '_dll').  Prints one JSON
line: the cases written and the value of SVAE_CTF_LDS it ran under."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ref64  # noqa: E402


def run_ctf(img, tgt, f, mask, want_dll=True):
    """(loglik, dll | None) of ops.gaussian_loglik for CPU numpy inputs, as float32 numpy arrays."""
    from spatial_vae_amd import ops
    dev = torch.device("cuda:0")
    y = torch.from_numpy(img).to(dev).requires_grad_(want_dll)
    m = None if mask is None else torch.from_numpy(np.asarray(mask)).to(dev)
    k = f.shape[-1]
    ll = ops.gaussian_loglik(y, torch.from_numpy(tgt).to(dev), m, torch.from_numpy(f).to(dev).view(-1, 1, k, k))
    dll = None
    if want_dll:
        ll.sum().backward()          # the upstream gradient is exactly 1: y.grad is the kernel's dll, bit for bit
        dll = y.grad.cpu().numpy()
    return ll.detach().cpu().numpy(), dll


def ctf(out_path):
    res = {}
    for n, k in ref64.CTF_BOTH_FORMS:
        for kind, make in (("random", ref64.ctf_inputs_random), ("integer", ref64.ctf_inputs_integer)):
            img, tgt, f = make(n, k)
            ll, dll = run_ctf(img, tgt, f, ref64.ctf_mask(n, True))
            res["%s_%d_%d_loglik" % (kind, n, k)] = ll
            res["%s_%d_%d_dll" % (kind, n, k)] = dll
    np.savez(out_path, **res)
    print(json.dumps({"cases": sorted(res), "SVAE_CTF_LDS": os.environ.get("SVAE_CTF_LDS")}))


if __name__ == "__main__":
    {"ctf": ctf}[sys.argv[1]](*sys.argv[2:])
