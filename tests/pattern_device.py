"""The device side that the GPU tests of the pattern ops (spmm, edge_softmax, edge_dot and the attention ops on K19, K20 and K21) share:
the device's pattern of a seeded case, the run of an op on a case's leaves, the spy that records launches, and the bodies of the
tests that are the same whatever the op.  What an op is (`_fused`, `_from_parts`) and what a test expects of it stay in its test
module.  pygat_amd is imported where it is used, so importing this module touches no device."""
import ctypes as C
import importlib

import numpy as np
import torch

DEV = "cuda:0"
# the launchers whose names more than one test module expects to see
FWD, ROWS, SPMM, SDDMM = "pygat_dot_attn_forward", "pygat_dot_attn_backward_rows", "pygat_spmm_forward", "pygat_spmm_grad_values"
BFWD, BROWS = "pygat_dot_attn_bias_forward", "pygat_dot_attn_bias_backward_rows"


def _graph(rowptr, col):
    import pygat_amd as pg
    return pg.CSRGraph(torch.as_tensor(np.asarray(rowptr), device=DEV), torch.as_tensor(np.asarray(col), device=DEV))


def _indices_pattern(row, col, shape):
    import pygat_amd as pg
    return pg.EdgePattern.from_indices(torch.stack([row, col]).to(DEV), shape)


def _pattern(c):
    if c.kind == "indices":
        pattern = _indices_pattern(c.row, c.col, c.shape)
        assert pattern.perm is not None
        return pattern
    pattern = _graph(*c.csr).edge_pattern()
    assert pattern.perm is None and torch.equal(pattern.edge_rc.cpu().long(), torch.stack([c.row, c.col], 1))
    return pattern


def to_leaves(tensors):
    return [t.float().to(DEV).requires_grad_(True) for t in tensors]


def leaves(c):
    return to_leaves(c.leaves)


def device_run(pattern, c, fn, leaves=None, **kw):
    """fn(pattern, c, **kw) is the op as a function of the case's leaves -> (out, the gradient of every leaf) on the device."""
    leaves = leaves or to_leaves(c.leaves)
    out = fn(pattern, c, **kw)(*leaves)
    assert out.dtype == torch.float32 and out.shape == c.G.shape and out.requires_grad
    return (out.detach(),) + torch.autograd.grad(out, leaves, c.G.float().to(DEV))


def _seed(value):
    """A dropout seed as the ops take it for graph capture: an int64 tensor of one element on the device."""
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def degree(c):
    return torch.bincount(c.row, minlength=c.shape[0])


def two_runs_bit_equal(c, run):
    """run(pattern, c) twice on one pattern: every output and gradient bit-equal, and priced -> the first run."""
    pattern = _pattern(c)
    runs = [run(pattern, c) for _ in range(2)]
    for p, q, what in zip(*runs, ["out"] + list(c.names)):
        assert torch.equal(p, q), what
    c.price(*runs[0])
    return runs[0]


def no_scratch(kernels, bad):
    """Every kernel of the list reports registers and no scratch; no name of `bad` is a kernel."""
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    for name in kernels:
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and regs.value > 0, (name, regs.value, scratch.value)
    for name in bad:
        assert lib.pygat_kernel_footprint(name, C.byref(regs), C.byref(scratch)) == -1, name


class _Spy:
    def __init__(self, real, seen):
        self._real, self._seen = real, seen

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("pygat_") or name == "pygat_last_error" or name.endswith("_workspace_bytes"):
            return fn

        def wrapped(*args):
            self._seen.append(name)
            return fn(*args)
        return wrapped


def spied(monkeypatch, *module_names):
    """-> the list that every pygat_ launch made through the `lib` of the named modules is appended to (by import path: the package
    attributes of these names are functions)."""
    seen = []
    for mod in module_names:
        m = importlib.import_module(mod)
        monkeypatch.setattr(m, "lib", _Spy(m.lib, seen))
    return seen
