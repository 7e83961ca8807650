"""The launchers of csrc/k18_edge_softmax.hip (additive under ABI 16) refuse bad arguments on the host, before anything is launched: no
GPU is needed, and a fake non-null address stands in for every device table (as in test_spmm_abi.py).  Also here, on the CPU: every
seeded case of tests/edge_softmax_case.py, the composition included, passes its pricing with the fp32 ground-truth run standing in
for the device."""
import ctypes as C
import os
import re

import pytest

import edge_softmax_case as case
from abi_support import P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_edge_softmax_workspace_bytes", "pygat_edge_softmax_rows", "pygat_edge_softmax_apply", "pygat_edge_softmax_grad_rows",
       "pygat_edge_softmax_grad_apply")


def _rows(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, perm=None, H=2, logits=P, m=P, Z=P, ws=P)
    a.update(kw)
    return L.lib.pygat_edge_softmax_rows(*a.values(), None)


def _apply(L, **kw):
    a = dict(nnz=20, edge_rc=P, side=0, H=2, logits=P, m=P, Z=P, alpha=P)
    a.update(kw)
    return L.lib.pygat_edge_softmax_apply(*a.values(), None)


def _grad_rows(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, perm=None, H=2, alpha=P, G=P, c=P, ws=P)
    a.update(kw)
    return L.lib.pygat_edge_softmax_grad_rows(*a.values(), None)


def _grad_apply(L, **kw):
    a = dict(nnz=20, edge_rc=P, side=1, H=2, alpha=P, G=P, c=P, dlogits=P)
    a.update(kw)
    return L.lib.pygat_edge_softmax_grad_apply(*a.values(), None)


LAUNCHERS = ((_rows, "edge_softmax_rows"), (_apply, "edge_softmax_apply"), (_grad_rows, "edge_softmax_grad_rows"),
             (_grad_apply, "edge_softmax_grad_apply"))


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    assert "K18" in header and "csrc/k18_edge_softmax.hip" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64 = C.c_void_p, C.c_int, C.c_int64
    assert lib.lib.pygat_edge_softmax_workspace_bytes.argtypes == [i64, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_edge_softmax_rows.argtypes == [i, i64, p, p, i, p, p, p, p, p]
    assert lib.lib.pygat_edge_softmax_apply.argtypes == [i64, p, i, i, p, p, p, p, p]
    assert lib.lib.pygat_edge_softmax_grad_rows.argtypes == [i, i64, p, p, i, p, p, p, p, p]
    assert lib.lib.pygat_edge_softmax_grad_apply.argtypes == [i64, p, i, i, p, p, p, p, p]


def test_exported_names():
    import pygat_amd as pg
    assert callable(pg.edge_softmax) and "edge_softmax" in pg.__all__


def test_workspace_bytes(lib):
    f = lib.edge_softmax_workspace_bytes
    # one record of (m, Z) per head -- 2 H floats -- per (2048-entry chunk, piece slot); the c records of the gradient fit in it
    assert f(20, 2) == 1 * 5 * 4 * 4
    assert f(2049, 3) == 2 * 5 * 6 * 4
    assert f(0, 1) == 5 * 2 * 4
    for bad, needle in (((-1, 2), "nnz"), ((1 << 31, 2), "2^31"), ((20, 0), "H=0"), ((20, 65), "H=65")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            f(*bad)
    assert lib.lib.pygat_edge_softmax_workspace_bytes(20, 2, None) == -1 and "null bytes" in _msg(lib)


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and name in _msg(lib), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own(lib):
    for fn, name in ((_apply, "edge_softmax_apply"), (_grad_apply, "edge_softmax_grad_apply")):
        for side in (-1, 2):
            assert fn(lib, side=side) == -1 and f"{name}: side={side}" in _msg(lib)
    for fn, name in ((_rows, "edge_softmax_rows"), (_grad_rows, "edge_softmax_grad_rows")):
        assert fn(lib, n_rows=-1) == -1 and f"{name}: n_rows=-1" in _msg(lib)
        assert fn(lib, n_rows=0) == -1 and f"{name}: n_rows=0 with nnz=20" in _msg(lib)
        assert fn(lib, ws=P + 4) == -1 and f"{name}: the workspace must be 16-byte aligned" in _msg(lib)
    # every pointer on its own: the message names the one that is null (perm may be null: the caller's order)
    for fn, name, pointers in ((_rows, "edge_softmax_rows", ("rowptr", "logits", "m", "Z", "ws")),
                               (_apply, "edge_softmax_apply", ("edge_rc", "logits", "m", "Z", "alpha")),
                               (_grad_rows, "edge_softmax_grad_rows", ("rowptr", "alpha", "G", "c", "ws")),
                               (_grad_apply, "edge_softmax_grad_apply", ("edge_rc", "alpha", "G", "c", "dlogits"))):
        for arg in pointers:
            want = f"{name}: null {'workspace' if arg == 'ws' else arg}"
            assert fn(lib, **{arg: None}) == -1 and _msg(lib) == want, (name, arg, _msg(lib))


def test_nothing_to_do_is_not_an_error(lib):
    """nnz == 0 launches nothing (no GPU here), whatever the pointers are."""
    for fn, name in LAUNCHERS:
        assert fn(lib, nnz=0) == 0, (name, _msg(lib))
    assert _rows(lib, nnz=0, rowptr=None, logits=None, m=None, Z=None, ws=None) == 0
    assert _grad_apply(lib, nnz=0, edge_rc=None, alpha=None, G=None, c=None, dlogits=None) == 0


def test_python_refusals_that_need_no_gpu():
    import torch
    import pygat_amd as pg
    with pytest.raises(ValueError, match="edge_softmax.*EdgePattern"):
        pg.edge_softmax(object(), torch.zeros(3))


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()


def test_composition_passes_with_the_fp32_reference():
    """The same rehearsal for the composition case: spmm(edge_softmax(logits), Wh) in fp32 in the device's place."""
    import torch
    from spmm_case import coo_of
    rowptr, col, x, W, a, logits, Wh, G = case.composition_inputs()
    leaves = [logits.float().requires_grad_(True), Wh.float().requires_grad_(True)]
    y = case.composition_ref(*coo_of(rowptr, col), len(rowptr) - 1)(*leaves)
    grads = torch.autograd.grad(y, leaves, G.float().reshape(-1))
    case.price_composition(y.detach(), grads, rowptr, col, logits, Wh, G)
