"""The launchers of csrc/k17_spmm.hip (additive under ABI 16) refuse bad arguments on the host, before anything is launched: no GPU
is needed, and a fake non-null address stands in for every device table (as in test_edge_logit_abi.py)."""
import ctypes as C
import os
import re

import pytest

from abi_support import P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_spmm_workspace_bytes", "pygat_spmm_forward", "pygat_spmm_grad_values")


def _fwd(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=16, val=P, b=P, ldb=32, out=P, ldo=32, ws=P)
    a.update(kw)
    return L.lib.pygat_spmm_forward(*a.values(), None)


def _gv(L, **kw):
    a = dict(nnz=20, edge_rc=P, H=2, F=16, G=P, ldg=32, b=P, ldb=32, dval=P)
    a.update(kw)
    return L.lib.pygat_spmm_grad_values(*a.values(), None)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int


def test_exported_names():
    import pygat_amd as pg
    from pygat_amd import graph
    for name in ("EdgePattern", "spmm", "SpecialSpmmFunction", "SpecialSpmm", "clear_pattern_cache"):
        assert hasattr(pg, name) and name in pg.__all__, name
    assert callable(graph.CSRGraph.edge_pattern)
    assert callable(pg.EdgePattern.from_indices)


def test_workspace_bytes(lib):
    f = lib.spmm_workspace_bytes
    # one record of H * F sums (rounded to 16 bytes) per (2048-entry chunk, piece slot)
    assert f(20, 2, 16) == 1 * 5 * 32 * 4
    assert f(2049, 3, 7) == 2 * 5 * 24 * 4
    assert f(0, 1, 1) == 5 * 4 * 4
    for bad, needle in (((-1, 2, 16), "nnz"), ((1 << 31, 2, 16), "2^31"), ((20, 0, 16), "H=0"), ((20, 65, 4), "H=65"),
                        ((20, 2, 0), "F=0"), ((20, 4, 257), "4 x 257 > 1024")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            f(*bad)
    assert lib.lib.pygat_spmm_workspace_bytes(20, 2, 16, None) == -1 and "null bytes" in _msg(lib)


@pytest.mark.parametrize("kw,needle", [
    (dict(H=0), "H=0"), (dict(H=65, F=1), "H=65"), (dict(F=0), "F=0"), (dict(H=4, F=257), "4 x 257 > 1024"), (dict(nnz=1 << 31), "2^31"),
    (dict(nnz=-1), "nnz"),
])
def test_both_launchers_refuse_the_limits(lib, kw, needle):
    for fn, name in ((_fwd, "spmm_forward"), (_gv, "spmm_grad_values")):
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and name in _msg(lib), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own(lib):
    assert _fwd(lib, n_rows=-1) == -1 and "n_rows" in _msg(lib)
    assert _fwd(lib, ldb=31) == -1 and "ldb=31" in _msg(lib)
    assert _fwd(lib, ldo=8) == -1 and "ldo=8" in _msg(lib)
    assert _fwd(lib, rowptr=None) == -1 and "rowptr" in _msg(lib)
    assert _fwd(lib, out=None) == -1 and "out" in _msg(lib)
    assert _fwd(lib, ws=None) == -1 and "workspace" in _msg(lib)
    assert _fwd(lib, col=None) == -1 and "col" in _msg(lib)
    assert _fwd(lib, val=None) == -1 and "val" in _msg(lib)
    assert _fwd(lib, ws=P + 4) == -1 and "16-byte aligned" in _msg(lib)
    assert _gv(lib, ldg=31) == -1 and "ldg=31" in _msg(lib)
    assert _gv(lib, edge_rc=None) == -1 and "edge_rc" in _msg(lib)
    assert _gv(lib, dval=None) == -1 and "dval" in _msg(lib)
    assert _gv(lib, edge_rc=P + 4) == -1 and "8-byte" in _msg(lib)
    # nothing to do is not an error, and launches nothing
    assert _fwd(lib, n_rows=0) == 0 and _gv(lib, nnz=0) == 0
