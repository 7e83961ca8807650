"""The launchers of csrc/k15_edge_logit.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_alpha_grad_abi.py)."""
import ctypes as C
import os
import re

import pytest

from abi_support import P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_gat_edge_workspace_bytes", "pygat_gat_edge_forward", "pygat_gat_edge_alpha", "pygat_gat_edge_backward_rows",
       "pygat_gat_edge_backward_cols")


def _fwd(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, H=2, Fo=16, alpha=0.2, flags=1, Wh=P, s=P, t=P, sk=None, u=P, u_rows=20, out=P,
             hattn=P, m=P, Z=P, ws=P)
    a.update(kw)
    return L.lib.pygat_gat_edge_forward(*a.values(), None)


def _att(L, **kw):
    a = dict(n=8, nnz=20, edge_rc=P, H=2, alpha=0.2, s=P, t=P, m=P, Z=P, u=P, u_rows=20, att=P)
    a.update(kw)
    return L.lib.pygat_gat_edge_alpha(*a.values(), None)


def _rows(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, H=2, Fo=16, alpha=0.2, flags=1, Wh=P, s=P, t=P, m=P, Z=P, u=P, u_rows=20, G=P, y=P,
             hattn=P, Gp=P, du=P, ds=P, ws=P)
    a.update(kw)
    return L.lib.pygat_gat_edge_backward_rows(*a.values(), None)


def _cols(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, perm_t=P, H=2, Fo=16, alpha=0.2, s=P, t=P, m=P, Z=P, u=P, u_rows=20, Gp=P, du=P, ds=P,
             a_pad=P, dt=P, dWh=P, ws=P)
    a.update(kw)
    return L.lib.pygat_gat_edge_backward_cols(*a.values(), None)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
    for s in NEW:
        assert getattr(lib.lib, s).restype is C.c_int      # (the size query too: it refuses bad sizes with a code and a message)


def test_workspace_bytes(lib):
    f = lib.edge_workspace_bytes
    # one record of H * Fp sums + (m, Z) per head (rounded to 16 bytes) per (2048-edge chunk, piece slot)
    assert f(20, 2, 16) == 1 * 5 * (2 * 16 + 4) * 4
    assert f(2049, 3, 7) == 2 * 5 * (3 * 8 + 8) * 4
    for bad in ((0, 2, 16), (20, 0, 16), (20, 2, 300)):
        with pytest.raises(ValueError, match="out of range"):
            f(*bad)
    assert lib.lib.pygat_gat_edge_workspace_bytes(20, 2, 16, None) == -1 and "null bytes" in _msg(lib)


@pytest.mark.parametrize("kw,needle", [
    (dict(n=0), "empty pattern"), (dict(nnz=0), "empty pattern"), (dict(H=0), "H=0"), (dict(Fo=0), "F'=0"), (dict(Fo=300), "F'=300"),
    (dict(H=8, Fo=256), "row too wide"), (dict(nnz=1 << 31, u_rows=1 << 31), "int32"), (dict(u=None), "null u"),
    (dict(u_rows=19), "u has 19 rows but the pattern has nnz = 20"), (dict(rowptr=None), "null rowptr"), (dict(edge_rc=None), "edge_rc"),
    (dict(ws=None), "workspace"), (dict(edge_rc=P + 4), "8-byte"), (dict(ws=P + 4), "16-byte aligned"),
])
def test_walking_launchers_reject(lib, kw, needle):
    for fn, name in ((_fwd, "gat_edge_forward"), (_rows, "gat_edge_backward_rows"), (_cols, "gat_edge_backward_cols")):
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and name in _msg(lib), (name, kw, _msg(lib))


def test_each_launcher_rejects_its_own(lib):
    assert _fwd(lib, Wh=None) == -1 and "null Wh" in _msg(lib)
    assert _fwd(lib, out=None) == -1 and "needs out" in _msg(lib)
    assert _fwd(lib, flags=3) == -1 and "needs sk" in _msg(lib)
    assert _fwd(lib, flags=4) == -1 and "flags 4" in _msg(lib)
    assert _fwd(lib, hattn=P + 4) == -1 and "aligned" in _msg(lib)
    assert _rows(lib, du=None) == -1 and "du" in _msg(lib)
    assert _rows(lib, y=None) == -1 and "saved output" in _msg(lib)
    assert _rows(lib, Gp=P + 8) == -1 and "aligned" in _msg(lib)
    assert _cols(lib, perm_t=None) == -1 and "perm_t" in _msg(lib)
    assert _cols(lib, dWh=None) == -1 and "dWh" in _msg(lib)
    assert _cols(lib, a_pad=P + 4) == -1 and "aligned" in _msg(lib)
    assert _att(lib, u=None) == -1 and "null u" in _msg(lib)
    assert _att(lib, u_rows=21) == -1 and "u has 21 rows" in _msg(lib)
    assert _att(lib, H=0) == -1 and "no heads" in _msg(lib)
    assert _att(lib, att=None) == -1 and "att" in _msg(lib)
