"""The launchers of csrc/k14_alpha_grad.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_attention_abi.py)."""
import ctypes as C

import pytest

from abi_support import P, lib, msg as _msg  # noqa: F401


def _rows(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, to_internal=None, H=2, Fo=16, alpha=0.2, s=P, t=P, m=P, Z=P, A=P, rec=P, ds2=P,
             part=P)
    a.update(kw)
    return L.lib.pygat_alpha_grad_rows(*a.values(), None)


def _cols(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, perm_t=P, to_internal=None, H=2, Fo=16, alpha=0.2, t=P, rec=P, A=P, dt2=P, part=P)
    a.update(kw)
    return L.lib.pygat_alpha_grad_cols(*a.values(), None)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    for s in ("pygat_alpha_grad_rows", "pygat_alpha_grad_cols", "pygat_alpha_grad_apply"):
        assert s in lib.SYMBOLS and getattr(lib.lib, s).restype is C.c_int
        assert "attention" not in s


@pytest.mark.parametrize("kw,needle", [
    (dict(n=0), "empty pattern"), (dict(nnz=0), "empty pattern"), (dict(H=0), "no heads"), (dict(H=65), "H=65"),
    (dict(A=None), "null rowptr / edge_rc / A"), (dict(rec=None), "rec"), (dict(rowptr=None), "null rowptr"),
    (dict(edge_rc=None), "edge_rc"), (dict(part=None), "part"),
    (dict(Fo=0), "F'=0"), (dict(Fo=300), "F'=300"), (dict(nnz=1 << 31), "int32"),
    (dict(A=P + 4), "A and rec must be 16-byte aligned"), (dict(edge_rc=P + 4), "edge_rc 8-byte aligned"),
])
def test_both_launchers_reject(lib, kw, needle):
    for fn in (_rows, _cols):
        assert fn(lib, **kw) == -1, (fn.__name__, kw)
        assert needle in _msg(lib), (fn.__name__, kw, _msg(lib))


@pytest.mark.parametrize("kw,needle", [(dict(ds2=None), "ds2"), (dict(s=None), "null s / t / m / Z"), (dict(t=None), "null s / t"),
                                       (dict(m=None), "m / Z"), (dict(Z=None), "m / Z")])
def test_row_launcher_rejects(lib, kw, needle):
    assert _rows(lib, **kw) == -1
    assert needle in _msg(lib) and "alpha_grad_rows" in _msg(lib), _msg(lib)


@pytest.mark.parametrize("kw,needle", [(dict(dt2=None), "dt2"), (dict(perm_t=None), "null perm_t / t"), (dict(t=None), "perm_t / t")])
def test_column_launcher_rejects(lib, kw, needle):
    assert _cols(lib, **kw) == -1
    assert needle in _msg(lib) and "alpha_grad_cols" in _msg(lib), _msg(lib)


def test_apply_rejects(lib):
    f = lib.lib.pygat_alpha_grad_apply
    assert f(0, 2, 16, P, P, P, P, None) == -1 and "n_rows=0" in _msg(lib)
    assert f(8, 2, 300, P, P, P, P, None) == -1 and "F'=300" in _msg(lib)
    assert f(8, 2, 16, P, P, P, None, None) == -1 and "dWh" in _msg(lib)
    assert f(8, 2, 16, P, P, P, P + 4, None) == -1 and "aligned" in _msg(lib)
