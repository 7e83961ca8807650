"""The attention launchers of ABI 16 (csrc/k13_attention.hip) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table."""
import ctypes as C

import pytest

from abi_support import P, lib, msg as _msg  # noqa: F401


def _v1(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, to_internal=None, H=2, Fo=16, alpha=0.2, Wh=P, ldwh=32, s=P, a_pad=P, m=P,
             Z=P, t_rows=8, t=P, att=P)
    a.update(kw)
    return L.lib.pygat_gat_attention(*a.values(), None)


def _v2(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, to_internal=None, H=2, Fo=16, alpha=0.2, WW=P, a2=P, m=P, Z=P, att=P)
    a.update(kw)
    return L.lib.pygat_gatv2_attention(*a.values(), None)


def test_abi_version_is_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    assert "pygat_gat_attention" in lib.SYMBOLS and "pygat_gatv2_attention" in lib.SYMBOLS


@pytest.mark.parametrize("kw,needle", [
    (dict(n=0), "empty pattern"), (dict(nnz=0), "empty pattern"), (dict(H=0), "no heads"),
    (dict(att=None), "null"), (dict(m=None), "null"), (dict(rowptr=None), "null"), (dict(edge_rc=None), "null"),
    (dict(Fo=0), "F'=0"), (dict(Fo=300), "F'=300"), (dict(nnz=1 << 31), "int32"),
    (dict(att=P + 4), "aligned"), (dict(edge_rc=P + 4), "aligned"),
])
def test_both_launchers_reject(lib, kw, needle):
    for fn in (_v1, _v2):
        assert fn(lib, **kw) == -1, (fn.__name__, kw)
        assert needle in _msg(lib), (fn.__name__, kw, _msg(lib))


@pytest.mark.parametrize("kw,needle", [
    (dict(t=None), "null Wh / s / a_pad / t"), (dict(Wh=None), "null Wh"), (dict(ldwh=16), "ld 16"), (dict(ldwh=34), "ld 34"),
    (dict(t_rows=9), "t_rows=9"), (dict(t_rows=-1), "t_rows=-1"),
])
def test_v1_launcher_rejects(lib, kw, needle):
    assert _v1(lib, **kw) == -1
    assert needle in _msg(lib), _msg(lib)


@pytest.mark.parametrize("H,Fo", [(8, 256), (5, 256), (2, 1000)])
def test_v2_launcher_rejects_wide_rows(lib, H, Fo):
    rc = _v2(lib, H=H, Fo=Fo)
    assert rc == -1
    if Fo <= 256:
        assert "row too wide" in _msg(lib) and f"{H} x 256" in _msg(lib)
    assert _v2(lib, WW=None) == -1 and "WW and a2" in _msg(lib)


def test_no_size_query_was_added(lib):
    """The v1 scratch size is stated in the header (n x H floats), not queried: every new export is a launcher."""
    new = [s for s in lib.SYMBOLS if "attention" in s]
    assert sorted(new) == ["pygat_gat_attention", "pygat_gatv2_attention"]
    for s in new:
        assert getattr(lib.lib, s).restype is C.c_int
