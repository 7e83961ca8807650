"""The entry points of csrc/k16_bf16_forward.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_edge_logit_abi.py)."""
import ctypes as C
import os
import re

import pytest

from abi_support import P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_gat_bf16_workspace_bytes", "pygat_gat_pack_bf16", "pygat_gat_forward_bf16")


def _graph(L, **kw):
    a = dict(n=8, nnz=20, rowptr=P, edge_rc=P, slot_edges=4, slot_begin=None, cut_rows=None, n_cut=0, n_cut_wide=0, slot_first=0,
             slot_count=0, slot_meta=None, slot_order=None, user_row=None)
    a.update(kw)
    return L.Graph(*a.values())


def _pack(L, **kw):
    a = dict(n=8, H=2, Fo=16, Wh=P, ldwh=32, a_pad=P, Whq=P, s=P)
    a.update(kw)
    return L.lib.pygat_gat_pack_bf16(*a.values(), None)


def _fwd(L, g=None, **kw):
    g = g if g is not None else _graph(L)
    a = dict(H=2, Fo=16, alpha=0.2, flags=1, Whq=P, s=P, a_pad=P, sk=None, out=P, hattn=None, head_group=0, part=P)
    a.update(kw)
    return L.lib.pygat_gat_forward_bf16(C.byref(g) if g != "null" else None, *a.values(), None)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert "attention" not in s
        assert getattr(lib.lib, s).restype is C.c_int      # (the size query too: it refuses bad sizes with a code and a message)


def test_workspace_bytes(lib):
    f = lib.bf16_workspace_bytes
    # two records per slot: H * Fp sums + (m, Z) per head, rounded up to 16 bytes
    assert f(20, 4, 2, 16) == 2 * 5 * (2 * 16 + 4) * 4
    assert f(1000, 64, 3, 7) == 2 * 16 * (3 * 8 + 8) * 4
    for bad in ((0, 4, 2, 16), (20, 0, 2, 16), (20, 6, 2, 16), (20, 4, 0, 16), (20, 4, 2, 300)):
        with pytest.raises(ValueError, match="out of range"):
            f(*bad)
    assert lib.lib.pygat_gat_bf16_workspace_bytes(20, 4, 2, 16, None) == -1 and "null bytes" in _msg(lib)
    assert lib.lib.pygat_gat_bf16_workspace_bytes(0, 0, 0, 0, None) == -1


@pytest.mark.parametrize("kw,needle", [
    (dict(Wh=None), "null Wh"), (dict(a_pad=None), "null Wh"), (dict(Whq=None), "null Wh"), (dict(s=None), "null Wh"),
    (dict(n=0), "n=0 rows"), (dict(H=0), "H=0 heads"), (dict(Fo=0), "F'=0"), (dict(Fo=257), "F'=257"),
    (dict(ldwh=16), "ldwh=16"), (dict(ldwh=34), "ldwh=34"), (dict(Whq=P + 8), "16-byte aligned"), (dict(Wh=P + 4), "16-byte aligned"),
    (dict(n=(1 << 31) - 1, H=256, Fo=256, ldwh=1 << 16), "too wide for one pass"),
])
def test_pack_rejects(lib, kw, needle):
    assert _pack(lib, **kw) == -1, kw
    assert needle in _msg(lib) and "gat_pack_bf16" in _msg(lib), (kw, _msg(lib))


@pytest.mark.parametrize("kw,needle", [
    (dict(Whq=None), "null Whq"), (dict(s=None), "null Whq"), (dict(a_pad=None), "null Whq"), (dict(part=None), "null Whq"),
    (dict(out=None), "need out and/or hattn"), (dict(flags=3), "PYGAT_F_SKIP without sk"), (dict(flags=4), "flags 4"),
    (dict(H=0), "H=0 heads"), (dict(Fo=0), "F'=0"), (dict(Fo=257), "F'=257"),
    (dict(Whq=P + 8), "16-byte aligned"), (dict(part=P + 4), "16-byte aligned"), (dict(out=P + 4), "16-byte aligned"),
    (dict(H=12, Fo=128, head_group=9), "head_group=9"), (dict(H=8, Fo=256, head_group=8), "head_group=8"),
    (dict(H=100, Fo=3, head_group=65), "head_group=65"), (dict(head_group=-1), "head_group=-1"),
])
def test_forward_rejects(lib, kw, needle):
    assert _fwd(lib, **kw) == -1, kw
    assert needle in _msg(lib) and "gat_forward_bf16" in _msg(lib), (kw, _msg(lib))


def test_forward_rejects_its_graph(lib):
    assert _fwd(lib, g="null") == -1 and "null graph" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, user_row=P)) == -1 and "row map" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, slot_first=0, slot_count=2)) == -1 and "slot range" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, nnz=1 << 31)) == -1 and "int32" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, slot_edges=6)) == -1 and "slot_edges" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, rowptr=None)) == -1 and "graph" in _msg(lib)
    assert _fwd(lib, g=_graph(lib, slot_meta=P + 4)) == -1 and "slot_meta" in _msg(lib)
