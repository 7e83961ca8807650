"""The launchers of csrc/k19_dot_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is launched: no
GPU is needed, and a fake non-null address stands in for every device table (as in test_spmm_abi.py).  Also here, on the CPU: every
seeded case of tests/dot_attention_case.py -- the composition from parts, the edge_dot cases and the module case included -- passes
its pricing with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import os
import re

import pytest

import dot_attention_case as case
from abi_support import DOT, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_dot_attn_workspace_bytes", "pygat_dot_attn_forward", "pygat_dot_attn_backward_rows")


LAUNCHERS = DOT
_forward, _backward = (fn for fn, _ in LAUNCHERS)
TABLES = {"dot_attn_forward": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo")),
          "dot_attn_backward_rows": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"), ("dq", "lddq"))}
SCALARS = {"dot_attn_forward": ("rowptr", "col", "m", "Z", "ws"), "dot_attn_backward_rows": ("rowptr", "col", "m", "Z", "P", "S", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    assert "K19" in header and "csrc/k19_dot_attention.hip" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert lib.lib.pygat_dot_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, i64, p,
                                                             i64, p, p, p, p]


def test_exported_names():
    import pygat_amd as pg
    for name in ("edge_dot", "dot_attention"):
        assert callable(getattr(pg, name)) and name in pg.__all__


def test_workspace_bytes(lib):
    f = lib.dot_attn_workspace_bytes
    # one record of (acc [H F], m [H], Z [H]), rounded up to 4 floats, per (2048-entry chunk, piece slot); the dq records fit in it
    assert f(20, 2, 8) == 1 * 5 * 20 * 4
    assert f(2049, 3, 8) == 2 * 5 * 32 * 4             # 24 + 6 = 30 floats -> 32
    assert f(0, 1, 4) == 5 * 8 * 4                     # 4 + 2 = 6 floats -> 8: never an empty workspace
    assert f(10_760_000, 8, 64) == -(-10_760_000 // 2048) * 5 * (512 + 16) * 4
    for bad, needle in (((-1, 2, 8), "nnz"), ((1 << 31, 2, 8), "2^31"), ((20, 0, 8), "H=0"), ((20, 65, 8), "H=65"), ((20, 2, 12), "F=12"),
                        ((20, 2, 512), "F=512"), ((20, 2, 3), "F=3"), ((20, 8, 256), "8 x 256")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            f(*bad)
    assert lib.lib.pygat_dot_attn_workspace_bytes(20, 2, 8, None) == -1 and "null bytes" in _msg(lib)


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and name in _msg(lib), (name, kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, F=12) == -1
        assert "power of two in 4..256" in _msg(lib) and "zero-padding the columns of q, k and v" in _msg(lib), _msg(lib)


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order)."""
    for fn, name in LAUNCHERS:
        for ptr, ld in TABLES[name]:
            assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == f"{name}: null {ptr}", (name, ptr, _msg(lib))
            assert fn(lib, **{ptr: P + 4}) == -1 and _msg(lib) == f"{name}: {ptr} must be 16-byte aligned", (name, ptr, _msg(lib))
            for short in (15, 12, 18):                                  # below H x F = 16; a stride that breaks the 16-byte rows
                assert fn(lib, **{ld: short}) == -1, (name, ld, short)
                assert f"the row stride of {ptr}, {short}," in _msg(lib) and name in _msg(lib), (name, ld, _msg(lib))
        for ptr in SCALARS[name]:
            want = f"{name}: null {'workspace' if ptr == 'ws' else ptr}"
            assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == want, (name, ptr, _msg(lib))
        assert fn(lib, ws=P + 8) == -1 and _msg(lib) == f"{name}: the workspace must be 16-byte aligned"


def test_python_refusals_that_need_no_gpu():
    import torch
    import pygat_amd as pg
    with pytest.raises(ValueError, match="dot_attention.*EdgePattern"):
        pg.dot_attention(object(), torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros(3, 4))
    with pytest.raises(ValueError, match="edge_dot.*EdgePattern"):
        pg.edge_dot(object(), torch.zeros(3, 4), torch.zeros(3, 4))


def test_the_cases_cover_what_they_are_meant_to():
    """Every lane shape on both patterns and both pattern kinds; a long row on the hub pattern; rows of one entry on the asymmetric and
    the lonely one; whole-number scores below 2^24 on the grid case; logits of std 3 on the sharp ones."""
    import torch
    cs = case.cases()
    for H, F in case.LANE_SHAPES:
        for pname in ("hub", "asym"):
            for kind in ("indices", "graph"):
                c = cs[f"lanes-{pname}-{H}x{F}-{kind}"]
                assert c.q.shape == (c.shape[0], H, F) and c.fed_scale is None
    assert cs["lanes-hub-noaxis-indices"].q.dim() == 2 and cs["lanes-asym-noaxis-graph"].q.dim() == 2
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    assert int(deg(cs["lanes-hub-8x16-graph"]).max()) == 699 and int((deg(cs["lanes-asym-8x16-graph"]) == 1).sum()) > 0
    assert int((deg(cs["lonely-8x16-graph"]) == 1).sum()) >= 12
    assert int((deg(cs["long-nine_hubs-8x16-graph"]) == 521).sum()) == 9 and int(deg(cs["long-three_chunk_hub-3x8-graph"]).max()) >= 4097
    s = cs["exact-hub-8x16-indices"].scores()
    assert torch.equal(s, s.round()) and 16 < float(s.abs().max()) < 2 ** 24 and cs["exact-hub-8x16-indices"].scale == 1.0
    for name in ("long-nine_hubs-8x16-graph", "long-three_chunk_hub-3x8-indices", "sharp-hub-4x256-indices"):
        s = cs[name].scores()
        assert 2.7 < float(s.std()) < 3.3 and float(s.max()) > 9.0, (name, float(s.std()), float(s.max()))
    assert max(c.shape[0] for c in cs.values()) <= 4500


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
