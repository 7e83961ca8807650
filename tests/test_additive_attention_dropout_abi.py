"""The two dropout launchers of csrc/k20_additive_attention.hip (additive under ABI 16) refuse bad arguments on the host, before
anything is launched: no GPU is needed, and a fake non-null address stands in for every device table.  Also here, on the CPU: the
signature of pygat_amd.additive_attention_dropout and its refusals that need no GPU, what the seeded cases of
tests/additive_attention_dropout_case.py cover -- asserted from the NumPy mask of tests/philox_ref.py -- and every such case's rehearsal
with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import additive_attention_dropout_case as case
import dot_attention_dropout_case as dot_case
import philox_ref
from abi_support import ADDITIVE, P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_add_attn_dropout_forward", "pygat_add_attn_dropout_backward_rows")


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, s_dst=P, s_src=P, v=P, ldv=16, edge_logit=P + 4,
             logit_head_stride=1, p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, ws=P)
    return call(L, "pygat_add_attn_dropout_forward", a, **kw)


def _backward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, s_dst=P, s_src=P, v=P, ldv=16, edge_logit=P + 4,
             logit_head_stride=1, p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, ds_dst=P, P=P, S=P, ws=P)
    return call(L, "pygat_add_attn_dropout_backward_rows", a, **kw)


LAUNCHERS = ((_forward, "add_attn_dropout_forward"), (_backward, "add_attn_dropout_backward_rows"))
TABLES = {"add_attn_dropout_forward": (("v", "ldv"), ("out", "ldo")),
          "add_attn_dropout_backward_rows": (("v", "ldv"), ("out", "ldo"), ("G", "ldg"))}
SCALARS = {"add_attn_dropout_forward": ("rowptr", "col", "s_dst", "s_src", "m", "Z", "ws"),
           "add_attn_dropout_backward_rows": ("rowptr", "col", "s_dst", "s_src", "m", "Z", "ds_dst", "P", "S", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert "attention" not in s and "dot_attn" not in s
    p, i, i64, f, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
    assert lib.lib.pygat_add_attn_dropout_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, f, p, u32, p, i64, p, p, p, p]
    assert lib.lib.pygat_add_attn_dropout_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, f, p, u32, p, i64, p, p,
                                                                     p, i64, p, p, p, p, p]
    # the K20 launchers before these keep their signatures, as do K19's and K21's, and the size query is theirs
    assert lib.lib.pygat_add_attn_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, p]
    assert lib.lib.pygat_add_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, i64, p, p, p, p, p]
    assert lib.lib.pygat_dot_attn_dropout_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, f, p, u32, p, i64, p,
                                                               p, p, p]
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_dot_attn_backward_rows.argtypes) == 26 and len(lib.lib.pygat_dot_attn_dropout_backward_rows.argtypes) == 32
    assert lib.lib.pygat_v2_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_v2_attn_backward_rows.argtypes) == 27 and len(lib.lib.pygat_v2_attn_backward_cols.argtypes) == 19
    assert [s for s in lib.SYMBOLS if "add_attn" in s and s.endswith("workspace_bytes")] == ["pygat_add_attn_workspace_bytes"]
    from pygat_amd.dropout import STREAM_ATT
    assert case.STREAM_ATT == STREAM_ATT == dot_case.STREAM_ATT


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(nnz=1 << 31), "2^31"),
                                       (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"), (dict(n_rows=0), "n_rows=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "a finite slope expected")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order; edge_logit may be null: no term, and its head stride is then not looked at)."""
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
        for stride in (2, -1, 8):
            assert fn(lib, logit_head_stride=stride) == -1, (name, stride)
            assert _msg(lib).startswith(f"{name}: logit_head_stride={stride},"), (name, _msg(lib))
        # a null perm and a null logit are no refusal: with everything else in order the next refusal is the seed's
        assert fn(lib, perm=None, edge_logit=None, logit_head_stride=7, seed=None) == -1 and _msg(lib) == f"{name}: null seed"


def test_the_same_wording_as_the_parent_pair(lib):
    """Whatever pygat_add_attn_forward / _backward_rows refuse, the dropout launchers refuse in the same words after their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS, ADDITIVE):
        for kw in (dict(H=65), dict(F=12), dict(nnz=-1), dict(n_rows=0), dict(s_dst=None), dict(v=P + 4), dict(ldv=12), dict(m=None),
                   dict(ws=None), dict(ws=P + 8), dict(col=None), dict(logit_head_stride=2), dict(out=None), dict(negative_slope=float("nan"))):
            assert fn(lib, **kw) == -1
            mine = _msg(lib)
            assert pfn(lib, **kw) == -1
            assert mine[len(name):] == _msg(lib)[len(pname):] and mine.startswith(name), (kw, mine, _msg(lib))


def test_a_null_seed_and_a_bad_p_are_refused(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, seed=None) == -1 and _msg(lib) == f"{name}: null seed", (name, _msg(lib))
        assert fn(lib, seed=P + 4) == -1 and _msg(lib) == f"{name}: seed must be 8-byte aligned", (name, _msg(lib))
        for p in (-0.1, 1.5, float("nan"), -1e-9, 1.0 + 1e-6, float("inf")):
            assert fn(lib, p=p) == -1, (name, p)
            assert _msg(lib).startswith(f"{name}: p=") and _msg(lib).endswith("outside [0, 1]"), (name, p, _msg(lib))
        # the parent's refusals come first, whatever p and the seed are
        assert fn(lib, p=2.0, seed=None, H=65) == -1 and "H=65" in _msg(lib)
        # and with every pointer null and every scalar 0
        n_args = len(getattr(lib.lib, "pygat_" + name).argtypes)
        assert getattr(lib.lib, "pygat_" + name)(*([0] * n_args)) < 0 and _msg(lib).startswith(name + ": ")


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    pattern.n_rows = pattern.n_cols = 3
    return pattern


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    assert "additive_attention_dropout" in pg.__all__ and "additive_attention" in pg.__all__
    sig = inspect.signature(pg.additive_attention_dropout)
    assert list(sig.parameters) == ["pattern", "s_dst", "s_src", "v", "p", "negative_slope", "edge_logit", "seed", "generator", "training"]
    for name in ("seed", "generator", "training"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["edge_logit"].default is None
    assert sig.parameters["seed"].default is None and sig.parameters["generator"].default is None
    assert sig.parameters["training"].default is True and sig.parameters["p"].default is inspect.Parameter.empty
    assert list(inspect.signature(pg.additive_attention).parameters) == ["pattern", "s_dst", "s_src", "v", "negative_slope", "edge_logit"]
    doc = pg.additive_attention.__doc__
    for absent in ("dropout", "bfloat16", "fused column pass", "additive_attention_dropout"):
        assert absent in doc[doc.index("Not provided"):], absent
    s, v = torch.zeros(3, 4), torch.zeros(3, 4, 8)
    pattern = _fake_pattern()
    for p in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"additive_attention_dropout: p = .*\[0, 1\]"):
            pg.additive_attention_dropout(pattern, s, s, v, p)
    for args in ((s.bfloat16(), s, v), (s, s, v.bfloat16())):
        with pytest.raises(ValueError, match="additive_attention_dropout: .* must be float32: there is no training path on bfloat16"):
            pg.additive_attention_dropout(pattern, *args, 0.5)
    for seed in (5, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), [1]):
        with pytest.raises(ValueError, match="additive_attention_dropout: seed must be an int64 tensor of shape \\[1\\] on the pattern's device"):
            pg.additive_attention_dropout(pattern, s, s, v, 0.5, seed=seed)        # (a CPU tensor is on the wrong device)
    with pytest.raises(ValueError, match="additive_attention_dropout: negative_slope = nan"):
        pg.additive_attention_dropout(pattern, s, s, v, 0.5, float("nan"))
    # what additive_attention refuses, under this op's name -- whether or not the dropout kernels would run
    for kw in (dict(), dict(training=False)):
        for p in (0.5, 0.0):
            with pytest.raises(ValueError, match="additive_attention_dropout: an EdgePattern expected"):
                pg.additive_attention_dropout(object(), s, s, v, p, **kw)
            with pytest.raises(ValueError, match="additive_attention_dropout: s_dst must be a tensor on the GPU"):
                pg.additive_attention_dropout(pattern, s, s, v, p, **kw)
            with pytest.raises(ValueError, match="additive_attention_dropout: edge_logit must be a tensor on the GPU"):
                pg.additive_attention_dropout(pattern, s, s, v, p, edge_logit=torch.zeros(3), **kw)


# ------------------------------------------------------------------------------------------------------- what the cases cover
def _deg(c):
    return torch.bincount(c.row, minlength=c.shape[0])


def test_the_mask_of_a_case_is_the_flat_layout():
    c = case.cases()["lanes-hub-3x8-indices-plain"]
    E = c.row.numel()
    thresh, scale = philox_ref.threshold(0.5)
    words = dot_case.flat_words(c.seed, E * 3)
    assert float(scale) == 2.0
    assert np.array_equal(np.where(words < np.uint32(thresh), np.float32(2.0), np.float32(0.0)).reshape(E, 3), c.mask.numpy())
    assert 0.45 < float((c.mask != 0).float().mean()) < 0.55


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            plain, u = cs[f"lanes-hub-{H}x{F}-{kind}-plain"], cs[f"lanes-hub-{H}x{F}-{kind}-logit"]
            assert plain.u is None and u.u.shape == (u.row.numel(), H) and plain.kind == u.kind == kind and plain.p == u.p == 0.5
            assert plain.v.shape == (plain.shape[1], H, F) and plain.seed != u.seed
    assert cs["lanes-hub-12x64-indices-shared"].u.dim() == 1 and cs["lanes-hub-noaxis-graph-logit"].s_dst.dim() == 1
    assert int(_deg(cs["lanes-hub-8x16-graph-plain"]).max()) == 699 and int((_deg(cs["lanes-asym-8x16-indices-plain"]) == 1).sum()) > 0
    assert {cs[n].p for n in case.case_names("long-")} == {0.5, 0.9}
    assert {(cs[n].H, cs[n].F) for n in case.case_names("long-")} == {(3, 8), (8, 16), (12, 64)}
    for name in case.case_names("long-"):
        assert int(_deg(cs[name]).max()) > 512 and cs[name].p == float(name.rsplit("-p", 1)[1]), name
    assert int(_deg(cs["long-three_chunk_hub-3x8-graph-p0.5"]).max()) >= 4097
    # rows of at least two entries, all of them dropped: the exact-zero check cannot pass vacuously
    for name in case.case_names("gone-"):
        assert cs[name].p == 0.9 and int(cs[name].all_dropped().sum()) >= 5, name
    for name in ("rect-4x16-plain", "rect-3x8-logit", "repeats-8x16-plain", "masked-rect-3x8") + tuple(case.case_names("single-")):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation finds the mask"
    c = cs["repeats-8x16-plain"]
    assert torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]]) and torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])
    assert bool((c.mask[c.pairs[:, 0]] != c.mask[c.pairs[:, 1]]).any()), "the two entries of a repeated pair draw their own decisions"
    for name in case.case_names("masked-"):
        c = cs[name]
        E = c.row.numel()
        assert 0.2 * E < int(c.masked.sum()) < 0.4 * E and bool((c.u[c.masked] == case.base.MASK).all())
        assert bool(((c.mask[c.masked] != 0).any(1)).any()), "a masked entry that the dropout keeps: still an exact zero"
    for name in case.case_names("single-"):
        c = cs[name]
        assert bool((_deg(c) == 1).all()) and c.shape == (300, 400) and c.p == 0.5
        assert bool((c.mask == 0).any(0).all()) and bool((c.mask == 2).any(0).all())
    thresh, scale = philox_ref.threshold(case.P_NEAR_0)
    assert thresh == 0xFFFFFFFF and float(scale) == 1.0
    for name in case.case_names("near0-"):
        c = cs[name]
        assert c.p == case.P_NEAR_0 and bool((c.mask == 1).all())
        assert not bool((dot_case.flat_words(c.seed, c.row.numel() * c.H) == np.uint32(0xFFFFFFFF)).any()), name
    for name in case.case_names("zero-"):
        assert float(cs[name].u.abs().max()) == 0.0
    m = cs["module-rect-4x8"]
    assert m.mask.shape == (m.row.numel(), m.H) and m.p == 0.5
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
