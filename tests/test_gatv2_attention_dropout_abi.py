"""The two dropout launchers of csrc/k21_gatv2_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything
is launched: no GPU is needed, and a fake non-null address stands in for every device table.  Also here, on the CPU: the signature of
pygat_amd.gatv2_attention_dropout and its refusals that need no GPU, what the seeded cases of tests/gatv2_attention_dropout_case.py
cover -- asserted from the NumPy mask of tests/philox_ref.py -- and every such case's rehearsal with the fp32 ground-truth run standing
in for the device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dot_attention_dropout_case as dot_case
import gatv2_attention_dropout_case as case
import philox_ref
from abi_support import GATV2, P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_v2_attn_dropout_forward", "pygat_v2_attn_dropout_backward_rows")


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P, lds=16, a=P, v=P, ldv=16,
             p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, ws=P)
    return call(L, "pygat_v2_attn_dropout_forward", a, **kw)


def _backward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=P, lds=16, a=P, v=P,
             ldv=16, p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dx_dst=P, lddx=16, P=P, S=P, ws=P)
    return call(L, "pygat_v2_attn_dropout_backward_rows", a, **kw)


LAUNCHERS = ((_forward, "v2_attn_dropout_forward"), (_backward, "v2_attn_dropout_backward_rows"))
TABLES = {"v2_attn_dropout_forward": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo")),
          "v2_attn_dropout_backward_rows": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"),
                                            ("dx_dst", "lddx"))}
SCALARS = {"v2_attn_dropout_forward": ("rowptr", "col", "a", "m", "Z", "ws"),
           "v2_attn_dropout_backward_rows": ("rowptr", "col", "a", "m", "Z", "P", "S", "ws")}


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
    # the K21 lists with (p, seed, stream_id) after (v, ldv); the forward takes perm after col
    assert lib.lib.pygat_v2_attn_dropout_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, f, p, u32, p, i64, p, p,
                                                              p, p]
    assert lib.lib.pygat_v2_attn_dropout_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, f, p, u32, p, i64,
                                                                    p, p, p, i64, p, i64, p, p, p, p]
    # the K21 launchers before these keep their signatures, as do K19's and K20's; no new size query
    assert lib.lib.pygat_v2_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, i64, p, i64,
                                                            p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_cols.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, p, i64, p, p, p]
    assert lib.lib.pygat_add_attn_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_add_attn_backward_rows.argtypes) == 25
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_dot_attn_dropout_forward.argtypes) == 25 and len(lib.lib.pygat_dot_attn_dropout_backward_rows.argtypes) == 32
    assert [s for s in lib.SYMBOLS if "v2_attn" in s and s.endswith("workspace_bytes")] == ["pygat_v2_attn_workspace_bytes"]
    assert not any("v2_attn_dropout_backward_cols" in s for s in lib.SYMBOLS), "the column pass reads S alone: no dropout variant"
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
    caller's order; v may be null: v is x_src)."""
    for fn, name in LAUNCHERS:
        for ptr, ld in TABLES[name]:
            if ptr != "v":
                assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == f"{name}: null {ptr}", (name, ptr, _msg(lib))
            assert fn(lib, **{ptr: P + 4}) == -1 and _msg(lib) == f"{name}: {ptr} must be 16-byte aligned", (name, ptr, _msg(lib))
            for short in (15, 12, 18):                                  # below H x F = 16; a stride that breaks the 16-byte rows
                assert fn(lib, **{ld: short}) == -1, (name, ld, short)
                assert f"the row stride of {ptr}, {short}," in _msg(lib) and name in _msg(lib), (name, ld, _msg(lib))
        for ptr in SCALARS[name]:
            want = f"{name}: null {'workspace' if ptr == 'ws' else ptr}"
            assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == want, (name, ptr, _msg(lib))
        assert fn(lib, ws=P + 8) == -1 and _msg(lib) == f"{name}: the workspace must be 16-byte aligned"
        assert fn(lib, a=P + 4) == -1 and _msg(lib) == f"{name}: a must be 16-byte aligned"
        # a null perm and a null v are no refusal: with everything else in order the next refusal is the seed's
        assert fn(lib, perm=None, v=None, ldv=0, seed=None) == -1 and _msg(lib) == f"{name}: null seed"


def test_the_same_wording_as_the_parent_pair(lib):
    """Whatever pygat_v2_attn_forward / _backward_rows refuse, the dropout launchers refuse in the same words after their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS, GATV2[:2]):
        for kw in (dict(H=65), dict(F=12), dict(nnz=-1), dict(n_rows=0), dict(x_dst=None), dict(x_src=P + 4), dict(ldv=12), dict(m=None),
                   dict(ws=None), dict(ws=P + 8), dict(col=None), dict(a=None), dict(out=None), dict(lds=15),
                   dict(negative_slope=float("nan"))):
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
    assert "gatv2_attention_dropout" in pg.__all__ and "gatv2_attention" in pg.__all__
    sig = inspect.signature(pg.gatv2_attention_dropout)
    assert list(sig.parameters) == ["pattern", "x_dst", "x_src", "a", "p", "v", "negative_slope", "seed", "generator", "training"]
    for name in ("seed", "generator", "training"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["v"].default is None
    assert sig.parameters["seed"].default is None and sig.parameters["generator"].default is None
    assert sig.parameters["training"].default is True and sig.parameters["p"].default is inspect.Parameter.empty
    assert list(inspect.signature(pg.gatv2_attention).parameters) == ["pattern", "x_dst", "x_src", "a", "v", "negative_slope"]
    doc = " ".join(pg.gatv2_attention.__doc__.split())
    for absent in ("a per-entry term or edge features", "dropout on the coefficients", "bfloat16 tables",
                   "the value product fused into the column pass", "gatv2_attention_dropout"):
        assert absent in doc[doc.index("Not provided"):], absent
    x, a = torch.zeros(3, 4, 8), torch.zeros(4, 8)
    pattern = _fake_pattern()
    for p in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"gatv2_attention_dropout: p = .*\[0, 1\]"):
            pg.gatv2_attention_dropout(pattern, x, x, a, p)
    for args, kw in (((x.bfloat16(), x, a), {}), ((x, x, a.bfloat16()), {}), ((x, x, a), dict(v=x.bfloat16()))):
        with pytest.raises(ValueError, match="gatv2_attention_dropout: .* must be float32: there is no training path on bfloat16"):
            pg.gatv2_attention_dropout(pattern, *args, 0.5, **kw)
    for seed in (5, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), [1]):
        with pytest.raises(ValueError, match="gatv2_attention_dropout: seed must be an int64 tensor of shape \\[1\\] on the pattern's device"):
            pg.gatv2_attention_dropout(pattern, x, x, a, 0.5, seed=seed)          # (a CPU tensor is on the wrong device)
    with pytest.raises(ValueError, match="gatv2_attention_dropout: negative_slope = nan"):
        pg.gatv2_attention_dropout(pattern, x, x, a, 0.5, negative_slope=float("nan"))
    # what gatv2_attention refuses, under this op's name -- whether or not the dropout kernels would run
    for kw in (dict(), dict(training=False)):
        for p in (0.5, 0.0):
            with pytest.raises(ValueError, match="gatv2_attention_dropout: an EdgePattern expected"):
                pg.gatv2_attention_dropout(object(), x, x, a, p, **kw)
            with pytest.raises(ValueError, match="gatv2_attention_dropout: x_dst must be a tensor on the GPU"):
                pg.gatv2_attention_dropout(pattern, x, x, a, p, **kw)


# ------------------------------------------------------------------------------------------------------- what the cases cover
def _deg(c):
    return torch.bincount(c.row, minlength=c.shape[0])


def test_the_mask_of_a_case_is_the_flat_layout():
    c = case.cases()["lanes-hub-3x8-indices-shared"]
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
            sh, sep = cs[f"lanes-hub-{H}x{F}-{kind}-shared"], cs[f"lanes-hub-{H}x{F}-{kind}-separate"]
            assert sh.v is None and sh.shared and sep.v.shape == sep.x_src.shape and not sep.shared
            assert sh.kind == sep.kind == kind and sh.p == sep.p == 0.5 and sh.x_dst.shape == (sh.shape[0], H, F) and sh.seed != sep.seed
    assert cs["lanes-hub-noaxis-graph-separate"].x_dst.dim() == 2
    assert int(_deg(cs["lanes-hub-8x16-graph-shared"]).max()) == 699 and int((_deg(cs["lanes-asym-8x16-indices-shared"]) == 1).sum()) > 0
    assert {cs[n].p for n in case.case_names("long-")} == {0.5, 0.9}
    assert {(cs[n].H, cs[n].F) for n in case.case_names("long-")} == {(3, 8), (8, 16), (12, 64)}
    for name in case.case_names("long-"):
        assert int(_deg(cs[name]).max()) > 512 and cs[name].p == float(name.rsplit("-p", 1)[1]), name
    assert int(_deg(cs["long-three_chunk_hub-3x8-graph-separate-p0.5"]).max()) >= 4097
    # rows of at least two entries, all of them dropped: the exact-zero check cannot pass vacuously
    for name in case.case_names("gone-"):
        assert cs[name].p == 0.9 and int(cs[name].all_dropped().sum()) >= 5, name
    for name in ("rect-4x16-shared", "rect-3x8-separate", "repeats-8x16-shared") + tuple(case.case_names("single-")):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation finds the mask"
    c = cs["repeats-8x16-shared"]
    assert torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]]) and torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])
    assert bool((c.mask[c.pairs[:, 0]] != c.mask[c.pairs[:, 1]]).any()), "the two entries of a repeated pair draw their own decisions"
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
    m = cs["module-rect-2x8"]
    assert m.mask.shape == (m.row.numel(), m.H) and m.p == 0.5
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
