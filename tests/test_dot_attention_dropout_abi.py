"""The two dropout launchers of csrc/k19_dot_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_dot_attention_bias_abi.py).  Also
here, on the CPU: the signature of pygat_amd.dot_attention_dropout and its refusals that need no GPU, what the seeded cases of
tests/dot_attention_dropout_case.py cover -- asserted from the NumPy mask of tests/philox_ref.py -- and every such case's rehearsal with
the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import dot_attention_dropout_case as case
import philox_ref
from abi_support import DOT_BIAS, P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_dot_attn_dropout_forward", "pygat_dot_attn_dropout_backward_rows")


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16, bias=P + 4,
             bias_head_stride=1, p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, ws=P)
    return call(L, "pygat_dot_attn_dropout_forward", a, **kw)


def _backward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P, ldk=16, v=P, ldv=16, bias=P + 4,
             bias_head_stride=1, p=0.5, seed=P + 8, stream_id=3, out=P, ldo=16, m=P, Z=P, G=P, ldg=16, dq=P, lddq=16, P=P, S=P,
             dbias=None, ws=P)
    return call(L, "pygat_dot_attn_dropout_backward_rows", a, **kw)


LAUNCHERS = ((_forward, "dot_attn_dropout_forward"), (_backward, "dot_attn_dropout_backward_rows"))
TABLES = {"dot_attn_dropout_forward": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo")),
          "dot_attn_dropout_backward_rows": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"), ("dq", "lddq"))}
SCALARS = {"dot_attn_dropout_forward": ("rowptr", "col", "m", "Z", "ws"),
           "dot_attn_dropout_backward_rows": ("rowptr", "col", "m", "Z", "P", "S", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert "dot_attn" in s and "attention" not in s
    p, i, i64, f, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
    assert lib.lib.pygat_dot_attn_dropout_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, f, p, u32, p, i64, p,
                                                               p, p, p]
    assert lib.lib.pygat_dot_attn_dropout_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, f, p, u32, p,
                                                                     i64, p, p, p, i64, p, i64, p, p, p, p, p]
    # the launchers before these keep their signatures, and the size query is theirs
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_dot_attn_backward_rows.argtypes) == 26 and len(lib.lib.pygat_dot_attn_bias_backward_rows.argtypes) == 29
    assert [s for s in lib.SYMBOLS if "dot_attn" in s and s.endswith("workspace_bytes")] == ["pygat_dot_attn_workspace_bytes"]
    from pygat_amd.dropout import STREAM_ATT
    assert case.STREAM_ATT == STREAM_ATT


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order; dbias may be null: not asked for; bias may be null: no bias, and its head stride is then not looked at)."""
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
            assert fn(lib, bias_head_stride=stride) == -1, (name, stride)
            assert _msg(lib).startswith(f"{name}: bias_head_stride={stride},"), (name, _msg(lib))


def test_the_same_wording_as_the_bias_pair(lib):
    """Whatever pygat_dot_attn_bias_forward / _backward_rows refuse, the dropout launchers refuse in the same words after their own
    name (a null bias apart: here it means no bias)."""
    for (fn, name), (bfn, bname) in zip(LAUNCHERS, DOT_BIAS):
        for kw in (dict(H=65), dict(F=12), dict(nnz=-1), dict(n_rows=0), dict(q=None), dict(k=P + 4), dict(ldv=12), dict(m=None),
                   dict(ws=None), dict(ws=P + 8), dict(col=None), dict(bias_head_stride=2), dict(out=None), dict(ldq=15)):
            assert fn(lib, **kw) == -1
            mine = _msg(lib)
            assert bfn(lib, **kw) == -1
            assert mine[len(name):] == _msg(lib)[len(bname):] and mine.startswith(name), (kw, mine, _msg(lib))


def test_a_null_seed_and_a_bad_p_are_refused(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, seed=None) == -1 and _msg(lib) == f"{name}: null seed", (name, _msg(lib))
        assert fn(lib, seed=P + 4) == -1 and _msg(lib) == f"{name}: seed must be 8-byte aligned", (name, _msg(lib))
        for p in (-0.25, 1.5, -1e-9, 1.0 + 1e-6, float("nan"), float("inf"), -float("inf")):
            assert fn(lib, p=p) == -1, (name, p)
            assert _msg(lib).startswith(f"{name}: p=") and _msg(lib).endswith("outside [0, 1]"), (name, p, _msg(lib))
        # the tables come first: what the bias pair refuses is refused in its words whatever p and the seed are
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
    assert "dot_attention_dropout" in pg.__all__ and "attention_dropout_mask" in pg.__all__
    sig = inspect.signature(pg.dot_attention_dropout)
    assert list(sig.parameters) == ["pattern", "q", "k", "v", "p", "scale", "bias", "seed", "generator", "training"]
    for name in ("seed", "generator", "training"):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters["scale"].default is None and sig.parameters["bias"].default is None
    assert sig.parameters["seed"].default is None and sig.parameters["generator"].default is None
    assert sig.parameters["training"].default is True and sig.parameters["p"].default is inspect.Parameter.empty
    assert list(inspect.signature(pg.attention_dropout_mask).parameters) == ["pattern", "H", "p", "seed"]
    assert list(inspect.signature(pg.dot_attention).parameters) == ["pattern", "q", "k", "v", "scale", "bias"]
    z = torch.zeros(3, 4)
    pattern = _fake_pattern()
    for p in (-0.1, 1.5, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match=r"dot_attention_dropout: p = .*\[0, 1\]"):
            pg.dot_attention_dropout(pattern, z, z, z, p)
        with pytest.raises(ValueError, match=r"attention_dropout_mask: p = .*\[0, 1\]"):
            pg.attention_dropout_mask(pattern, 2, p, torch.zeros(1, dtype=torch.int64))
    for k, v in ((z.bfloat16(), z.bfloat16()), (z, z.bfloat16()), (z.bfloat16(), z)):
        with pytest.raises(ValueError, match="dot_attention_dropout: k and v must be float32: there is no training path on bfloat16"):
            pg.dot_attention_dropout(pattern, z, k, v, 0.5)
    for seed in (5, torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), [1]):
        with pytest.raises(ValueError, match="dot_attention_dropout: seed must be an int64 tensor of shape \\[1\\] on the pattern's device"):
            pg.dot_attention_dropout(pattern, z, z, z, 0.5, seed=seed)            # (a CPU tensor is on the wrong device)
        with pytest.raises(ValueError, match="attention_dropout_mask: seed must be an int64 tensor"):
            pg.attention_dropout_mask(pattern, 2, 0.5, seed)
    # what dot_attention refuses, under this op's name -- whether or not the dropout kernels would run
    for kw in (dict(), dict(training=False)):
        for p in (0.5, 0.0):
            with pytest.raises(ValueError, match="dot_attention_dropout: an EdgePattern expected"):
                pg.dot_attention_dropout(object(), z, z, z, p, **kw)
            with pytest.raises(ValueError, match="dot_attention_dropout: q must be a tensor on the GPU"):
                pg.dot_attention_dropout(pattern, z, z, z, p, **kw)
            with pytest.raises(ValueError, match="dot_attention_dropout: bias must be a tensor on the GPU"):
                pg.dot_attention_dropout(pattern, z, z, z, p, bias=torch.zeros(3), **kw)


# ------------------------------------------------------------------------------------------------------- what the cases cover
def _deg(c):
    return torch.bincount(c.row, minlength=c.shape[0])


def _top_entry_dropped(c, rows):
    """bool [len(rows), H]: the entry of the largest score of the row is dropped in that head."""
    s = c.scores()
    out = []
    for r in rows:
        e = torch.nonzero(c.row == r)[:, 0]
        top = e[s[e].argmax(0)]                                  # [H] entry indices
        out.append(c.mask[top, torch.arange(c.H)] == 0)
    return torch.stack(out)


def test_the_mask_of_a_case_is_the_flat_layout():
    c = case.cases()["lanes-hub-3x8-indices-plain"]
    E = c.row.numel()
    thresh, scale = philox_ref.threshold(0.5)
    words = case.flat_words(c.seed, E * 3)
    assert words.dtype == np.uint32 and float(scale) == 2.0
    assert np.array_equal(np.where(words < np.uint32(thresh), np.float32(2.0), np.float32(0.0)).reshape(E, 3), c.mask.numpy())
    level = philox_ref.level_masks(c.seed, 0.5, 3, 4, 4, 4, 4, E, "bits")["att"]          # the level's attention mask: the same table
    assert np.array_equal(level, c.mask.numpy())
    assert 0.45 < float((c.mask != 0).float().mean()) < 0.55


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            plain, b = cs[f"lanes-hub-{H}x{F}-{kind}-plain"], cs[f"lanes-hub-{H}x{F}-{kind}-bias"]
            assert plain.bias is None and b.bias.shape == (b.row.numel(), H) and plain.kind == b.kind == kind and plain.p == b.p == 0.5
            assert plain.q.shape == (plain.shape[0], H, F) and plain.seed != b.seed
    for kind in ("indices", "graph"):
        assert cs[f"lanes-hub-noaxis-{kind}-plain"].q.dim() == 2 and cs[f"lanes-hub-noaxis-{kind}-bias"].bias.dim() == 1
    for name in ("lanes-hub-8x16-indices-shared", "lanes-hub-12x64-graph-shared"):
        assert cs[name].bias.dim() == 1 and cs[name].H > 1
    hubc = cs["lanes-hub-8x16-graph-plain"]
    assert int(_deg(hubc).max()) == 699 and int((_deg(cs["lanes-asym-8x16-indices-plain"]) == 1).sum()) > 0
    # dropout after the softmax, not masking before it: the entry of the largest score is dropped, on a short row and on a long one
    deg = _deg(hubc)
    long_row, short_row = int(deg.argmax()), int(torch.nonzero((deg >= 3) & (deg <= 16))[0, 0])
    assert deg[long_row] > 512
    assert bool(_top_entry_dropped(hubc, [long_row]).any()) and bool(_top_entry_dropped(hubc, [short_row, short_row + 1, short_row + 2]).any())
    for name in case.case_names("long-"):
        c = cs[name]
        assert c.p == float(name.rsplit("-p", 1)[1]) and 2.5 < float(c.inner.scores().std()) < 3.5, name
        long_rows = torch.nonzero(_deg(c) > 512)[:, 0].tolist()
        assert bool(_top_entry_dropped(c, long_rows).any()), name
    assert {cs[n].p for n in case.case_names("long-")} == {0.5, 0.9}
    # kept and dropped entries in every piece of a long row (a piece: the entries of the row inside one 2048-entry chunk, which one
    # slot of the chunk's records sums), in every head
    for name in ("long-nine_hubs-8x16-graph-p0.5", "long-nine_hubs-8x16-graph-p0.9", "long-three_chunk_hub-3x8-graph-p0.5"):
        c = cs[name]
        assert c.kind == "graph" and bool((c.row[1:] >= c.row[:-1]).all()), "the caller's entry order is the CSR order"
        rowptr = np.asarray(c.csr[0], dtype=np.int64)
        pieces = 0
        for r in torch.nonzero(_deg(c) > 512)[:, 0].tolist():
            a, b = int(rowptr[r]), int(rowptr[r + 1])
            cuts = [a] + [x for x in range((a // 2048 + 1) * 2048, b, 2048)] + [b]
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                kept = (c.mask[lo:hi] != 0)
                assert bool(kept.any(0).all()) and bool((~kept).any(0).all()), (name, r, lo, hi)
                pieces += 1
        assert pieces >= (3 if "three" in name else 9 + 2), (name, pieces)      # rows 3 and 7 of nine_hubs are cut by a chunk boundary
    assert int((_deg(cs["long-nine_hubs-8x16-graph-p0.5"]) == 521).sum()) == 9
    assert int(_deg(cs["long-three_chunk_hub-3x8-graph-p0.5"]).max()) >= 4097
    # rows of at least two entries, all of them dropped
    for name in case.case_names("gone-"):
        gone = cs[name].all_dropped()
        assert int(gone.sum()) >= 5, (name, int(gone.sum()))
    for name in ("rect-3x8-plain", "rect-4x16-bias", "repeats-8x16-plain", "masked-rect-3x8") + tuple(case.case_names("single-")):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation finds the mask"
    c = cs["repeats-8x16-plain"]
    assert torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]]) and torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])
    assert bool((c.mask[c.pairs[:, 0]] != c.mask[c.pairs[:, 1]]).any()), "the two entries of a repeated pair draw their own decisions"
    for name in case.case_names("masked-"):
        c = cs[name]
        E = c.row.numel()
        assert 0.2 * E < int(c.masked.sum()) < 0.4 * E and bool((c.bias[c.masked] == case.MASK).all())
        assert bool(((c.mask[c.masked] != 0).any(1)).any()), "a masked entry that the dropout keeps: still an exact zero"
        leaves = [t.clone().requires_grad_(True) for t in c.leaves]
        db64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))[3]
        assert float(db64[c.masked].abs().max()) == 0.0, "the fp64 ground truth's db at a masked entry is an exact zero too"
    for name in case.case_names("single-"):
        c = cs[name]
        assert bool((_deg(c) == 1).all()) and c.shape == (300, 400) and c.p == 0.5
        assert bool((c.mask == 0).any(0).all()) and bool((c.mask == 2).any(0).all())
    # p next to 0: the threshold is 0xFFFFFFFF, the factor rounds to 1, and no draw of these cases is the one word that is dropped
    thresh, scale = philox_ref.threshold(case.P_NEAR_0)
    assert thresh == 0xFFFFFFFF and float(scale) == 1.0
    for name in case.case_names("near0-"):
        c = cs[name]
        assert c.p == case.P_NEAR_0
        assert not bool((case.flat_words(c.seed, c.row.numel() * c.H) == np.uint32(0xFFFFFFFF)).any()), name
        assert bool((c.mask == 1).all())
    assert sorted(case.case_names("twice-")) == ["twice-hub-3x8-graph-plain", "twice-nine_hubs-8x16-indices-bias"]
    m = cs["module-hub-4x16-graph"]
    assert m.mask.shape == (m.row.numel(), m.H) and m.weights[3].shape == (case.biased.N_TYPES, m.H) and m.p == 0.5
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


def test_masking_before_the_softmax_is_another_function():
    """What separates the op from a softmax over the kept entries: on the hub row the two differ far beyond the pricing."""
    c = case.cases()["lanes-hub-8x16-graph-plain"]
    want = c.ref(c.q, c.k, c.v).reshape(c.q.shape)
    s = c.scores().masked_fill(c.mask == 0, -math.inf)
    alpha = case.edge_softmax_ref(c.row, c.shape[0], s).nan_to_num(0.0)
    other = case.spmm_ref(c.row, c.col, c.shape[0], alpha, c.v)
    assert float((want - other).abs().max()) > 0.1


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
