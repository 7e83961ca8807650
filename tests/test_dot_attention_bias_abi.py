"""The two bias launchers of csrc/k19_dot_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_dot_attention_abi.py).  Also
here, on the CPU: the refusals of `bias` that pygat_amd.dot_attention makes before it looks at q, what the seeded cases of
tests/dot_attention_bias_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import dot_attention_bias_case as case
from abi_support import DOT, DOT_BIAS, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_dot_attn_bias_forward", "pygat_dot_attn_bias_backward_rows")


LAUNCHERS = DOT_BIAS
_forward, _backward = (fn for fn, _ in LAUNCHERS)
TABLES = {"dot_attn_bias_forward": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo")),
          "dot_attn_bias_backward_rows": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"), ("dq", "lddq"))}
SCALARS = {"dot_attn_bias_forward": ("rowptr", "col", "m", "Z", "bias", "ws"),
           "dot_attn_bias_backward_rows": ("rowptr", "col", "m", "Z", "P", "S", "bias", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert "attention" not in s
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert lib.lib.pygat_dot_attn_bias_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p,
                                                                  i64, p, i64, p, p, p, p, p]
    # the pair without a bias keeps its signatures
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_dot_attn_backward_rows.argtypes) == 26


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
    caller's order; dbias may be null: not asked for; bias needs no alignment beyond its 4 bytes)."""
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


def test_the_same_wording_as_the_pair_without_a_bias(lib):
    """Whatever pygat_dot_attn_forward / _backward_rows refuse, the bias launchers refuse in the same words after their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS, DOT):
        for kw in (dict(H=65), dict(F=12), dict(nnz=-1), dict(n_rows=0), dict(q=None), dict(k=P + 4), dict(ldv=12), dict(m=None),
                   dict(ws=None), dict(ws=P + 8), dict(col=None)):
            assert fn(lib, **kw) == -1
            mine = _msg(lib)
            assert pfn(lib, **kw) == -1
            assert mine[len(name):] == _msg(lib)[len(pname):] and mine.startswith(name), (kw, mine, _msg(lib))


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    return pattern


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    sig = inspect.signature(pg.dot_attention)
    assert list(sig.parameters) == ["pattern", "q", "k", "v", "scale", "bias"]
    assert sig.parameters["bias"].default is None and sig.parameters["scale"].default is None
    assert "-9e15" in pg.dot_attention.__doc__ and "unmasked" in pg.dot_attention.__doc__
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="dot_attention.*EdgePattern"):
        pg.dot_attention(object(), z, z, z, bias=torch.zeros(3))
    for bad in ([0.0, 1.0], 1.0, torch.zeros(3), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="dot_attention: bias must be a tensor on the GPU"):
            pg.dot_attention(_fake_pattern(), z, z, z, bias=bad)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            c = cs[f"lanes-hub-{H}x{F}-{kind}"]
            assert c.q.shape == (c.shape[0], H, F) and c.bias.shape == (c.row.numel(), H) and c.fed_scale is None and c.kind == kind
            assert 0.9 < float(c.bias.std()) < 1.1
    for H, F in ((3, 8), (8, 16), (12, 64)):
        assert cs[f"lanes-asym-{H}x{F}-indices"].bias.shape[1] == H
    assert int(deg(cs["lanes-hub-8x16-graph"]).max()) == 699 and int((deg(cs["lanes-asym-8x16-indices"]) == 1).sum()) > 0
    for kind in ("indices", "graph"):
        c = cs[f"lanes-hub-noaxis-{kind}"]
        assert c.q.dim() == 2 and c.bias.dim() == 1
    for name in ("shared-hub-8x16-indices", "shared-hub-3x8-graph"):
        assert cs[name].bias.dim() == 1 and cs[name].H > 1 and cs[name].q.dim() == 3
    for name in case.case_names("long-"):
        c = cs[name]
        assert c.fed_scale is None and 2.8 < float(c.bias.std()) < 3.2, name
        assert float(c.inner.scores().std()) < 0.5 * float(c.bias.std()), "the bias decides which entries dominate a row"
    assert int((deg(cs["long-nine_hubs-8x16-graph"]) == 521).sum()) == 9 and int(deg(cs["long-three_chunk_hub-3x8-graph"]).max()) >= 4097
    for name in ("rect-3x8", "rect-4x16", "repeats-8x16", "masked-rect-3x8"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a bias"
    c = cs["repeats-8x16"]
    pairs = c.pairs
    assert pairs.shape[0] > 100
    assert torch.equal(c.row[pairs[:, 0]], c.row[pairs[:, 1]]) and torch.equal(c.col[pairs[:, 0]], c.col[pairs[:, 1]])
    alpha = c.coefficients()
    assert bool((c.bias[pairs[:, 0]] != c.bias[pairs[:, 1]]).all()) and bool((alpha[pairs[:, 0]] != alpha[pairs[:, 1]]).all())
    for name in case.case_names("masked-"):
        c = cs[name]
        E = c.row.numel()
        assert 0.2 * E < int(c.masked.sum()) < 0.4 * E, (name, int(c.masked.sum()), E)
        assert bool((c.bias[c.masked] == case.MASK).all()) and bool((c.bias[~c.masked].abs() < 10.0).all())
        assert not bool((c.masked & case.first_of_row(c.row)).any()), "every row keeps an unmasked entry"
        assert float(c.coefficients()[c.masked].abs().max()) == 0.0
        leaves = [t.clone().requires_grad_(True) for t in (c.q, c.k, c.v, c.bias)]
        db64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))[3]
        assert float(db64[c.masked].abs().max()) == 0.0, "the fp64 ground truth's db at a masked entry is an exact zero too"
    assert int(deg(cs["masked-three_chunk_hub-3x8-graph"]).max()) >= 4097
    assert int((deg(cs["lonely-8x16-graph"]) == 1).sum()) >= 12
    import dot_attention_case as plain
    for name in case.case_names("zero-"):
        c = cs[name]
        assert float(c.bias.abs().max()) == 0.0 and c.inner is plain.cases()[name[len("zero-"):]]
    assert cs["zero-lanes-hub-12x64-indices"].H * cs["zero-lanes-hub-12x64-indices"].F == 3 * 256
    a, b = cs["shift-hub-8x16-plain"], cs["shift-hub-8x16-shifted"]
    d = b.bias - a.bias
    assert a.inner is b.inner and 2.0 < float(d.std()) < 4.0
    for r in (0, 7, int(a.row.max())):                             # one value per row and head (up to the fp32 rounding of the sum)
        assert float((d[a.row == r] - d[a.row == r][0]).abs().max()) < 1e-5
    assert sorted(case.case_names("twice-")) == ["twice-hub-3x8-graph", "twice-nine_hubs-8x16-indices"]
    m = cs["module-hub-4x16-graph"]
    assert m.types.shape == (m.row.numel(),) and sorted(m.types.unique().tolist()) == list(range(case.N_TYPES))
    assert m.weights[3].shape == (case.N_TYPES, m.H)
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()


def test_shifted_rows_in_the_fp32_reference():
    """db sums to 0 over every row; the fp32 ground truth's own sums are what the device's are held against."""
    for name in case.case_names("shift-"):
        c = case.cases()[name]
        own = float(c.db_row_sums(c.stand_in()[4]).abs().max())
        print(name, f"row sums of db in the fp32 ground truth: {own:.2e}")
        assert own < 1e-4
