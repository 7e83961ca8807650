"""The two EDGE launchers of csrc/k19_dot_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is
launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_dot_attention_abi.py).  Also
here, on the CPU: the signature of pygat_amd.dot_attention_edge and its refusals that need no GPU, what the seeded cases of
tests/dot_attention_edge_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import dot_attention_edge_case as case
from abi_support import DOT, DOT_EDGE, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_dot_attn_edge_forward", "pygat_dot_attn_edge_backward_rows")


LAUNCHERS = DOT_EDGE
_forward, _backward = (fn for fn, _ in LAUNCHERS)
TABLES = {"dot_attn_edge_forward": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo"), ("e", "lde")),
          "dot_attn_edge_backward_rows": (("q", "ldq"), ("k", "ldk"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"), ("dq", "lddq"),
                                          ("e", "lde"))}
SCALARS = {"dot_attn_edge_forward": ("rowptr", "col", "m", "Z", "ws"),
           "dot_attn_edge_backward_rows": ("rowptr", "col", "m", "Z", "P", "S", "ws")}
# the refusals of test_dot_attention_bias_abi.py::test_every_launcher_refuses_the_limits
LIMITS = [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"), (dict(F=2), "F=2"),
          (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"), (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"),
          (dict(n_rows=-1), "n_rows=-1"), (dict(n_rows=0), "n_rows=0 with nnz=20")]


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, f, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint32
    assert lib.lib.pygat_dot_attn_edge_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, i, p, i64, p, p,
                                                            p, p]
    assert lib.lib.pygat_dot_attn_edge_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, i, p, i64,
                                                                  p, p, p, i64, p, i64, p, p, p, i64, p, p, p]
    # the six launchers before this pair and the size query keep their signatures
    assert lib.lib.pygat_dot_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, i64, p,
                                                             i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p,
                                                                  i64, p, i64, p, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bf16_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p]
    assert lib.lib.pygat_dot_attn_dropout_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, f, p, u32, p, i64,
                                                               p, p, p, p]
    assert lib.lib.pygat_dot_attn_dropout_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, f, p, u32, p,
                                                                     i64, p, p, p, i64, p, i64, p, p, p, p, p]


@pytest.mark.parametrize("kw,needle", LIMITS)
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        for extra in ({}, dict(bias=None)):                          # with a bias and without one
            assert fn(lib, **kw, **extra) == -1, (name, kw)
            assert needle in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short.  perm may be null (the
    caller's order), dbias may be null (not asked for), bias may be null (no bias; its head stride is then not looked at), de may be
    null (not asked for; ldde is then not looked at) -- as far as the checks go: those calls are made either with one more argument
    that is refused after the one in question, or without rows, where a launcher returns 0 after its checks and launches nothing."""
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
        # a null bias passes every check, whatever its head stride says; so does a null e where there are no entries
        assert fn(lib, n_rows=0, nnz=0, bias=None, bias_head_stride=7) == 0, _msg(lib)
        assert fn(lib, n_rows=0, nnz=0, col=None, e=None, lde=0) == 0, _msg(lib)
    # de: misaligned and short strides are refused under its name; null, it is not looked at, nor is ldde
    name = "dot_attn_edge_backward_rows"
    assert _backward(lib, de=P + 4) == -1 and _msg(lib) == f"{name}: de must be 16-byte aligned"
    for short in (15, 12, 18):
        assert _backward(lib, ldde=short) == -1 and f"the row stride of de, {short}," in _msg(lib) and name in _msg(lib), _msg(lib)
    assert _backward(lib, de=None, ldde=3, bias_head_stride=5) == -1 and _msg(lib).startswith(f"{name}: bias_head_stride=5,"), _msg(lib)
    # e is checked before de and both before the bias; without entries a null e is not refused
    assert _backward(lib, e=None, de=P + 4) == -1 and _msg(lib) == f"{name}: null e"
    assert _backward(lib, de=P + 4, bias_head_stride=5) == -1 and _msg(lib) == f"{name}: de must be 16-byte aligned"
    assert _backward(lib, n_rows=0, nnz=0, de=None, ldde=3) == 0, _msg(lib)
    for fn, name in LAUNCHERS:
        assert fn(lib, nnz=0, col=None, e=None, bias_head_stride=5) == -1 and _msg(lib).startswith(f"{name}: bias_head_stride=5,")
        assert fn(lib, nnz=0, col=None, e=P + 4) == -1 and _msg(lib) == f"{name}: e must be 16-byte aligned"


def test_the_same_wording_as_the_pair_without_a_bias(lib):
    """Whatever pygat_dot_attn_forward / _backward_rows refuse, the EDGE launchers refuse in the same words after their own name."""
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
    assert "dot_attention_edge" in pg.__all__ and pg.dot_attention_edge.__module__ == "pygat_amd.dot_attention"
    sig = inspect.signature(pg.dot_attention_edge)
    assert list(sig.parameters) == ["pattern", "q", "k", "v", "e", "scale", "bias"]
    assert sig.parameters["bias"].default is None and sig.parameters["scale"].default is None
    assert sig.parameters["e"].default is inspect.Parameter.empty
    assert list(inspect.signature(pg.dot_attention).parameters) == ["pattern", "q", "k", "v", "scale", "bias"]
    assert list(inspect.signature(pg.dot_attention_dropout).parameters) == ["pattern", "q", "k", "v", "p", "scale", "bias", "seed",
                                                                            "generator", "training"]
    assert list(inspect.signature(pg.edge_dot).parameters) == ["pattern", "q", "k", "scale"]
    assert list(inspect.signature(pg.attention_dropout_mask).parameters) == ["pattern", "H", "p", "seed"]
    z = torch.zeros(3, 4)
    with pytest.raises(ValueError, match="dot_attention_edge.*EdgePattern"):
        pg.dot_attention_edge(object(), z, z, z, torch.zeros(5, 4))
    for bad in ([0.0, 1.0], 1.0, None, torch.zeros(5, 4), torch.zeros(5, 4, dtype=torch.float64)):      # (not a tensor; a CPU tensor)
        with pytest.raises(ValueError, match=r"dot_attention_edge: e must be a tensor on the GPU.*\[E, H, F\]"):
            pg.dot_attention_edge(_fake_pattern(), z, z, z, bad)
    b16 = torch.zeros(5, 4, dtype=torch.bfloat16)
    for args in ((z, z, z, b16), (z, b16, z, z), (z, z, b16, z), (z, b16, b16, z)):
        with pytest.raises(ValueError, match="dot_attention_edge: k, v and e must be float32"):
            pg.dot_attention_edge(_fake_pattern(), *args)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    edge = [c for c in cs.values() if isinstance(c, case.EdgeCase)]
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            c = cs[f"lanes-hub-{H}x{F}-{kind}"]
            assert c.q.shape == (c.shape[0], H, F) and c.bias is None and c.fed_scale is None and c.kind == kind
    c = cs["lanes-hub-8x16-graph"]
    e = c.e
    assert e.shape == (c.row.numel(), 8, 16) and 0.95 < float(e.std()) < 1.05 and torch.equal(e, c.e), "seeded: drawn the same again"
    assert int(deg(c).max()) == 699 and int((deg(cs["lanes-asym-8x16-indices"]) == 1).sum()) > 0
    for H, F in ((3, 8), (8, 16), (12, 64)):
        assert cs[f"lanes-asym-{H}x{F}-indices"].q.shape[1:] == (H, F)
    for kind in ("indices", "graph"):
        c = cs[f"lanes-hub-noaxis-{kind}"]
        assert c.q.dim() == 2 and c.e.shape == (c.row.numel(), c.F)
    assert cs["bias-hub-8x16-indices"].bias.shape == (cs["bias-hub-8x16-indices"].row.numel(), 8)
    assert cs["bias-hub-3x8-graph"].bias.shape[1] == 3 and cs["bias-hub-3x8-graph"].kind == "graph"
    c = cs["bias-shared-hub-8x16-indices"]
    assert c.bias.dim() == 1 and c.H == 8 and c.q.dim() == 3
    for name in case.case_names("masked-"):
        c = cs[name]
        E = c.row.numel()
        assert 0.2 * E < int(c.masked.sum()) < 0.4 * E, (name, int(c.masked.sum()), E)
        assert bool((c.bias[c.masked] == case.MASK).all()) and bool((c.bias[~c.masked].abs() < 10.0).all())
        assert not bool((c.masked & case.first_of_row(c.row)).any()), "every row keeps an unmasked entry"
        assert float(c.coefficients()[c.masked].abs().max()) == 0.0
        leaves = [t.clone().requires_grad_(True) for t in c.leaves]
        g64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))
        assert float(g64[3][c.masked].abs().max()) == 0.0, "the fp64 ground truth's de at a masked entry is an exact zero too"
        assert float(g64[4][c.masked].abs().max()) == 0.0
    assert len(case.case_names("masked-")) == 1
    assert len(case.case_names("long-")) == 8
    for name in case.case_names("long-"):
        c = cs[name]
        e = c.e
        kq, eq = c.key_terms()
        assert c.fed_scale is None and 2.9 < float(e.std()) < 3.1, name
        assert float(kq.std()) < 0.5 * float(eq.std()), "the key-side term of e decides which entries dominate a row"
    assert int((deg(cs["long-nine_hubs-8x16-graph"]) == 521).sum()) == 9 and int(deg(cs["long-three_chunk_hub-3x8-graph"]).max()) >= 4097
    for name in ("rect-3x8", "rect-4x16", "repeats-8x16"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a row of e"
    assert int((deg(cs["rect-3x8"]) == 0).sum()) == 100
    c = cs["repeats-8x16"]
    pairs, e = c.pairs, c.e
    assert pairs.shape[0] > 100
    assert torch.equal(c.row[pairs[:, 0]], c.row[pairs[:, 1]]) and torch.equal(c.col[pairs[:, 0]], c.col[pairs[:, 1]])
    alpha = c.coefficients()
    assert bool((e[pairs[:, 0]] != e[pairs[:, 1]]).any(-1).all()) and bool((alpha[pairs[:, 0]] != alpha[pairs[:, 1]]).all())
    leaves = [t.clone().requires_grad_(True) for t in c.leaves]
    de64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))[3]
    assert bool((de64[pairs[:, 0]] != de64[pairs[:, 1]]).flatten(1).any(1).all()), "the two entries of a pair get different rows of de"
    for kind in ("indices", "graph"):
        for hf in ("8x16", "3x8"):
            assert int((deg(cs[f"lonely-{hf}-{kind}"]) == 1).sum()) >= 12 and cs[f"lonely-{hf}-{kind}"].bias is None
    import dot_attention_bias_case as biased
    import dot_attention_case as plain
    zero = case.case_names("zero-")
    assert len(zero) == 4
    for name in zero:
        c = cs[name]
        assert float(c.e.abs().max()) == 0.0
        if name.startswith("zero-bias-"):
            assert c.inner is biased.cases()[name[len("zero-bias-"):]].inner and c.bias is biased.cases()[name[len("zero-bias-"):]].bias
        else:
            assert c.inner is plain.cases()[name[len("zero-"):]] and c.bias is None
    assert cs["zero-lanes-hub-12x64-indices"].H * cs["zero-lanes-hub-12x64-indices"].F == 3 * 256
    assert sorted(case.case_names("twice-")) == ["twice-hub-3x8-graph", "twice-nine_hubs-8x16-indices"]
    assert cs["twice-nine_hubs-8x16-indices"].bias is not None, "db is among the outputs of one of the two"
    assert sorted(case.case_names("composed-")) == ["composed-hub-8x16-graph", "composed-hub-8x16-indices"]
    assert all(isinstance(cs[n], case.ComposedEdgeCase) for n in case.case_names("composed-"))
    assert cs["composed-hub-8x16-indices"].bias is not None and cs["composed-hub-8x16-graph"].bias is None
    m = cs["module-hub-4x16-graph"]
    assert m.edge_attr.shape == (m.row.numel(), case.EDGE_DIM) and m.weights[3].shape == (m.H * m.F, case.EDGE_DIM)
    assert m.NAMES[-1] == "lin_edge.weight"
    # the conditions every case meets: e of at most 2^23 floats, patterns of at most 4 500 rows
    assert max(c.row.numel() * c.H * c.F for c in edge) <= case.MAX_E_FLOATS == 1 << 23
    assert max(c.row.numel() * c.H * c.F for c in edge) == 7646 * 1024
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()


def test_a_row_of_one_entry_in_the_fp32_reference():
    """What the device is held to bit for bit, the fp32 ground truth meets in value: out_i = v_j + e_c, dq_i = 0, de_c = G_i."""
    c = case.cases()["lonely-3x8-indices"]
    out, dq, dk, dv, de = c.stand_in()
    single = torch.bincount(c.row, minlength=c.shape[0])[c.row] == 1
    rows, cols = c.row[single], c.col[single]
    assert torch.equal(out[rows], (c.v.float()[cols] + c.e.float()[single]))
    assert float(dq[rows].abs().max()) < 1e-6 and float((de[single] - c.G.float()[rows]).abs().max()) < 1e-6
