"""The three EDGE launchers of csrc/k21_gatv2_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything
is launched: no GPU is needed, and a fake non-null address stands in for every device table (as in test_gatv2_attention_abi.py).  Also
here, on the CPU: the signature of pygat_amd.gatv2_attention_edge and its refusals that need no GPU, what the seeded cases of
tests/gatv2_attention_edge_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import gatv2_attention_edge_case as case
from abi_support import DOT_EDGE, GATV2, GATV2_EDGE, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_v2_attn_edge_forward", "pygat_v2_attn_edge_backward_rows", "pygat_v2_attn_edge_backward_cols")


LAUNCHERS = GATV2_EDGE
_forward, _backward, _columns = (fn for fn, _ in LAUNCHERS)
TABLES = {"v2_attn_edge_forward": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo"), ("e", "lde")),
          "v2_attn_edge_backward_rows": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"),
                                         ("dx_dst", "lddx"), ("e", "lde")),
          "v2_attn_edge_backward_cols": (("x_dst", "ldd"), ("x_src", "lds"), ("dx_src", "lddx"), ("e", "lde"))}
SCALARS = {"v2_attn_edge_forward": ("rowptr", "col", "a", "m", "Z", "ws"),
           "v2_attn_edge_backward_rows": ("rowptr", "col", "a", "m", "Z", "P", "S", "ws"),
           "v2_attn_edge_backward_cols": ("rowptr_t", "row_t", "a", "S", "da", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    # the K21 lists with (e, lde) after (v, ldv) -- after a in the column pass -- the forward takes perm after col, and the row pass
    # (de, ldde) after S
    assert lib.lib.pygat_v2_attn_edge_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_edge_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, i64, p, p,
                                                                 p, i64, p, i64, p, p, p, i64, p, p]
    assert lib.lib.pygat_v2_attn_edge_backward_cols.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, p, i64, p, p, p]
    # the K21 launchers before these keep their signatures; no new size query
    assert lib.lib.pygat_v2_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, i64, p, i64,
                                                            p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_cols.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, p, i64, p, p, p]
    assert len(lib.lib.pygat_v2_attn_dropout_forward.argtypes) == 24 and len(lib.lib.pygat_v2_attn_dropout_backward_rows.argtypes) == 30
    assert [s for s in lib.SYMBOLS if "v2_attn" in s and s.endswith("workspace_bytes")] == ["pygat_v2_attn_workspace_bytes"]
    assert not any("edge_dropout" in s or "dropout_edge" in s for s in lib.SYMBOLS), "EDGE does not combine with DROP"


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n=-1), "=-1"),
                                       (dict(n=0), "=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "negative_slope=nan, a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "negative_slope=inf")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        n = "n_cols" if name.endswith("cols") else "n_rows"
        mine = {(n if k == "n" else k): v for k, v in kw.items()}
        want = n + needle if "n" in kw else needle
        assert fn(lib, **mine) == -1, (name, kw)
        assert want in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order; v may be null: v is x_src; de may be null: not asked for, ldde is then not looked at)."""
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
        # the launcher's own tables come before e; without entries a null e is not refused, a misaligned one is
        assert fn(lib, e=None, ws=None) == -1 and _msg(lib) == f"{name}: null workspace"
        n = "n_cols" if name.endswith("cols") else "n_rows"
        col = "row_t" if name.endswith("cols") else "col"
        assert fn(lib, **{n: 0, "nnz": 0, col: None, "e": None, "lde": 0}) == 0, _msg(lib)
        assert fn(lib, **{"nnz": 0, col: None, "e": P + 4}) == -1 and _msg(lib) == f"{name}: e must be 16-byte aligned"
    # de: misaligned and short strides are refused under its name; null, it is not looked at, nor is ldde
    name = "v2_attn_edge_backward_rows"
    assert _backward(lib, de=P + 4) == -1 and _msg(lib) == f"{name}: de must be 16-byte aligned"
    for short in (15, 12, 18):
        assert _backward(lib, ldde=short) == -1 and f"the row stride of de, {short}," in _msg(lib) and name in _msg(lib), _msg(lib)
    assert _backward(lib, e=None, de=P + 4) == -1 and _msg(lib) == f"{name}: null e"
    assert _backward(lib, n_rows=0, nnz=0, de=None, ldde=3) == 0, _msg(lib)
    assert _backward(lib, n_rows=0, nnz=0, de=P, ldde=3) == -1 and "the row stride of de, 3," in _msg(lib)
    for fn, name in LAUNCHERS[:2]:
        # a null v selects the shared-value kernels: its stride is then not looked at
        assert fn(lib, v=None, ldv=7, e=P + 8) == -1 and _msg(lib) == f"{name}: e must be 16-byte aligned"
    assert _columns(lib, da=P + 4) == -1 and _msg(lib) == "v2_attn_edge_backward_cols: da must be 16-byte aligned"


def test_the_same_wording_as_the_launchers_without_e(lib):
    """Whatever pygat_v2_attn_forward / _backward_rows / _backward_cols refuse, the EDGE launchers refuse in the same words after
    their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS, GATV2):
        cols = name.endswith("cols")
        for kw in (dict(H=65), dict(F=12), dict(nnz=-1), dict(x_dst=None), dict(x_src=P + 4), dict(lds=15), dict(ws=None),
                   dict(ws=P + 8), dict(a=None), dict(negative_slope=float("nan")), dict(H=8, F=256),
                   dict(dx_src=None) if cols else dict(ldv=12), dict(S=None) if cols else dict(m=None),
                   dict(row_t=None) if cols else dict(col=None), dict(n_cols=0) if cols else dict(n_rows=0)):
            assert fn(lib, **kw) == -1
            mine = _msg(lib)
            assert pfn(lib, **kw) == -1
            assert mine[len(name):] == _msg(lib)[len(pname):] and mine.startswith(name), (kw, mine, _msg(lib))


def test_e_and_de_are_refused_in_the_words_of_dot_attn_edge(lib):
    for (fn, name), (dfn, dname) in ((LAUNCHERS[0], DOT_EDGE[0]), (LAUNCHERS[1], DOT_EDGE[1]), (LAUNCHERS[2], DOT_EDGE[0])):
        kws = [dict(e=None), dict(e=P + 4), dict(e=P + 8), dict(lde=15), dict(lde=12), dict(lde=18), dict(lde=0), dict(lde=-16)]
        if name.endswith("backward_rows"):
            kws += [dict(de=P + 4), dict(ldde=15), dict(ldde=18), dict(ldde=0), dict(e=None, de=P + 4)]
        for kw in kws:
            assert fn(lib, **kw) == -1, (name, kw)
            mine = _msg(lib)
            assert dfn(lib, **kw) == -1, (dname, kw)
            assert mine[len(name):] == _msg(lib)[len(dname):] and mine.startswith(name + ": "), (kw, mine, _msg(lib))


def test_with_every_pointer_null(lib):
    for name in NEW:
        n_args = len(getattr(lib.lib, name).argtypes)
        assert getattr(lib.lib, name)(*([0] * n_args)) < 0 and _msg(lib).startswith(name[len("pygat_"):] + ": ")


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    pattern.n_rows = pattern.n_cols = 3
    return pattern


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    assert "gatv2_attention_edge" in pg.__all__ and pg.gatv2_attention_edge.__module__ == "pygat_amd.gatv2_attention"
    sig = inspect.signature(pg.gatv2_attention_edge)
    assert list(sig.parameters) == ["pattern", "x_dst", "x_src", "a", "e", "v", "negative_slope"]
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["v"].default is None
    assert sig.parameters["e"].default is inspect.Parameter.empty
    assert list(inspect.signature(pg.gatv2_attention).parameters) == ["pattern", "x_dst", "x_src", "a", "v", "negative_slope"]
    doc = " ".join(pg.gatv2_attention_edge.__doc__.split())
    for absent in ("dropout on the coefficients together with edge features", "bfloat16 tables", "e in the value sum"):
        assert absent in doc[doc.index("Not provided"):], absent
    parent = " ".join(pg.gatv2_attention.__doc__.split())
    assert "gatv2_attention_edge" in parent[parent.index("Not provided"):]
    x, a, e = torch.zeros(3, 4, 8), torch.zeros(4, 8), torch.zeros(5, 4, 8)
    with pytest.raises(ValueError, match="gatv2_attention_edge: an EdgePattern expected"):
        pg.gatv2_attention_edge(object(), x, x, a, e)
    for bad in ([0.0, 1.0], 1.0, None, e, e.double()):                                # (not a tensor; a CPU tensor)
        with pytest.raises(ValueError, match=r"gatv2_attention_edge: e must be a tensor on the GPU.*\[E, H, F\]"):
            pg.gatv2_attention_edge(_fake_pattern(), x, x, a, bad)
    for args, kw in (((x.bfloat16(), x, a, e), {}), ((x, x, a.bfloat16(), e), {}), ((x, x, a, e.bfloat16()), {}),
                     ((x, x, a, e), dict(v=x.bfloat16()))):
        with pytest.raises(ValueError, match="gatv2_attention_edge: x_dst, x_src, a, v and e must be float32"):
            pg.gatv2_attention_edge(_fake_pattern(), *args, **kw)
    for slope in (float("nan"), float("inf"), None, "0.2", True):
        with pytest.raises(ValueError, match="gatv2_attention_edge: negative_slope = .* a finite float expected"):
            pg.gatv2_attention_edge(_fake_pattern(), x, x, a, e, None, slope)

    # tensors that say they live on the GPU: the refusals of e's dtype, device and shape, before any of them is touched
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    where = _fake_pattern()
    where.device, where.nnz = torch.device("cpu"), 5
    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    with pytest.raises(ValueError, match="gatv2_attention_edge: e must be float32, not torch.float64"):
        pg.gatv2_attention_edge(where, g(x), g(x), g(a), g(e.double()))
    elsewhere = _fake_pattern()
    elsewhere.device = torch.device("cuda", 1)
    with pytest.raises(ValueError, match="gatv2_attention_edge: e lives on cpu, the pattern on cuda:1"):
        pg.gatv2_attention_edge(elsewhere, g(x), g(x), g(a), g(e))
    for bad, got in ((torch.zeros(6, 4, 8), "(6, 4, 8)"), (torch.zeros(4, 4, 8), "(4, 4, 8)"), (torch.zeros(5, 4, 4), "(5, 4, 4)"),
                     (torch.zeros(5, 2, 8), "(5, 2, 8)"), (torch.zeros(5, 32), "(5, 32)"), (torch.zeros(5), "(5,)")):
        with pytest.raises(ValueError, match=r"gatv2_attention_edge: e \[5, 4, 8\] expected for E = 5 entries") as err:
            pg.gatv2_attention_edge(where, g(x), g(x), g(a), g(bad))
        assert str(err.value).endswith("got " + got), str(err.value)
    x2, a2 = torch.zeros(3, 8), torch.zeros(8)
    with pytest.raises(ValueError, match=r"gatv2_attention_edge: e \[5, 8\] expected"):
        pg.gatv2_attention_edge(where, g(x2), g(x2), g(a2), g(torch.zeros(5, 1, 8)))
    # what gatv2_attention refuses of the other tensors, under this op's name
    with pytest.raises(ValueError, match=r"gatv2_attention_edge: a \(4, 4\) does not match x_dst"):
        pg.gatv2_attention_edge(where, g(x), g(x), g(torch.zeros(4, 4)), g(e))
    with pytest.raises(ValueError, match="gatv2_attention_edge: F = 12"):
        pg.gatv2_attention_edge(where, g(torch.zeros(3, 4, 12)), g(torch.zeros(3, 4, 12)), g(torch.zeros(4, 12)), g(torch.zeros(5, 4, 12)))


def test_a_strided_e_is_passed_by_its_leading_dimension():
    from pygat_amd.gatv2_attention import _edge_rows
    wide = torch.zeros(7, 40)
    e = wide[:, 4:36].view(7, 4, 8)
    got, ld = _edge_rows(e, 32)
    assert ld == 40 and got.data_ptr() == e.data_ptr(), "a column slice at a 16-byte offset: read in place"
    got, ld = _edge_rows(wide[:, :32], 32)
    assert ld == 40 and got.data_ptr() == wide.data_ptr()
    got, ld = _edge_rows(torch.zeros(7, 4, 8), 32)
    assert ld == 32
    for odd in (wide[:, 1:33].view(7, 4, 8), torch.zeros(7, 42)[:, :32], torch.zeros(7, 4, 16)[:, :, :8], torch.zeros(7, 8, 4).transpose(1, 2)):
        got, ld = _edge_rows(odd, 32)
        assert ld == 32 and got.is_contiguous() and got.data_ptr() != odd.data_ptr(), "misaligned, odd or not row-dense: a copy"


# ------------------------------------------------------------------------------------------------------- what the cases cover
def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    edge = [c for c in cs.values() if isinstance(c, case.EdgeCase)]
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    cdeg = lambda c: torch.bincount(c.col, minlength=c.shape[1])  # noqa: E731
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            c, cv = cs[f"lanes-hub-{H}x{F}-{kind}-shared"], cs[f"lanes-hub-{H}x{F}-{kind}-separate"]
            assert c.x_dst.shape == (c.shape[0], H, F) and c.e.shape == (c.row.numel(), H, F) and c.a.shape == (H, F)
            assert c.v is None and c.shared and c.kind == kind and len(c.leaves) == 4 and c.names[-1] == "de"
            assert cv.v.shape == (cv.shape[1], H, F) and not cv.shared and cv.kind == kind and len(cv.leaves) == 5 and cv.leaves[-1] is cv.e
        c, cv = cs[f"lanes-asym-{H}x{F}-indices-shared"], cs[f"lanes-asym-{H}x{F}-graph-separate"]
        assert c.shared and c.kind == "indices" and not cv.shared and cv.kind == "graph" and cv.e.shape[1:] == (H, F)
    assert cs["lanes-hub-noaxis-indices-shared"].e.dim() == 2 and cs["lanes-asym-noaxis-graph-separate"].e.shape[1:] == (64,)
    hub, asym = cs["lanes-hub-8x16-graph-shared"], cs["lanes-asym-8x16-graph-separate"]
    assert int(deg(hub).max()) == 699 and int(cdeg(hub).max()) == 699, "a long row and a long column at every lane shape"
    assert int((deg(asym) == 1).sum()) > 0
    assert 0.95 < float(hub.e.std()) < 1.05 and all(0.7 < float(s) < 1.4 for s in hub.scores().std(0))
    for name in case.case_names("long"):
        c = cs[name]
        sd = c.scores().std(0)
        assert c.std == 3.0 and 2.5 < float(sd.mean()) < 3.5, (name, sd)
        assert float(c.coefficients().max()) > 0.5, name
    assert int((deg(cs["long-nine_hubs-8x16-graph-separate"]) == 521).sum()) == 9
    assert int(deg(cs["long-three_chunk_hub-3x8-indices-shared"]).max()) >= 4097
    for name in case.case_names("longcol-"):
        c = cs[name]
        assert c.kind == "indices" and bool((c.row[1:] < c.row[:-1]).any()), name
    assert int((cdeg(cs["longcol-nine_hubs-8x16-shared"]) == 521).sum()) == 9
    assert int(cdeg(cs["longcol-three_chunk_hub-8x16-separate"]).max()) >= 4097
    for name in ("rect-4x16-shared", "rect-3x8-separate", "repeats-8x16-shared", "repeats-8x16-separate", "composed-rect-3x8-separate",
                 "strided-rect-4x16-shared"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a row of e"
    assert cs["rect-4x16-shared"].shape == (300, 500) and int((deg(cs["rect-4x16-shared"]) == 0).sum()) == 100
    c = cs["tail-rect-3x8-shared"]
    assert c.shape == (310, 520) and int(c.row.max()) < 300 and int(c.col.max()) < 500, "rows and columns without entries at the end"
    c = cs["repeats-8x16-separate"]
    pairs = c.pairs
    assert pairs.shape[0] > 100 and torch.equal(c.row[pairs[:, 0]], c.row[pairs[:, 1]]) and torch.equal(c.col[pairs[:, 0]], c.col[pairs[:, 1]])
    assert bool((c.e[pairs[:, 0]] != c.e[pairs[:, 1]]).flatten(1).any(1).all())
    leaves = [t.clone().requires_grad_(True) for t in c.leaves]
    de64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))[-1]
    assert bool((de64[pairs[:, 0]] != de64[pairs[:, 1]]).flatten(1).any(1).all()), "the two entries of a pair get different rows of de"
    assert int((deg(cs["lonely-8x16-indices-shared"]) == 1).sum()) >= 12 and int((deg(cs["lonely-3x8-graph-separate"]) == 1).sum()) >= 12
    zero = case.case_names("zero-")
    assert len(zero) == 6
    for name in zero:
        c = cs[name]
        p = case.plain.cases()[name[len("zero-"):]]
        assert float(c.e.abs().max()) == 0.0 and c.inner is p and c.a is p.a and c.x_dst is p.x_dst and c.G is p.G and c.shared == p.shared
    assert {cs[n].H * cs[n].F for n in zero} >= {128, 768, 1024, 24}
    assert sorted({cs[n].slope for n in case.case_names("slope-")}) == [0.0, 0.2, 1.0]
    for name in case.case_names("slope-"):
        c = cs[name]
        assert bool((c.t() < 0).any()) and bool((c.t() > 0).any())
        if c.slope == 1.0:                                        # the score is linear: the second ground truth is the first
            lin = case.linear_scores(c.row, c.col, c.x_dst, c.x_src, c.a, c.e)
            assert float((c.scores() - lin).abs().max()) < 1e-12
    assert {cs[n].shared for n in case.case_names("slope-")} == {True, False}
    twice = case.case_names("twice-")
    assert any("longcol" in n for n in twice) and any("hub-" in n and "longcol" not in n for n in twice)
    assert {cs[n].shared for n in twice} == {True, False}
    assert {cs[n].shared for n in case.case_names("composed-")} == {True, False}
    assert {cs[n].shared for n in case.case_names("strided-")} == {True, False}
    md = cs["module-rect-2x8"]
    assert md.shape == (300, 500) and md.edge_attr.shape == (md.row.numel(), case.EDGE_DIM)
    assert [tuple(w.shape) for w in md.weights] == [(md.F_IN, md.H * md.F), (md.F_IN, md.H * md.F), (md.H, md.F),
                                                    (md.H * md.F, case.EDGE_DIM)]
    assert md.NAMES[-1] == "lin_edge.weight"
    assert max(c.row.numel() * c.H * c.F for c in edge) <= case.MAX_E_FLOATS == 1 << 23
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


def test_the_grid_case_has_entries_at_the_kink():
    """All three tables on the multiples of 2^-10 in [-4, 4]: both adds are exact in fp32, so t is the same number in fp32 and fp64,
    and some t are exactly 0.  There LeakyReLU takes the slope, in the value and in the derivative: the fp64 ground truth's de at such
    an element is S a slope, and a run that took 1 there would differ by S a (1 - slope)."""
    c = case.cases()["grid-hub-8x16-indices-separate"]
    for t in (c.x_dst, c.x_src, c.e):
        assert torch.equal(t, case.on_grid(t)) and float(t.abs().max()) <= 4.0
    t64, t32 = c.t(), c.t(torch.float32)
    assert torch.equal(t64, t32.double())
    at0 = t64 == 0
    assert int(at0.sum()) >= 20, int(at0.sum())
    leaves = [t.clone().requires_grad_(True) for t in c.leaves]
    de64 = torch.autograd.grad(c.ref(*leaves), leaves, c.G.reshape(-1))[-1]
    # de = S a g'(t): S from the elements beside the kink of the same (entry, head), where g' is 1 or the slope
    pos = (t64 > 0) & (c.a != 0)
    S = torch.where(pos, de64 / c.a, torch.zeros_like(de64)).sum(-1) / pos.sum(-1).clamp_min(1)
    want = (S[..., None] * c.a * c.slope)[at0]
    seen = pos.any(-1)[..., None].expand_as(at0)[at0]
    assert int(seen.sum()) >= 20 and float((de64[at0] - want)[seen].abs().max()) <= 1e-12 * float(de64.abs().max())
    assert float(want[seen].abs().max()) * (1 - c.slope) / c.slope > 1e-4, "taking 1 at the kink would move de far beyond the tolerance"


def test_no_case_has_an_entry_at_the_kink():
    """Asserted when a case is built, and again here; NEXT_SEED lists the cases that moved on."""
    cs = case.cases()
    for name, c in cs.items():
        if isinstance(c, case.EdgeCase):
            assert case.t3_signs_agree(c.row, c.col, c.x_dst, c.x_src, c.e), name
    assert cs["module-rect-2x8"].kinks() == 0
    assert set(case.NEXT_SEED) <= set(cs)
    # the rule sees a flip where there is one: (1 + 2^-24) - 1 - 2^-25 is positive in fp64, and the first add rounds it to zero in fp32
    row = col = torch.tensor([0])
    one = torch.tensor([[1.0]], dtype=torch.float64)
    assert not case.t3_signs_agree(row, col, one, torch.tensor([[2.0 ** -24]], dtype=torch.float64), -one - 2.0 ** -25 + 2.0 ** -24)
    assert case.t3_signs_agree(row, col, one, -one, torch.tensor([[0.0]], dtype=torch.float64))
    # and the band counts a triple that cancels to the last bits, not an exact zero
    h = torch.tensor([[[1.0, 1.0]]], dtype=torch.float64)
    e = torch.tensor([[[2.0 ** -30, 0.0]]], dtype=torch.float64)
    assert case.product_kinks3(row, col, h, -h, e) == 1 and case.product_kinks3(row, col, h, -h, torch.zeros_like(e)) == 0


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()


def test_a_row_of_one_entry_in_the_fp32_reference():
    """What the device is held to bit for bit, the fp32 ground truth meets in value: out_i = v_j and an all-zero row of de."""
    c = case.cases()["lonely-3x8-graph-separate"]
    res = c.stand_in()
    out, de = res[0], res[-1]
    single = torch.bincount(c.row, minlength=c.shape[0])[c.row] == 1
    rows, cols = c.row[single], c.col[single]
    assert torch.equal(out[rows], c.v.float()[cols]) and float(de[single].abs().max()) < 1e-6
