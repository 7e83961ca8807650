"""The launchers of csrc/k21_gatv2_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table (as in test_additive_attention_abi.py).  Also here,
on the CPU: the refusals pygat_amd.gatv2_attention makes before it touches a device, what the seeded cases of
tests/gatv2_attention_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import gatv2_attention_case as case
from abi_support import ADDITIVE, GATV2, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_v2_attn_workspace_bytes", "pygat_v2_attn_forward", "pygat_v2_attn_backward_rows", "pygat_v2_attn_backward_cols")


LAUNCHERS = GATV2
_forward, _backward, _columns = (fn for fn, _ in LAUNCHERS)
TABLES = {"v2_attn_forward": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo")),
          "v2_attn_backward_rows": (("x_dst", "ldd"), ("x_src", "lds"), ("v", "ldv"), ("out", "ldo"), ("G", "ldg"), ("dx_dst", "lddx")),
          "v2_attn_backward_cols": (("x_dst", "ldd"), ("x_src", "lds"), ("dx_src", "lddx"))}
SCALARS = {"v2_attn_forward": ("rowptr", "col", "a", "m", "Z", "ws"),
           "v2_attn_backward_rows": ("rowptr", "col", "a", "m", "Z", "P", "S", "ws"),
           "v2_attn_backward_cols": ("rowptr_t", "row_t", "a", "S", "da", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    assert "K21" in header and "csrc/k21_gatv2_attention.hip" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert "attention" not in s and "dot_attn" not in s
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert lib.lib.pygat_v2_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_v2_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, i64, p,
                                                            i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_backward_cols.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, p, i64, p, p, p]
    # the K20 signatures pinned elsewhere are as they were
    assert lib.lib.pygat_add_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_add_attn_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, p]
    # the K13 coefficient launcher of the GATv2 level keeps its name; the new entry points do not resemble it
    assert "pygat_gatv2_attention" in lib.SYMBOLS


def test_exported_name_and_signature():
    import pygat_amd as pg
    assert callable(pg.gatv2_attention) and "gatv2_attention" in pg.__all__
    assert pg.gatv2_attention.__module__ == "pygat_amd.gatv2_attention"
    sig = inspect.signature(pg.gatv2_attention)
    assert list(sig.parameters) == ["pattern", "x_dst", "x_src", "a", "v", "negative_slope"]
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["v"].default is None
    doc = " ".join(pg.gatv2_attention.__doc__.split())
    assert "v=Whi" in doc and "v=None" in doc and "H * F <= 1024" in doc and "sum_f a[f] LeakyReLU(x_dst[i, f] + x_src[j, f])" in doc
    for absent in ("a per-entry term or edge features", "dropout on the coefficients", "bfloat16 tables",
                   "the value product fused into the column pass"):
        assert absent in doc[doc.index("Not provided"):], absent
    import importlib
    mod, dot = (importlib.import_module(m) for m in ("pygat_amd.gatv2_attention", "pygat_amd.dot_attention"))
    assert mod._require_pattern is dot._require_pattern and mod._require_tensor is dot._require_tensor


def _da_floats(nnz, H, F):
    """The da records of the column pass, H F floats each: one per 2048-entry chunk (the long-column kernel), four per work-group of
    the column kernel (its waves; a work-group per chunk, one for a pattern without entries) and 128 partial sums of the reduce."""
    chunks = -(-nnz // 2048)
    return (chunks + 4 * max(chunks, 1) + 128) * H * F


def test_workspace_bytes(lib):
    f = lib.v2_attn_workspace_bytes
    # one record of (acc [H F], m [H], Z [H]), rounded up to 4 floats, per (2048-entry chunk, piece slot) -- the H F sums of dx fit in
    # it -- as K19's and K20's; then the da records
    for nnz, H, F in ((20, 2, 8), (2049, 3, 8), (0, 1, 4), (10_760_000, 8, 64), (4097, 64, 16), (100_000, 1, 4)):
        long_records = (-(-nnz // 2048) if nnz else 1) * 5
        stride = (H * F + 2 * H + 3) & ~3
        assert f(nnz, H, F) == (long_records * stride + _da_floats(nnz, H, F)) * 4, (nnz, H, F)
        assert f(nnz, H, F) == lib.add_attn_workspace_bytes(nnz, H, F) + 4 * _da_floats(nnz, H, F) and f(nnz, H, F) % 16 == 0
    for bad, needle in (((-1, 2, 8), "nnz"), ((1 << 31, 2, 8), "2^31"), ((20, 0, 8), "H=0"), ((20, 65, 8), "H=65"), ((20, 2, 12), "F=12"),
                        ((20, 2, 512), "F=512"), ((20, 2, 3), "F=3"), ((20, 8, 256), "8 x 256")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            f(*bad)
    assert lib.lib.pygat_v2_attn_workspace_bytes(20, 2, 8, None) == -1 and _msg(lib) == "v2_attn_workspace_bytes: null bytes"
    assert lib.lib.pygat_v2_attn_workspace_bytes(0, 0, 0, None) < 0 and len(_msg(lib)) > 0


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n=-1), "=-1"),
                                       (dict(n=0), "=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "negative_slope=nan, a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "negative_slope=inf"),
                                       (dict(negative_slope=-float("inf")), "negative_slope=-inf")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        n = "n_cols" if name.endswith("cols") else "n_rows"
        mine = {(n if k == "n" else k): v for k, v in kw.items()}
        want = n + needle if "n" in kw else needle
        assert fn(lib, **mine) == -1, (name, kw)
        assert want in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, F=12) == -1
        assert "power of two in 4..256" in _msg(lib), _msg(lib)
        assert "zero-padding the columns of x_dst, x_src, a and v to the next allowed F" in _msg(lib), _msg(lib)
        assert "zero columns of a add nothing to a score" in _msg(lib), _msg(lib)


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order; v may be null: v is x_src; a and da are dense, 16-byte aligned)."""
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
        if "v" in dict(TABLES[name]):
            # a null v selects the shared-value kernels: its stride is then not looked at, and nothing above changes
            assert fn(lib, v=None, ldv=7, ws=None) == -1 and _msg(lib) == f"{name}: null workspace"
    assert _columns(lib, da=P + 4) == -1 and _msg(lib) == "v2_attn_backward_cols: da must be 16-byte aligned"


def test_the_same_wording_as_additive_attention(lib):
    """Whatever pygat_add_attn_forward / _backward_rows refuse of the arguments both families have, these refuse in the same words
    after their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS[:2], ADDITIVE):
        for kw in (dict(H=65), dict(nnz=-1), dict(n_rows=0), dict(n_rows=-1), dict(v=P + 4), dict(ldv=12), dict(m=None), dict(ws=None),
                   dict(ws=P + 8), dict(col=None), dict(rowptr=None), dict(out=P + 8), dict(out=None), dict(Z=None), dict(H=8, F=256),
                   dict(negative_slope=float("nan")), dict(nnz=1 << 31)):
            assert fn(lib, **kw) == -1
            mine = _msg(lib)
            assert pfn(lib, **kw) == -1
            assert mine[len(name):] == _msg(lib)[len(pname):] and mine.startswith(name), (kw, mine, _msg(lib))
    for kw in (dict(G=None), dict(G=P + 4), dict(ldg=12), dict(P=None), dict(S=None)):
        assert _backward(lib, **kw) == -1
        mine = _msg(lib)
        assert ADDITIVE[1][0](lib, **kw) == -1
        assert mine[len("v2_attn_backward_rows"):] == _msg(lib)[len("add_attn_backward_rows"):], (kw, mine, _msg(lib))


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    return pattern


def test_python_refusals_that_need_no_gpu():
    import pygat_amd as pg
    x, a = torch.zeros(3, 2, 4), torch.zeros(2, 4)
    with pytest.raises(ValueError, match="gatv2_attention: an EdgePattern expected"):
        pg.gatv2_attention(object(), x, x, a)
    with pytest.raises(ValueError, match="gatv2_attention: an EdgePattern expected"):
        pg.gatv2_attention(object(), x, x, a, v=x)
    for name, args in (("x_dst", (x, x.double(), a)), ("x_dst", ([0.0], x, a))):
        with pytest.raises(ValueError, match=f"gatv2_attention: {name} must be a tensor on the GPU"):          # a CPU tensor
            pg.gatv2_attention(_fake_pattern(), *args)
    for slope in (float("nan"), float("inf"), -float("inf"), None, "0.2", True):
        with pytest.raises(ValueError, match="gatv2_attention: negative_slope = .* a finite float expected"):
            pg.gatv2_attention(_fake_pattern(), x, x, a, None, slope)
    # a wrong dtype, on a tensor that says it lives on the GPU (the dtype is looked at before the device is)
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    where = _fake_pattern()
    where.device = torch.device("cpu")                              # (so that the float32 tensors in front of the wrong one pass)
    for name, args, kw in (("x_dst", (x.double(), x, a), {}), ("x_src", (x, x.half(), a), {}), ("a", (x, x, a.bfloat16()), {}),
                           ("v", (x, x, a), dict(v=x.double()))):
        args = [t.as_subclass(OnGpu) for t in args]
        kw = {k: t.as_subclass(OnGpu) for k, t in kw.items()}
        with pytest.raises(ValueError, match=f"gatv2_attention: {name} must be float32, not torch."):
            pg.gatv2_attention(where, *args, **kw)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    cdeg = lambda c: torch.bincount(c.col, minlength=c.shape[1])  # noqa: E731
    for H, F in case.LANE_SHAPES:
        for pname in ("hub", "asym"):
            for kind in ("indices", "graph"):
                c, cv = cs[f"lanes-{pname}-{H}x{F}-{kind}-shared"], cs[f"lanes-{pname}-{H}x{F}-{kind}-separate"]
                assert c.x_dst.shape == (c.shape[0], H, F) and c.x_src.shape == (c.shape[1], H, F) and c.a.shape == (H, F)
                assert c.v is None and c.shared and c.kind == kind and len(c.leaves) == 3
                assert cv.v.shape == (cv.shape[1], H, F) and not cv.shared and cv.kind == kind and len(cv.leaves) == 4
                assert not torch.equal(cv.v, cv.x_src)
    for pname in ("hub", "asym"):
        c, cv = cs[f"lanes-{pname}-noaxis-indices-shared"], cs[f"lanes-{pname}-noaxis-graph-separate"]
        assert c.x_dst.dim() == 2 and c.a.dim() == 1 and c.v is None and cv.v.dim() == 2 and cv.a.shape == (64,)
    hub, asym = cs["lanes-hub-8x16-graph-shared"], cs["lanes-asym-8x16-graph-shared"]
    assert int(deg(hub).max()) == 699 and int(cdeg(hub).max()) == 699, "a long row and a long column at every lane shape"
    assert int((deg(asym) == 1).sum()) > 0
    # the default cases: scores of about unit standard deviation per head
    assert all(0.7 < float(s) < 1.4 for s in hub.scores().std(0))
    for name in case.case_names("long"):
        c = cs[name]
        sd = c.scores().std(0)                                    # (a hub's own row enters half the entries: a head's spread varies)
        assert c.std == 3.0 and all(2.0 < float(s) < 4.0 for s in sd) and 2.7 < float(sd.mean()) < 3.3, (name, sd)
        assert float(c.coefficients().max()) > 0.5, name
    assert int((deg(cs["long-nine_hubs-8x16-graph-separate"]) == 521).sum()) == 9
    assert int(deg(cs["long-three_chunk_hub-3x8-indices-shared"]).max()) >= 4097
    for name in case.case_names("longcol-"):
        c = cs[name]
        assert c.kind == "indices" and bool((c.row[1:] < c.row[:-1]).any()), name
    assert int((cdeg(cs["longcol-nine_hubs-8x16-shared"]) == 521).sum()) == 9
    for name in ("longcol-three_chunk_hub-8x16-shared", "longcol-three_chunk_hub-3x8-shared", "longcol-three_chunk_hub-8x16-separate",
                 "same-longcol-three_chunk_hub-3x8", "twice-longcol-three_chunk_hub-8x16-separate"):
        assert int(cdeg(cs[name]).max()) >= 4097, f"{name}: the column pass meets a column of three chunks"
    for name in ("rect-4x16-shared", "rect-3x8-separate", "repeats-8x16-shared", "repeats-8x16-separate", "composed-rect-3x8-shared"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted"
    assert cs["rect-4x16-shared"].shape == (300, 500) and int((deg(cs["rect-4x16-shared"]) == 0).sum()) == 100
    c = cs["tail-rect-3x8-shared"]
    assert c.shape == (310, 520) and int(c.row.max()) < 300 and int(c.col.max()) < 500, "rows and columns without entries at the end"
    c = cs["repeats-8x16-separate"]
    assert c.pairs.shape[0] > 100 and torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]])
    assert torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])
    assert int((deg(cs["lonely-8x16-graph-separate"]) == 1).sum()) >= 12
    assert sorted({cs[n].slope for n in case.case_names("slope-")}) == [0.0, 0.2, 1.0]
    for name in case.case_names("slope-"):
        c = cs[name]
        t = c.x_dst[c.row] + c.x_src[c.col]
        assert bool((t < 0).any()) and bool((t > 0).any())
        if c.slope == 1.0:                                        # the score is linear: the second ground truth is the first
            assert float((c.scores() - case.linear_scores(c.row, c.col, c.x_dst, c.x_src, c.a)).abs().max()) < 1e-12
    assert {cs[n].shared for n in case.case_names("slope-")} == {True, False}
    assert all(cs[n].shared for n in case.case_names("same-")) and len(case.case_names("same-")) >= 3
    twice = case.case_names("twice-")
    assert any("longcol" in n for n in twice) and any("hub-" in n and "longcol" not in n for n in twice)
    assert {cs[n].shared for n in twice} == {True, False}
    lv, md = cs["level-hub-3x6"], cs["module-rect-2x8"]
    assert lv.F % 4 and lv.FP == 8 and lv.shape[0] == lv.shape[1] and lv.W.shape == (lv.H, 2 * lv.F_IN, lv.F) and md.shape == (300, 500)
    assert [tuple(w.shape) for w in md.weights] == [(md.F_IN, md.H * md.F), (md.F_IN, md.H * md.F), (md.H, md.F)]
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


def test_no_case_has_an_entry_at_the_kink():
    """Where the tables are the leaves t is one correctly rounded add: the fp32 t has the sign of the fp64 t, an exact zero included.
    The module case's tables are fp32 products: its band, asserted when it is built, is asserted again here."""
    cs = case.cases()
    for name, c in cs.items():
        if isinstance(c, case.Case):
            assert case.t_signs_agree(c.row, c.col, c.x_dst, c.x_src), name
    md = cs["module-rect-2x8"]
    W_l, W_r, _ = md.weights
    h_src, h_dst = (md.x_src @ W_l).view(-1, md.H, md.F), (md.x_dst @ W_r).view(-1, md.H, md.F)
    assert case.product_kinks(md.row, md.col, h_dst, h_src) == 0
    # the band is what decides: a pair of table entries that cancel to the last bits is counted, an exact zero is not
    row, col = torch.tensor([0, 0]), torch.tensor([0, 1])
    h_dst = torch.tensor([[[1.0, 1.0]]], dtype=torch.float64)
    assert case.product_kinks(row, col, h_dst, torch.tensor([[[-1.0 + 2.0 ** -30, 0.5]], [[0.25, 0.5]]], dtype=torch.float64)) == 1
    assert case.product_kinks(row, col, h_dst, torch.tensor([[[-1.0, 0.5]], [[0.25, 0.5]]], dtype=torch.float64)) == 0
    # and the sign rule sees a flip where there is one: 1 + (-1 - 2^-30) is negative in fp64 and zero once the second is rounded
    assert not case.t_signs_agree(row[:1], col[:1], torch.tensor([[1.0]], dtype=torch.float64),
                                  torch.tensor([[-1.0 - 2.0 ** -30]], dtype=torch.float64))


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes its pricing."""
    case.cases()[name].rehearse()
