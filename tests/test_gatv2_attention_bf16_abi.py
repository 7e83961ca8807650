"""pygat_v2_attn_bf16_forward and pygat_v2_attn_edge_bf16_forward, the launchers of the inference forwards on bfloat16 tables
(csrc/k21_gatv2_attention.hip, additive under ABI 16), refuse bad arguments on the host, before anything is launched: no GPU is needed,
and a fake non-null address stands in for every device table (as in test_gatv2_attention_abi.py).  Also here, on the CPU: the refusals
pygat_amd.gatv2_attention_bf16 and pygat_amd.gatv2_attention_edge_bf16 make before they touch the device, what the seeded cases of
tests/gatv2_attention_bf16_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import gatv2_attention_bf16_case as case
from abi_support import GATV2, GATV2_EDGE, P, call, lib, msg as _msg  # noqa: F401

H8 = P + 8        # 8 bytes off a 16-byte line: where a table of bf16 rows may begin and a table of floats may not


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=H8, lds=16, a=P, v=H8, ldv=16,
             out=P, ldo=16, ws=P)
    return call(L, "pygat_v2_attn_bf16_forward", a, **kw)


def _edge_forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, x_dst=P, ldd=16, x_src=H8, lds=16, a=P, v=H8,
             ldv=16, e=H8, lde=16, out=P, ldo=16, ws=P)
    return call(L, "pygat_v2_attn_edge_bf16_forward", a, **kw)


LAUNCHERS = ((_forward, "v2_attn_bf16_forward"), (_edge_forward, "v2_attn_edge_bf16_forward"))
TABLES = {"v2_attn_bf16_forward": (("x_dst", "ldd", 16), ("x_src", "lds", 8), ("v", "ldv", 8), ("out", "ldo", 16)),
          "v2_attn_edge_bf16_forward": (("x_dst", "ldd", 16), ("x_src", "lds", 8), ("v", "ldv", 8), ("out", "ldo", 16), ("e", "lde", 8))}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in ("pygat_v2_attn_bf16_forward", "pygat_v2_attn_edge_bf16_forward"):
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    # the fp32 forward launchers' lists without m and Z; perm where the fp32 launcher has it
    assert lib.lib.pygat_v2_attn_bf16_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p]
    assert lib.lib.pygat_v2_attn_edge_bf16_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, i64, p, p]
    # the launchers beside them keep their signatures; no new size query
    fwd, efwd = lib.lib.pygat_v2_attn_forward.argtypes, lib.lib.pygat_v2_attn_edge_forward.argtypes
    assert fwd == [i, i64, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, p, p, p]
    assert efwd == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_v2_attn_bf16_forward.argtypes == fwd[:16] + fwd[18:]
    assert lib.lib.pygat_v2_attn_edge_bf16_forward.argtypes == efwd[:19] + efwd[21:]
    assert len(lib.lib.pygat_v2_attn_backward_rows.argtypes) == 27 and len(lib.lib.pygat_v2_attn_backward_cols.argtypes) == 19
    assert len(lib.lib.pygat_v2_attn_edge_backward_rows.argtypes) == 31 and len(lib.lib.pygat_v2_attn_edge_backward_cols.argtypes) == 21
    assert len(lib.lib.pygat_v2_attn_dropout_forward.argtypes) == 24 and len(lib.lib.pygat_v2_attn_dropout_backward_rows.argtypes) == 30
    assert [s for s in lib.SYMBOLS if "v2_attn" in s and s.endswith("workspace_bytes")] == ["pygat_v2_attn_workspace_bytes"]
    assert not any("bf16_backward" in s or "bf16_dropout" in s or "dropout_bf16" in s for s in lib.SYMBOLS), "forward only, no dropout"


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "negative_slope=nan, a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "negative_slope=inf")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        for v in (H8, None):                                            # a table of its own, and v is x_src
            assert fn(lib, v=v, **kw) == -1, (name, kw)
            assert needle in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, F=12) == -1
        assert "power of two in 4..256" in _msg(lib) and "zero-padding the columns of x_dst, x_src, a and v" in _msg(lib), _msg(lib)


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short.  x_src, v and e are rows of
    bf16 values whose chunk of 4 is 8 bytes: an address that is 8 bytes off a 16-byte line passes (the stand-ins are), 4, 2 or 12 bytes
    off does not; x_dst, a, out and the workspace keep the 16-byte rule.  perm may be null: the caller's order; v may be null: v is
    x_src, its stride is then not looked at."""
    for fn, name in LAUNCHERS:
        for ptr, ld, align in TABLES[name]:
            if ptr != "v":
                assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == f"{name}: null {ptr}", (name, ptr, _msg(lib))
            for off in ((4, 8) if align == 16 else (4, 2, 12)):
                assert fn(lib, **{ptr: P + off}) == -1, (name, ptr, off)
                assert _msg(lib) == f"{name}: {ptr} must be {align}-byte aligned", (name, ptr, off, _msg(lib))
            for short in (15, 12, 18):                                  # below H x F = 16; a stride that is no multiple of 4 elements
                assert fn(lib, **{ld: short}) == -1, (name, ld, short)
                assert f"the row stride of {ptr}, {short}," in _msg(lib) and _msg(lib).startswith(name), (name, ld, _msg(lib))
        for ptr in ("rowptr", "col", "a", "ws"):
            want = f"{name}: null {'workspace' if ptr == 'ws' else ptr}"
            assert fn(lib, **{ptr: None}) == -1 and _msg(lib) == want, (name, ptr, _msg(lib))
        assert fn(lib, ws=P + 8) == -1 and _msg(lib) == f"{name}: the workspace must be 16-byte aligned"
        assert fn(lib, a=P + 8) == -1 and _msg(lib) == f"{name}: a must be 16-byte aligned"
        assert fn(lib, v=None, ldv=7, ws=None) == -1 and _msg(lib) == f"{name}: null workspace"
        # neither m nor Z is asked for: without rows and entries the call passes every check and launches nothing
        assert fn(lib, n_rows=0, nnz=0, col=None) == 0, _msg(lib)
        assert fn(lib, n_rows=0, nnz=0, v=None, ldv=7) == 0, _msg(lib)
    # the launcher's own tables come before e; without entries a null e is not refused, a misaligned one is
    name = "v2_attn_edge_bf16_forward"
    assert _edge_forward(lib, e=None, ws=None) == -1 and _msg(lib) == f"{name}: null workspace"
    assert _edge_forward(lib, n_rows=0, nnz=0, col=None, e=None, lde=0) == 0, _msg(lib)
    assert _edge_forward(lib, nnz=0, col=None, e=P + 4) == -1 and _msg(lib) == f"{name}: e must be 8-byte aligned"
    assert _edge_forward(lib, v=None, ldv=7, e=P + 12) == -1 and _msg(lib) == f"{name}: e must be 8-byte aligned"


def test_the_same_wording_as_the_float32_launchers(lib):
    """Whatever pygat_v2_attn_forward / pygat_v2_attn_edge_forward refuse, these launchers refuse in the same words after their own
    name (x_src, v and e: the same but for the 8 bytes of their alignment)."""
    for (fn, name), (pfn, pname) in ((LAUNCHERS[0], (GATV2[0][0], "v2_attn_forward")),
                                     (LAUNCHERS[1], (GATV2_EDGE[0][0], "v2_attn_edge_forward"))):
        for kw in (dict(H=65), dict(F=12), dict(H=8, F=256), dict(nnz=-1), dict(nnz=1 << 31), dict(n_rows=0), dict(x_dst=None),
                   dict(x_dst=P + 4), dict(x_src=None), dict(lds=15), dict(ldv=12), dict(ldd=18), dict(out=P + 8), dict(ws=None),
                   dict(ws=P + 8), dict(a=None), dict(a=P + 4), dict(col=None), dict(rowptr=None), dict(negative_slope=float("nan"))):
            assert fn(lib, **kw) == -1
            got = _msg(lib)
            assert pfn(lib, **kw) == -1
            assert got[len(name):] == _msg(lib)[len(pname):] and got.startswith(name), (kw, got, _msg(lib))
    for kw in (dict(e=None), dict(lde=12), dict(lde=18)):
        assert _edge_forward(lib, **kw) == -1
        got = _msg(lib)
        assert GATV2_EDGE[0][0](lib, **kw) == -1
        assert got[len("v2_attn_edge_bf16_forward"):] == _msg(lib)[len("v2_attn_edge_forward"):], (kw, got, _msg(lib))


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    pattern.n_rows = pattern.n_cols = 3
    return pattern


def test_python_signatures_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    for name in ("gatv2_attention_bf16", "gatv2_attention_edge_bf16"):
        assert callable(getattr(pg, name)) and name in pg.__all__ and getattr(pg, name).__module__ == "pygat_amd.gatv2_attention"
        doc = getattr(pg, name).__doc__
        assert "bit for bit" in doc and "torch.no_grad()" in doc and "x_src16.float()" in doc
        assert name in inspect.getmodule(pg.gatv2_attention).__doc__
    sig = inspect.signature(pg.gatv2_attention_bf16)
    assert list(sig.parameters) == ["pattern", "x_dst", "x_src16", "a", "v16", "negative_slope"]
    assert sig.parameters["v16"].default is None and sig.parameters["negative_slope"].default == 0.2
    sig = inspect.signature(pg.gatv2_attention_edge_bf16)
    assert list(sig.parameters) == ["pattern", "x_dst", "x_src16", "a", "e16", "v16", "negative_slope"]
    assert sig.parameters["v16"].default is None and sig.parameters["negative_slope"].default == 0.2
    assert "gatv2_attention_bf16" in pg.gatv2_attention.__doc__ and "gatv2_attention_edge_bf16" in pg.gatv2_attention_edge.__doc__
    x, a, e = torch.zeros(3, 4, 8), torch.zeros(4, 8), torch.zeros(5, 4, 8)
    xh, eh = x.bfloat16(), e.bfloat16()
    plain_op = lambda *args, **kw: pg.gatv2_attention_bf16(_fake_pattern(), *args, **kw)           # noqa: E731
    edge_op = lambda x_dst, x_src16, a, v16=None, e16=eh: pg.gatv2_attention_edge_bf16(_fake_pattern(), x_dst, x_src16, a, e16, v16)   # noqa: E731
    # a float32 tensor where bfloat16 is asked for, and the reverse: the message names the tensor and both dtypes
    for op, fn in (("gatv2_attention_bf16", plain_op), ("gatv2_attention_edge_bf16", edge_op)):
        for args, name, want, got in (((x, x, a), "x_src16", "torch.bfloat16", "torch.float32"),
                                      ((x, x.half(), a), "x_src16", "torch.bfloat16", "torch.float16"),
                                      ((xh, xh, a), "x_dst", "torch.float32", "torch.bfloat16"),
                                      ((x, xh, a.bfloat16()), "a", "torch.float32", "torch.bfloat16"),
                                      ((x, xh, a, x), "v16", "torch.bfloat16", "torch.float32"),
                                      ((x.double(), xh, a), "x_dst", "torch.float32", "torch.float64")):
            with pytest.raises(ValueError, match=f"{op}: {name} must be {want}, not {got}"):
                fn(*args)
        with pytest.raises(ValueError, match=f"{op}: an EdgePattern expected"):
            getattr(pg, op)(object(), x, xh, a, *((eh,) if "edge" in op else ()))
        first = "e16" if "edge" in op else "x_dst"                      # (e16 is looked at first, as gatv2_attention_edge looks at e)
        with pytest.raises(ValueError, match=f"{op}: {first} must be a tensor on the GPU"):
            fn(x, xh, a)                                                # (no CPU path for these tables either)
        for slope in (float("nan"), float("inf"), None, "0.2", True):
            with pytest.raises(ValueError, match=f"{op}: negative_slope = .* a finite float expected"):
                getattr(pg, op)(_fake_pattern(), x, xh, a, *((eh,) if "edge" in op else ()), negative_slope=slope)
        # inference only: grad mode on and a tensor that requires grad -> refused, and the message names both ways out
        for which in range(4):
            args = [t.clone().requires_grad_(k == which) for k, t in enumerate((x, xh, a, xh))]
            with pytest.raises(ValueError, match=f"{op}: bfloat16 tables are for inference") as err:
                fn(*args)
            assert "torch.no_grad()" in str(err.value) and f"use {op[:-5]} on float32 tables" in str(err.value)
        with torch.no_grad():                                           # under no_grad the same call gets as far as the next refusal
            with pytest.raises(ValueError, match=f"{first} must be a tensor on the GPU"):
                fn(x.clone().requires_grad_(True), xh, a)
    with pytest.raises(ValueError, match="gatv2_attention_edge_bf16: e16 must be torch.bfloat16, not torch.float32"):
        edge_op(x, xh, a, None, e)
    with pytest.raises(ValueError, match="gatv2_attention_edge_bf16: bfloat16 tables are for inference"):
        edge_op(x, xh, a, None, eh.clone().requires_grad_(True))
    for bad in (None, [0.0], 1.0):
        with pytest.raises(ValueError, match="gatv2_attention_edge_bf16: e16 must be a tensor on the GPU.*a row per entry"):
            edge_op(x, xh, a, None, bad)
    # what the float32 ops refuse today stays refused in today's words
    with pytest.raises(ValueError, match="gatv2_attention_edge: x_dst, x_src, a, v and e must be float32"):
        pg.gatv2_attention_edge(_fake_pattern(), x, xh, a, e)
    with pytest.raises(ValueError, match="gatv2_attention_dropout: x_dst, x_src, a and v must be float32"):
        pg.gatv2_attention_dropout(_fake_pattern(), x, xh, a, 0.5)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for c in cs.values():
        assert c.name.startswith("edge-") == c.edge == (c.e16 is not None) and (c.v16 is None) == c.shared
        for wide, narrow, on_grid in ((c.inner.x_src, c.x_src16, c.grid), (c.inner.v, c.v16, False), (getattr(c.inner, "e", None), c.e16, c.grid)):
            if narrow is None:
                continue
            assert narrow.dtype == torch.bfloat16 and narrow.shape == wide.shape
            assert torch.equal(narrow.double().float().bfloat16(), narrow), "widening is exact"
            assert float((narrow.double() - wide).abs().max()) <= 2.0 ** -8 * float(wide.abs().max()), "nearest: half a bf16 ulp"
            if float(wide.abs().max()) > 0.0:
                assert case.changed(wide, narrow) >= (0.5 if on_grid else 0.9), c.name
        assert c.x_dst is c.inner.x_dst and c.a is c.inner.a
    for prefix in ("plain", "edge"):
        for H, F in case.LANE_SHAPES + (case.WIDE_SHAPE,):
            names = [n for n in case.case_names(f"{prefix}-lanes-hub-{H}x{F}-")]
            assert {cs[n].shared for n in names} == {True, False} and {cs[n].kind for n in names} == {"indices", "graph"}, (prefix, H, F)
            assert all(cs[n].x_src16.shape[1:] == (H, F) for n in names)
        assert int(deg(cs[f"{prefix}-lanes-hub-8x16-graph-shared"]).max()) == 699
        for H, F in ((3, 8), (8, 16), (12, 64)):
            assert int((deg(cs[f"{prefix}-lanes-asym-{H}x{F}-indices-shared"]) == 1).sum()) > 0
        assert cs[f"{prefix}-lanes-hub-noaxis-indices-shared"].x_src16.dim() == 2
        assert cs[f"{prefix}-lanes-asym-noaxis-graph-separate"].v16.dim() == 2
        assert int((deg(cs[f"{prefix}-long-nine_hubs-8x16-graph-separate"]) == 521).sum()) == 9
        assert int(deg(cs[f"{prefix}-long-three_chunk_hub-3x8-indices-shared"]).max()) >= 4097
        for name in ("rect-4x16-shared", "rect-3x8-separate", "repeats-8x16-shared", "repeats-8x16-separate"):
            c = cs[f"{prefix}-{name}"]
            assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted entries"
        assert cs[f"{prefix}-rect-4x16-shared"].shape == (300, 500) and cs[f"{prefix}-repeats-8x16-shared"].pairs.shape[0] > 100
        assert len(case.case_names(f"{prefix}-lonely-")) >= 2
    H, F = case.WIDE_SHAPE
    assert H * F // 4 == 128 and not any(64 < h * f // 4 <= 128 for h, f in case.LANE_SHAPES), "two chunks per lane: only here"
    zeros = case.case_names("edge-zero-")
    assert len(zeros) == 6
    for name in zeros:
        c, p = cs[name], cs["plain-" + name[len("edge-zero-"):]]
        assert float(c.e16.float().abs().max()) == 0.0 and c.inner.inner is p.inner and torch.equal(c.x_src16, p.x_src16)
    g = cs["edge-grid-hub-8x16-indices-separate"]
    assert g.grid and int((g.inner.t() == 0).sum()) > 0
    for t in (g.x_src16, g.e16):
        steps = t.double() / case.edge.GRID
        assert torch.equal(steps, steps.round()) and float(t.float().abs().max()) <= 4.0
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
