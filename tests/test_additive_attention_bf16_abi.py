"""pygat_add_attn_bf16_forward, the launcher of the inference forward on a bfloat16 v table (csrc/k20_additive_attention.hip, additive
under ABI 16), refuses bad arguments on the host, before anything is launched: no GPU is needed, and a fake non-null address stands in
for every device table (as in test_additive_attention_abi.py).  Also here, on the CPU: the refusals pygat_amd.additive_attention_bf16
makes before it touches the device, what the seeded cases of tests/additive_attention_bf16_case.py cover, and every such case's
rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import additive_attention_bf16_case as case
from abi_support import ADDITIVE, P, call, lib, msg as _msg  # noqa: F401

NAME = "add_attn_bf16_forward"


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, negative_slope=0.2, s_dst=P + 4, s_src=P + 4, v=P + 8, ldv=16,
             edge_logit=P + 4, logit_head_stride=1, out=P, ldo=16, ws=P)
    return call(L, "pygat_add_attn_bf16_forward", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    s = "pygat_" + NAME
    assert s in lib.SYMBOLS and hasattr(lib.lib, s)
    assert re.search(r"\b" + s + r"\(", header)
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    fn = lib.lib.pygat_add_attn_bf16_forward
    assert fn.restype is C.c_int
    # pygat_add_attn_forward's without m and Z
    assert fn.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p]
    # the launchers beside it keep their signatures
    assert lib.lib.pygat_add_attn_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, p]
    assert fn.argtypes == lib.lib.pygat_add_attn_forward.argtypes[:16] + [p, p]
    assert len(lib.lib.pygat_add_attn_backward_rows.argtypes) == 25
    assert len(lib.lib.pygat_add_attn_dropout_forward.argtypes) == 23 and len(lib.lib.pygat_add_attn_dropout_backward_rows.argtypes) == 28
    assert lib.lib.pygat_add_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_dot_attn_bf16_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p]


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "negative_slope=nan, a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "negative_slope=inf"),
                                       (dict(negative_slope=-float("inf")), "negative_slope=-inf")])
def test_the_launcher_refuses_the_limits(lib, kw, needle):
    for logit in (P + 4, None):                                         # with and without a logit
        assert _forward(lib, edge_logit=logit, **kw) == -1, kw
        assert needle in _msg(lib) and _msg(lib).startswith(NAME + ": "), (kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    assert _forward(lib, F=12) == -1
    assert "power of two in 4..256" in _msg(lib) and "zero-padding the columns of v to the next allowed F" in _msg(lib), _msg(lib)


def test_the_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short.  v is rows of bf16 values
    whose chunk of 4 is 8 bytes: an address that is 8 bytes off a 16-byte line passes (the stand-in is one), 4, 2 or 12 bytes off does
    not; out and the workspace keep the 16-byte rule; s_dst and s_src are read 4 bytes at a time.  perm may be null: the caller's
    order; edge_logit may be null: no term."""
    for ptr, ld, align in (("v", "ldv", 8), ("out", "ldo", 16)):
        assert _forward(lib, **{ptr: None}) == -1 and _msg(lib) == f"{NAME}: null {ptr}", (ptr, _msg(lib))
        for off in ((4, 8) if align == 16 else (4, 2, 12)):
            assert _forward(lib, **{ptr: P + off}) == -1, (ptr, off)
            assert _msg(lib) == f"{NAME}: {ptr} must be {align}-byte aligned", (ptr, off, _msg(lib))
        for short in (15, 12, 18):                                      # below H x F = 16; a stride that is no multiple of 4 elements
            assert _forward(lib, **{ld: short}) == -1, (ld, short)
            assert f"the row stride of {ptr}, {short}," in _msg(lib) and _msg(lib).startswith(NAME), (ld, _msg(lib))
    for ptr in ("rowptr", "col", "s_dst", "s_src", "ws"):
        want = f"{NAME}: null {'workspace' if ptr == 'ws' else ptr}"
        assert _forward(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    assert _forward(lib, ws=P + 8) == -1 and _msg(lib) == f"{NAME}: the workspace must be 16-byte aligned"
    for stride in (2, -1, 8):
        assert _forward(lib, logit_head_stride=stride) == -1, stride
        assert _msg(lib).startswith(f"{NAME}: logit_head_stride={stride},"), _msg(lib)
    # a null edge_logit selects the kernels without the term: its head stride is then not looked at, and nothing above changes
    assert _forward(lib, edge_logit=None, logit_head_stride=7, ws=None) == -1 and _msg(lib) == f"{NAME}: null workspace"


def test_neither_m_nor_z_is_asked_for(lib):
    """With n_rows = 0 and no entries the call passes every check and returns before it launches anything: there is no m and no Z to
    be null, with and without a logit."""
    assert _forward(lib, n_rows=0, nnz=0) == 0
    assert _forward(lib, n_rows=0, nnz=0, edge_logit=None, logit_head_stride=7, perm=None, col=None) == 0
    assert _forward(lib, n_rows=0, nnz=0, logit_head_stride=0) == 0
    assert _forward(lib, n_rows=0, nnz=0, logit_head_stride=7) == -1


def test_the_same_wording_as_the_float32_launcher(lib):
    """Whatever pygat_add_attn_forward refuses, this launcher refuses in the same words after its own name (v: the same but for the
    8 bytes of its alignment)."""
    for kw in (dict(H=65), dict(F=12), dict(H=8, F=256), dict(nnz=-1), dict(nnz=1 << 31), dict(n_rows=0), dict(v=None), dict(ldv=12),
               dict(ldv=18), dict(out=P + 8), dict(ws=None), dict(ws=P + 8), dict(col=None), dict(rowptr=None), dict(s_dst=None),
               dict(s_src=None), dict(logit_head_stride=3), dict(negative_slope=float("nan"))):
        assert _forward(lib, **kw) == -1
        got = _msg(lib)
        assert ADDITIVE[0][0](lib, **kw) == -1
        assert got[len(NAME):] == _msg(lib)[len("add_attn_forward"):] and got.startswith(NAME), (kw, got, _msg(lib))


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    pattern.n_rows = pattern.n_cols = 3
    return pattern


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    assert callable(pg.additive_attention_bf16) and "additive_attention_bf16" in pg.__all__
    assert pg.additive_attention_bf16.__module__ == "pygat_amd.additive_attention"
    sig = inspect.signature(pg.additive_attention_bf16)
    assert list(sig.parameters) == ["pattern", "s_dst", "s_src", "v16", "negative_slope", "edge_logit"]
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["edge_logit"].default is None
    doc = pg.additive_attention_bf16.__doc__
    assert "bit for bit" in doc and "torch.no_grad()" in doc and "v16.float()" in doc
    assert "additive_attention_bf16" in pg.additive_attention.__doc__ and "additive_attention_bf16" in inspect.getmodule(
        pg.additive_attention_bf16).__doc__
    z, zv = torch.zeros(3, 2), torch.zeros(3, 2, 4)
    h = zv.bfloat16()
    # a float32 tensor where bfloat16 is asked for, and the reverse: the message names the tensor and both dtypes
    for args, kw, name, want, got in (((z, z, zv), {}, "v16", "torch.bfloat16", "torch.float32"),
                                      ((z, z, zv.half()), {}, "v16", "torch.bfloat16", "torch.float16"),
                                      ((z.bfloat16(), z, h), {}, "s_dst", "torch.float32", "torch.bfloat16"),
                                      ((z, z.bfloat16(), h), {}, "s_src", "torch.float32", "torch.bfloat16"),
                                      ((z, z.double(), h), {}, "s_src", "torch.float32", "torch.float64"),
                                      ((z, z, h), dict(edge_logit=torch.zeros(5, 2).bfloat16()), "edge_logit", "torch.float32",
                                       "torch.bfloat16")):
        with pytest.raises(ValueError, match=f"additive_attention_bf16: {name} must be {want}, not {got}"):
            pg.additive_attention_bf16(_fake_pattern(), *args, **kw)
    with pytest.raises(ValueError, match="additive_attention_bf16: an EdgePattern expected"):
        pg.additive_attention_bf16(object(), z, z, h)
    with pytest.raises(ValueError, match="additive_attention_bf16: s_dst must be a tensor on the GPU"):
        pg.additive_attention_bf16(_fake_pattern(), z, z, h)            # (no CPU path for this table either)
    with pytest.raises(ValueError, match="additive_attention_bf16: s_dst must be a tensor on the GPU"):
        pg.additive_attention_bf16(_fake_pattern(), [0.0], z, h)
    for bad in ([0.0, 1.0], 1.0, torch.zeros(3)):
        with pytest.raises(ValueError, match="additive_attention_bf16: edge_logit must be a tensor on the GPU"):
            pg.additive_attention_bf16(_fake_pattern(), z, z, h, edge_logit=bad)
    for slope in (float("nan"), float("inf"), None, "0.2", True):
        with pytest.raises(ValueError, match="additive_attention_bf16: negative_slope = .* a finite float expected"):
            pg.additive_attention_bf16(_fake_pattern(), z, z, h, slope)
    # inference only: grad mode on and a tensor that requires grad -> refused, and the message names both ways out
    for needs in ((True, False, False), (False, True, False), (False, False, True)):
        args = [t.clone().requires_grad_(n) for t, n in zip((z, z, h), needs)]
        with pytest.raises(ValueError, match="additive_attention_bf16: bfloat16 tables are for inference") as err:
            pg.additive_attention_bf16(_fake_pattern(), *args)
        assert "torch.no_grad()" in str(err.value) and "use additive_attention on float32 tables" in str(err.value)
    with pytest.raises(ValueError, match="bfloat16 tables are for inference"):
        pg.additive_attention_bf16(_fake_pattern(), z, z, h, edge_logit=torch.zeros(5, requires_grad=True))
    with torch.no_grad():                                               # under no_grad the same call gets as far as the next refusal
        with pytest.raises(ValueError, match="s_dst must be a tensor on the GPU"):
            pg.additive_attention_bf16(_fake_pattern(), z.clone().requires_grad_(True), z, h)
    # what the float32 ops refuse today stays refused in today's words
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    where = _fake_pattern()
    where.device = torch.device("cpu")
    with pytest.raises(ValueError, match="additive_attention: v must be float32, not torch.bfloat16"):
        pg.additive_attention(where, *[t.as_subclass(OnGpu) for t in (z, z, h)])
    with pytest.raises(ValueError, match="additive_attention_dropout: s_dst, s_src, v and edge_logit must be float32"):
        pg.additive_attention_dropout(_fake_pattern(), z, z, h, 0.5)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for c in cs.values():
        assert c.v16.dtype == torch.bfloat16 and c.v16.shape == c.inner.v.shape and c.s_dst is c.inner.s_dst and c.u is c.inner.u
        assert torch.equal(c.v16.double().float().bfloat16(), c.v16), "widening is exact"
        assert case.changed(c.inner.v, c.v16) >= 0.9, c.name
        assert float((c.v16.double() - c.inner.v).abs().max()) <= 2.0 ** -8 * float(c.inner.v.abs().max()), "nearest: half a bf16 ulp"
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            c, cu = cs[f"lanes-hub-{H}x{F}-{kind}"], cs[f"lanes-hub-{H}x{F}-{kind}-logit"]
            assert c.v16.shape == (c.shape[1], H, F) and c.kind == kind and c.u is None and cu.u.shape == (cu.row.numel(), H)
    assert int(deg(cs["lanes-hub-8x16-graph"]).max()) == 699
    H, F = case.WIDE_SHAPE
    assert H * F // 4 == 128 and not any(64 < h * f // 4 <= 128 for h, f in case.LANE_SHAPES), "two chunks per lane: only here"
    assert cs[f"lanes-hub-{H}x{F}-indices"].v16.shape[1:] == (H, F) and cs[f"lanes-hub-{H}x{F}-graph-logit"].u.shape[1] == H
    shared = [n for n in case.case_names("lanes-hub-") if n.endswith("-shared")]
    assert len(shared) >= 4 and all(cs[n].u.dim() == 1 and cs[n].H > 1 for n in shared)
    for H, F in ((3, 8), (8, 16), (12, 64)):
        assert int((deg(cs[f"lanes-asym-{H}x{F}-indices"]) == 1).sum()) > 0
    assert cs["lanes-hub-noaxis-indices"].v16.dim() == 2 and cs["lanes-hub-noaxis-graph-logit"].u.dim() == 1
    assert int((deg(cs["long-nine_hubs-8x16-graph-shared"]) == 521).sum()) == 9
    assert int(deg(cs["long-three_chunk_hub-3x8-indices"]).max()) >= 4097
    for name in ("rect-4x16", "rect-3x8-logit", "repeats-8x16", "repeats-8x16-logit", "masked-rect-3x8"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a logit"
    assert cs["rect-4x16"].shape == (300, 500) and cs["repeats-8x16-logit"].pairs.shape[0] > 100
    assert int((deg(cs["lonely-8x16-graph-logit"]) == 1).sum()) >= 12
    assert len(case.case_names("zero-")) == 3 and all(float(cs[n].u.abs().max()) == 0.0 for n in case.case_names("zero-"))
    for name in case.case_names("masked-"):
        c = cs[name]
        assert int(c.masked.sum()) > 0.2 * c.row.numel() and bool((c.u[c.masked] == case.base.MASK).all()) and c.slope > 0
    assert int(deg(cs["masked-three_chunk_hub-3x8-graph"]).max()) >= 4097
    assert sorted(case.case_names("twice-")) == ["twice-hub-3x8-graph", "twice-nine_hubs-8x16-indices-logit"]
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
