"""pygat_dot_attn_bf16_forward, the launcher of the inference forward on bfloat16 k and v tables (csrc/k19_dot_attention.hip, additive
under ABI 16), refuses bad arguments on the host, before anything is launched: no GPU is needed, and a fake non-null address stands
in for every device table (as in test_dot_attention_abi.py).  Also here, on the CPU: the refusals pygat_amd.dot_attention makes of
bfloat16 tables before it touches the device, what the seeded cases of tests/dot_attention_bf16_case.py cover, and every such case's
rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import dot_attention_bf16_case as case
from abi_support import DOT, DOT_BIAS, P, call, lib, msg as _msg  # noqa: F401

NAME = "dot_attn_bf16_forward"


def _forward(L, **kw):
    a = dict(n_rows=8, nnz=20, rowptr=P, col=P, perm=None, H=2, F=8, scale=0.5, q=P, ldq=16, k=P + 8, ldk=16, v=P + 8, ldv=16,
             bias=P + 4, bias_head_stride=1, out=P, ldo=16, ws=P)
    return call(L, "pygat_dot_attn_bf16_forward", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    s = "pygat_" + NAME
    assert s in lib.SYMBOLS and hasattr(lib.lib, s)
    assert re.search(r"\b" + s + r"\(", header)
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    fn = lib.lib.pygat_dot_attn_bf16_forward
    assert fn.restype is C.c_int
    assert fn.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p]
    # the four launchers beside it keep their signatures
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p, p]
    assert len(lib.lib.pygat_dot_attn_backward_rows.argtypes) == 26 and len(lib.lib.pygat_dot_attn_bias_backward_rows.argtypes) == 29


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20")])
def test_the_launcher_refuses_the_limits(lib, kw, needle):
    for bias in (P + 4, None):                                          # with and without a bias
        assert _forward(lib, bias=bias, **kw) == -1, kw
        assert needle in _msg(lib) and _msg(lib).startswith(NAME + ": "), (kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    assert _forward(lib, F=12) == -1
    assert "power of two in 4..256" in _msg(lib) and "zero-padding the columns of q, k and v" in _msg(lib), _msg(lib)


def test_the_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short.  k and v are rows of bf16
    values whose chunk of 4 is 8 bytes: an address that is 8 bytes off a 16-byte line passes (the stand-in is one), 4 or 2 bytes off
    does not; q, out and the workspace keep the 16-byte rule.  perm may be null: the caller's order; bias may be null: no bias."""
    for ptr, ld, align in (("q", "ldq", 16), ("k", "ldk", 8), ("v", "ldv", 8), ("out", "ldo", 16)):
        assert _forward(lib, **{ptr: None}) == -1 and _msg(lib) == f"{NAME}: null {ptr}", (ptr, _msg(lib))
        for off in ((4, 8) if align == 16 else (4, 2, 12)):
            assert _forward(lib, **{ptr: P + off}) == -1, (ptr, off)
            assert _msg(lib) == f"{NAME}: {ptr} must be {align}-byte aligned", (ptr, off, _msg(lib))
        for short in (15, 12, 18):                                      # below H x F = 16; a stride that is no multiple of 4 elements
            assert _forward(lib, **{ld: short}) == -1, (ld, short)
            assert f"the row stride of {ptr}, {short}," in _msg(lib) and _msg(lib).startswith(NAME), (ld, _msg(lib))
    for ptr in ("rowptr", "col", "ws"):
        want = f"{NAME}: null {'workspace' if ptr == 'ws' else ptr}"
        assert _forward(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    assert _forward(lib, ws=P + 8) == -1 and _msg(lib) == f"{NAME}: the workspace must be 16-byte aligned"
    for stride in (2, -1, 8):
        assert _forward(lib, bias_head_stride=stride) == -1, stride
        assert _msg(lib).startswith(f"{NAME}: bias_head_stride={stride},"), _msg(lib)


def test_a_null_bias_is_no_bias(lib):
    """Without a bias neither perm nor bias_head_stride is looked at: with n_rows = 0 and no entries the call passes every check and
    returns before it launches anything."""
    assert _forward(lib, n_rows=0, nnz=0, bias=None, bias_head_stride=7, perm=None) == 0
    assert _forward(lib, n_rows=0, nnz=0, bias=None, col=None) == 0
    assert _forward(lib, n_rows=0, nnz=0, bias=P + 4, bias_head_stride=0) == 0
    assert _forward(lib, n_rows=0, nnz=0, bias=P + 4, bias_head_stride=7) == -1


def test_the_same_wording_as_the_float32_launchers(lib):
    """Whatever pygat_dot_attn_forward / pygat_dot_attn_bias_forward refuse, this launcher refuses in the same words after its own
    name (k and v: the same but for the 8 bytes of their alignment)."""
    for other, oname, mine in ((DOT[0][0], "dot_attn_forward", dict(bias=None)),
                               (DOT_BIAS[0][0], "dot_attn_bias_forward", dict())):
        for kw in (dict(H=65), dict(F=12), dict(H=8, F=256), dict(nnz=-1), dict(nnz=1 << 31), dict(n_rows=0), dict(q=None),
                   dict(q=P + 4), dict(k=None), dict(ldv=12), dict(ldk=18), dict(out=P + 8), dict(ws=None), dict(ws=P + 8),
                   dict(col=None), dict(rowptr=None)):
            assert _forward(lib, **mine, **kw) == -1
            got = _msg(lib)
            assert other(lib, **kw) == -1
            assert got[len(NAME):] == _msg(lib)[len(oname):] and got.startswith(NAME), (kw, got, _msg(lib))
    assert _forward(lib, bias_head_stride=3) == -1
    got = _msg(lib)
    assert DOT_BIAS[0][0](lib, bias_head_stride=3) == -1 and got[len(NAME):] == _msg(lib)[len("dot_attn_bias_forward"):]


def _fake_pattern():
    """An EdgePattern that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    pattern = object.__new__(pg.EdgePattern)
    pattern.device = torch.device("cuda", 0)
    pattern.n_rows = pattern.n_cols = 3
    return pattern


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    sig = inspect.signature(pg.dot_attention)
    assert list(sig.parameters) == ["pattern", "q", "k", "v", "scale", "bias"]
    doc = pg.dot_attention.__doc__
    assert "bfloat16" in doc and "torch.no_grad()" in doc and "-9e15" in doc and "unmasked" in doc
    assert "bfloat16" in inspect.getmodule(pg.dot_attention).__doc__
    z, h = torch.zeros(3, 4), torch.zeros(3, 4, dtype=torch.bfloat16)
    for k, v in ((h, z), (z, h), (h, z.half()), (z.double(), h), (h, None)):
        with pytest.raises(ValueError, match="dot_attention: k is .* and v is .*both k and v as bfloat16"):
            pg.dot_attention(_fake_pattern(), z, k, v)
    with pytest.raises(ValueError, match="dot_attention.*EdgePattern"):
        pg.dot_attention(object(), z, h, h)
    with pytest.raises(ValueError, match="dot_attention: q must be a tensor on the GPU"):
        pg.dot_attention(_fake_pattern(), z, h, h)                      # (no CPU path for these tables either)
    for bad in ([0.0, 1.0], torch.zeros(3)):
        with pytest.raises(ValueError, match="dot_attention: bias must be a tensor on the GPU"):
            pg.dot_attention(_fake_pattern(), z, h, h, bias=bad)
    # inference only: grad mode on and a tensor that requires grad -> refused, and the message names the way out
    for needs in ((True, False, False), (False, True, False), (False, False, True)):
        q, k, v = (t.clone().requires_grad_(n) for t, n in zip((z, h, h), needs))
        with pytest.raises(ValueError, match="dot_attention: bfloat16 k and v are for inference") as err:
            pg.dot_attention(_fake_pattern(), q, k, v)
        assert "torch.no_grad()" in str(err.value) and "float32 tables" in str(err.value)
    with pytest.raises(ValueError, match="bfloat16 k and v are for inference"):
        pg.dot_attention(_fake_pattern(), z, h, h, bias=torch.zeros(3, requires_grad=True))
    with torch.no_grad():                                               # under no_grad the same call gets as far as the next refusal
        with pytest.raises(ValueError, match="q must be a tensor on the GPU"):
            pg.dot_attention(_fake_pattern(), z.clone().requires_grad_(True), h, h)
    # what is refused today stays refused in today's words
    with pytest.raises(ValueError, match="edge_dot: q must be a tensor on the GPU"):
        pg.edge_dot(_fake_pattern(), z, h)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for c in cs.values():
        assert c.k16.dtype == torch.bfloat16 and c.v16.dtype == torch.bfloat16 and c.k16.shape == c.inner.k.shape
        assert torch.equal(c.k16.double().float().bfloat16(), c.k16), "widening is exact"
        for wide, narrow in ((c.inner.k, c.k16), (c.inner.v, c.v16)):
            assert float((narrow.double() != wide).double().mean()) >= 0.9, c.name
            assert float((narrow.double() - wide).abs().max()) <= 2.0 ** -8 * float(wide.abs().max()), "nearest: half a bf16 ulp"
    for H, F in case.LANE_SHAPES:
        for kind in ("indices", "graph"):
            c = cs[f"plain-lanes-hub-{H}x{F}-{kind}"]
            assert c.q.shape == (c.shape[0], H, F) and c.kind == kind and c.bias is None
    assert int(deg(cs["plain-lanes-hub-8x16-graph"]).max()) == 699
    H, F = case.WIDE_SHAPE
    assert H * F // 4 == 128 and not any(64 < h * f // 4 <= 128 for h, f in case.LANE_SHAPES), "two chunks per lane: only here"
    assert cs[f"plain-lanes-hub-{H}x{F}-indices"].q.shape[1:] == (H, F) and cs[f"bias-lanes-hub-{H}x{F}-graph"].bias.shape[1] == H
    for H, F in ((3, 8), (8, 16), (12, 64)):
        assert int((deg(cs[f"plain-lanes-asym-{H}x{F}-indices"]) == 1).sum()) > 0
    assert cs["plain-lanes-hub-noaxis-indices"].q.dim() == 2 and cs["bias-lanes-hub-noaxis-indices"].bias.dim() == 1
    for kind in ("indices", "graph"):
        assert int((deg(cs[f"plain-long-nine_hubs-8x16-{kind}"]) == 521).sum()) == 9
        assert int(deg(cs[f"plain-long-three_chunk_hub-3x8-{kind}"]).max()) >= 4097
    assert int(deg(cs["bias-masked-three_chunk_hub-3x8-graph"]).max()) >= 4097
    assert int((deg(cs["plain-lonely-8x16-graph"]) == 1).sum()) >= 12
    for name in ("bias-rect-3x8", "bias-rect-4x16", "bias-repeats-8x16", "bias-masked-rect-3x8"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a bias"
    for name in ("bias-shared-hub-8x16-indices", "bias-shared-hub-3x8-graph"):
        assert cs[name].bias.dim() == 1 and cs[name].H > 1
    for name in case.case_names("bias-masked-"):
        c = cs[name]
        assert int(c.masked.sum()) > 0.2 * c.row.numel() and bool((c.bias[c.masked] == case.biased.MASK).all())
    for name in case.case_names("bias-zero-"):
        c = cs[name]
        assert float(c.bias.abs().max()) == 0.0 and cs["plain-" + name[len("bias-zero-"):]].inner is c.inner.inner
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
