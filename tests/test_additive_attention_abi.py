"""The launchers of csrc/k20_additive_attention.hip (additive under ABI 16) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table (as in test_dot_attention_abi.py).  Also here, on the
CPU: the refusals pygat_amd.additive_attention makes before it touches a device, what the seeded cases of
tests/additive_attention_case.py cover, and every such case's rehearsal with the fp32 ground-truth run standing in for the device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

import additive_attention_case as case
from abi_support import ADDITIVE, DOT, P, lib, msg as _msg  # noqa: F401

NEW = ("pygat_add_attn_workspace_bytes", "pygat_add_attn_forward", "pygat_add_attn_backward_rows")


LAUNCHERS = ADDITIVE
_forward, _backward = (fn for fn, _ in LAUNCHERS)
TABLES = {"add_attn_forward": (("v", "ldv"), ("out", "ldo")), "add_attn_backward_rows": (("v", "ldv"), ("out", "ldo"), ("G", "ldg"))}
SCALARS = {"add_attn_forward": ("rowptr", "col", "s_dst", "s_src", "m", "Z", "ws"),
           "add_attn_backward_rows": ("rowptr", "col", "s_dst", "s_src", "m", "Z", "ds_dst", "P", "S", "ws")}


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    assert "K20" in header and "csrc/k20_additive_attention.hip" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert "attention" not in s
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    assert lib.lib.pygat_add_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_add_attn_forward.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, p]
    assert lib.lib.pygat_add_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, p, p, i64, p, i, p, i64, p, p, p, i64, p, p, p,
                                                             p, p]
    # every K19 signature pinned elsewhere is as it was
    assert lib.lib.pygat_dot_attn_workspace_bytes.argtypes == [i64, i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_dot_attn_forward.argtypes == [i, i64, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i64, p, p, p, i64, p,
                                                             i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_forward.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p, p]
    assert lib.lib.pygat_dot_attn_bias_backward_rows.argtypes == [i, i64, p, p, p, i, i, f, p, i64, p, i64, p, i64, p, i, p, i64, p, p, p,
                                                                  i64, p, i64, p, p, p, p, p]


def test_exported_name_and_signature():
    import pygat_amd as pg
    assert callable(pg.additive_attention) and "additive_attention" in pg.__all__
    assert pg.additive_attention.__module__ == "pygat_amd.additive_attention"
    sig = inspect.signature(pg.additive_attention)
    assert list(sig.parameters) == ["pattern", "s_dst", "s_src", "v", "negative_slope", "edge_logit"]
    assert sig.parameters["negative_slope"].default == 0.2 and sig.parameters["edge_logit"].default is None
    doc = pg.additive_attention.__doc__
    assert "-9e15" in doc and "does not mask at negative_slope == 0" in doc
    for absent in ("dropout", "bfloat16", "fused column pass"):
        assert absent in doc[doc.index("Not provided"):], absent
    import importlib
    mod, dot = (importlib.import_module(m) for m in ("pygat_amd.additive_attention", "pygat_amd.dot_attention"))
    assert mod._require_pattern is dot._require_pattern and mod._require_tensor is dot._require_tensor


def test_workspace_bytes(lib):
    f = lib.add_attn_workspace_bytes
    # one record of (acc [H F], m [H], Z [H]), rounded up to 4 floats, per (2048-entry chunk, piece slot); the H sums of dz fit in it
    for nnz, H, F in ((20, 2, 8), (2049, 3, 8), (0, 1, 4), (10_760_000, 8, 64), (4097, 64, 16)):
        long_records = (-(-nnz // 2048) if nnz else 1) * 5
        stride = (H * F + 2 * H + 3) & ~3
        assert f(nnz, H, F) == long_records * stride * 4 == lib.dot_attn_workspace_bytes(nnz, H, F), (nnz, H, F)
    for bad, needle in (((-1, 2, 8), "nnz"), ((1 << 31, 2, 8), "2^31"), ((20, 0, 8), "H=0"), ((20, 65, 8), "H=65"), ((20, 2, 12), "F=12"),
                        ((20, 2, 512), "F=512"), ((20, 2, 3), "F=3"), ((20, 8, 256), "8 x 256")):
        with pytest.raises(ValueError, match=re.escape(needle)):
            f(*bad)
    assert lib.lib.pygat_add_attn_workspace_bytes(20, 2, 8, None) == -1 and _msg(lib) == "add_attn_workspace_bytes: null bytes"
    assert lib.lib.pygat_add_attn_workspace_bytes(0, 0, 0, None) < 0 and len(_msg(lib)) > 0


@pytest.mark.parametrize("kw,needle", [(dict(H=0), "H=0"), (dict(H=65), "H=65"), (dict(F=12), "F=12"), (dict(F=512), "F=512"),
                                       (dict(F=2), "F=2"), (dict(H=8, F=256), "8 x 256"), (dict(H=64, F=32), "64 x 32"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(nnz=-1), "nnz"), (dict(n_rows=-1), "n_rows=-1"),
                                       (dict(n_rows=0), "n_rows=0 with nnz=20"),
                                       (dict(negative_slope=float("nan")), "negative_slope=nan, a finite slope expected"),
                                       (dict(negative_slope=float("inf")), "negative_slope=inf"),
                                       (dict(negative_slope=-float("inf")), "negative_slope=-inf")])
def test_every_launcher_refuses_the_limits(lib, kw, needle):
    for fn, name in LAUNCHERS:
        assert fn(lib, **kw) == -1, (name, kw)
        assert needle in _msg(lib) and _msg(lib).startswith(name + ": "), (name, kw, _msg(lib))


def test_a_width_that_is_refused_names_the_way_out(lib):
    for fn, name in LAUNCHERS:
        assert fn(lib, F=12) == -1
        assert "power of two in 4..256" in _msg(lib) and "zero-padding the columns of v to the next allowed F" in _msg(lib), _msg(lib)


def test_each_launcher_refuses_its_own_tables(lib):
    """Every pointer on its own: the message names the one that is null, misaligned or strided too short (perm may be null: the
    caller's order; s_dst, s_src and ds_dst are read and written 4 bytes at a time: no alignment beyond that)."""
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
        # a null edge_logit selects the kernels without the term: its head stride is then not looked at, and nothing above changes
        assert fn(lib, edge_logit=None, logit_head_stride=7, ws=None) == -1 and _msg(lib) == f"{name}: null workspace"


def test_the_same_wording_as_dot_attention(lib):
    """Whatever pygat_dot_attn_forward / _backward_rows refuse of the arguments both families have, these refuse in the same words
    after their own name."""
    for (fn, name), (pfn, pname) in zip(LAUNCHERS, DOT):
        for kw in (dict(H=65), dict(nnz=-1), dict(n_rows=0), dict(v=None), dict(v=P + 4), dict(ldv=12), dict(m=None), dict(ws=None),
                   dict(ws=P + 8), dict(col=None), dict(out=P + 8)):
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


def test_python_refusals_that_need_no_gpu():
    import pygat_amd as pg
    z, zv = torch.zeros(3, 2), torch.zeros(3, 2, 4)
    with pytest.raises(ValueError, match="additive_attention: an EdgePattern expected"):
        pg.additive_attention(object(), z, z, zv)
    with pytest.raises(ValueError, match="additive_attention: an EdgePattern expected"):
        pg.additive_attention(object(), z, z, zv, edge_logit=torch.zeros(3))
    for name, args in (("s_dst", (z, z.double(), zv)), ("s_dst", ([0.0], z, zv))):
        with pytest.raises(ValueError, match=f"additive_attention: {name} must be a tensor on the GPU"):        # a CPU tensor
            pg.additive_attention(_fake_pattern(), *args)
    for bad in ([0.0, 1.0], 1.0, torch.zeros(3), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(ValueError, match="additive_attention: edge_logit must be a tensor on the GPU"):
            pg.additive_attention(_fake_pattern(), z, z, zv, edge_logit=bad)
    for slope in (float("nan"), float("inf"), -float("inf"), None, "0.2", True):
        with pytest.raises(ValueError, match="additive_attention: negative_slope = .* a finite float expected"):
            pg.additive_attention(_fake_pattern(), z, z, zv, slope)
    # a wrong dtype, on a tensor that says it lives on the GPU (the dtype is looked at before the device is)
    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    where = _fake_pattern()
    where.device = torch.device("cpu")                              # (so that the float32 tensors in front of the wrong one pass)
    for name, args, kw in (("s_dst", (z.double(), z, zv), {}), ("s_src", (z, z.half(), zv), {}), ("v", (z, z, zv.bfloat16()), {}),
                           ("edge_logit", (z, z, zv), dict(edge_logit=torch.zeros(3, 2, dtype=torch.float64)))):
        args = [t.as_subclass(OnGpu) for t in args]
        kw = {k: t.as_subclass(OnGpu) for k, t in kw.items()}
        with pytest.raises(ValueError, match=f"additive_attention: {name} must be float32, not torch."):
            pg.additive_attention(where, *args, **kw)


def test_the_cases_cover_what_they_are_meant_to():
    cs = case.cases()
    deg = lambda c: torch.bincount(c.row, minlength=c.shape[0])  # noqa: E731
    for H, F in case.LANE_SHAPES:
        for pname in ("hub", "asym"):
            for kind in ("indices", "graph"):
                c, cu = cs[f"lanes-{pname}-{H}x{F}-{kind}"], cs[f"lanes-{pname}-{H}x{F}-{kind}-logit"]
                assert c.s_dst.shape == (c.shape[0], H) and c.v.shape == (c.shape[1], H, F) and c.u is None and c.kind == kind
                assert cu.u.shape == (cu.row.numel(), H) and cu.kind == kind and 0.9 < float(cu.u.std()) < 1.1
    shared = [n for n in case.case_names("lanes-") if n.endswith("-shared")]
    assert len(shared) >= 8 and all(cs[n].u.dim() == 1 and cs[n].H > 1 for n in shared)
    for pname in ("hub", "asym"):
        for kind in ("indices", "graph"):
            c, cu = cs[f"lanes-{pname}-noaxis-{kind}"], cs[f"lanes-{pname}-noaxis-{kind}-logit"]
            assert c.s_dst.dim() == 1 and c.v.dim() == 2 and cu.u.dim() == 1 and cu.s_src.dim() == 1
    assert int(deg(cs["lanes-hub-8x16-graph"]).max()) == 699 and int((deg(cs["lanes-asym-8x16-graph"]) == 1).sum()) > 0
    for name in case.case_names("long-"):
        c = cs[name]
        assert 2.8 < float(c.s_dst.std()) < 3.2 and float(c.coefficients().max()) > 0.5, name
    assert int((deg(cs["long-nine_hubs-8x16-graph"]) == 521).sum()) == 9 and int(deg(cs["long-three_chunk_hub-3x8-indices"]).max()) >= 4097
    for name in case.case_names("exact-"):
        c = cs[name]
        z = case.logits_z(c.row, c.col, c.s_dst, c.s_src, c.u)
        l = torch.nn.functional.leaky_relu(z, c.slope)
        assert c.slope == 0.5 and torch.equal(4 * z, (4 * z).round()) and float(z.abs().min()) >= 0.25, name
        assert torch.equal(l.float().double(), l) and torch.equal(8 * l, (8 * l).round()) and bool((z < 0).any()) and bool((z > 0).any())
    for name in ("rect-4x16", "rect-3x8-logit", "repeats-8x16", "repeats-8x16-logit", "masked-rect-3x8", "composed-rect-3x8-shared"):
        c = cs[name]
        assert bool((c.row[1:] < c.row[:-1]).any()) and c.kind == "indices", f"{name}: unsorted, so only the permutation places a logit"
    assert cs["rect-4x16"].shape == (300, 500) and int((deg(cs["rect-4x16"]) == 0).sum()) == 100
    c = cs["repeats-8x16-logit"]
    assert c.pairs.shape[0] > 100 and bool((c.u[c.pairs[:, 0]] != c.u[c.pairs[:, 1]]).all())
    alpha = c.coefficients()
    assert bool((alpha[c.pairs[:, 0]] != alpha[c.pairs[:, 1]]).all())
    assert int((deg(cs["lonely-8x16-graph-logit"]) == 1).sum()) >= 12
    for name in case.case_names("zero-"):
        assert float(cs[name].u.abs().max()) == 0.0 and cs[name].u.shape == (cs[name].row.numel(), cs[name].H)
    assert int(deg(cs["zero-three_chunk_hub-8x16-indices"]).max()) >= 4097
    for name in case.case_names("masked-"):
        c = cs[name]
        E = c.row.numel()
        assert c.slope > 0 and 0.2 * E < int(c.masked.sum()) < 0.4 * E, (name, int(c.masked.sum()), E)
        assert bool((c.u[c.masked] == case.MASK).all()) and bool((c.u[~c.masked].abs() < 10.0).all())
        assert not bool((c.masked & case.first_of_row(c.row)).any()), "every row keeps an unmasked entry"
        assert float(c.coefficients()[c.masked].abs().max()) == 0.0
    assert int(deg(cs["masked-three_chunk_hub-3x8-graph"]).max()) >= 4097
    # at slope 0 the same logit does not mask: LeakyReLU sends it to 0, the maximum of a row of negative scores
    c = cs["masked-rect-3x8"]
    z = case.logits_z(c.row, c.col, c.s_dst, c.s_src, c.u)
    flat = case.edge_softmax_ref(c.row, c.shape[0], torch.nn.functional.leaky_relu(z, 0.0))
    assert float(flat[c.masked].min()) > 0.0
    assert sorted(case.case_names("twice-")) == ["twice-hub-3x8-graph", "twice-nine_hubs-8x16-indices-logit"]
    lv, md = cs["level-hub-3x6"], cs["module-rect-4x8"]
    assert lv.F % 4 and lv.FP == 8 and lv.shape[0] == lv.shape[1] and md.shape == (300, 500)
    assert [tuple(w.shape) for w in md.weights] == [(md.F_IN, md.H * md.F), (md.H, 2 * md.F)]
    assert max(c.shape[0] for c in cs.values()) <= 4500 and max(c.row.numel() for c in cs.values()) <= 31000


def test_no_case_has_an_entry_at_the_kink():
    """The assertion every case with a logit makes when it is built, made again here, and the reason the others need none."""
    cs = case.cases()
    for name, c in cs.items():
        if isinstance(c, case.Case) and c.u is not None:
            assert case.kinks(c.row, c.col, c.s_dst, c.s_src, c.u) == 0, name
        elif isinstance(c, case.Case):                            # one correctly rounded add: the fp32 z has the sign of the fp64 z
            z64 = case.logits_z(c.row, c.col, c.s_dst, c.s_src)
            z32 = case.logits_z(c.row, c.col, c.s_dst.float(), c.s_src.float())
            assert torch.equal(torch.sign(z64), torch.sign(z32.double())), name
    # the band is what decides: a logit that cancels s_dst + s_src to the last bits is counted
    row, col = torch.tensor([0, 0]), torch.tensor([0, 1])
    s_dst, s_src = torch.tensor([[1.0]], dtype=torch.float64), torch.tensor([[0.5], [0.25]], dtype=torch.float64)
    assert case.kinks(row, col, s_dst, s_src, torch.tensor([[-1.5 + 2.0 ** -30], [1.0]], dtype=torch.float64)) == 1
    assert case.kinks(row, col, s_dst, s_src, torch.tensor([[-1.5], [1.0]], dtype=torch.float64)) == 0        # an exact zero is no kink


@pytest.mark.parametrize("name", case.case_names())
def test_seeded_case_passes_with_the_fp32_reference(name):
    """The rehearsal of every seeded GPU case: the fp32 ground-truth run in the device's place passes the pricing."""
    case.cases()[name].rehearse()
