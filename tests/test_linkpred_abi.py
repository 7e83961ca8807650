"""The K24 entry points (csrc/k24_linkpred.hip, additive under ABI 16) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table (as in test_subgraph_abi.py).  Also here, on the CPU:
the signatures of pygat_amd.find_edges / negative_edges / link_batch and their refusals that need no GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from abi_support import P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_find_edges", "pygat_draw_negatives")


def _find(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_pairs=8, row=P, colq=P, pos=P, info=P)
    return call(L, "pygat_find_edges", a, **kw)


def _draw(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_src=8, src=P, num_neg=5, exclude_self=1, seed=P, hop=0, neg=P, info=P)
    return call(L, "pygat_draw_negatives", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
        assert not any(word in s for word in ("sample", "walk", "subgraph", "weighted", "attention")), s
    p, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    assert lib.lib.pygat_find_edges.argtypes == [i, i64, p, p, i64, p, p, p, p, p]
    assert lib.lib.pygat_draw_negatives.argtypes == [i, i64, p, p, i64, p, i, i, p, u32, p, p, p]
    assert [s for s in lib.SYMBOLS if "find_edges" in s or "negatives" in s] == list(NEW)


@pytest.mark.parametrize("call,kw,needle", [
    ("find", dict(n=0), "n=0 nodes"), ("find", dict(n=-3), "n=-3 nodes"), ("find", dict(nnz=0), "nnz=0"), ("find", dict(nnz=1 << 31), "2^31"),
    ("find", dict(n_pairs=0), "n_pairs=0: 1 <= n_pairs < 2^31 pairs expected"), ("find", dict(n_pairs=-1), "n_pairs=-1"),
    ("find", dict(n_pairs=1 << 31), "n_pairs=2147483648"),
    ("draw", dict(n=0), "n=0 nodes"), ("draw", dict(nnz=0), "nnz=0"), ("draw", dict(nnz=1 << 31), "2^31"),
    ("draw", dict(n_src=0), "n_src=0: 1 <= n_src < 2^31 source nodes expected"), ("draw", dict(n_src=1 << 31), "n_src=2147483648"),
    ("draw", dict(num_neg=0), "num_neg=0: num_neg >= 1 draws per source node expected"), ("draw", dict(num_neg=-2), "num_neg=-2"),
    ("draw", dict(n_src=1 << 20, num_neg=1 << 11), "n_src=1048576 x num_neg=2048 draws: fewer than 2^31 expected"),
    ("draw", dict(n_src=(1 << 31) - 1, num_neg=2), "draws: fewer than 2^31 expected"),
    ("draw", dict(exclude_self=2), "exclude_self=2: 0 or 1 expected"), ("draw", dict(exclude_self=-1), "exclude_self=-1")])
def test_the_launchers_refuse_the_limits(lib, call, kw, needle):
    fn, prefix = {"find": (_find, "find_edges: "), "draw": (_draw, "draw_negatives: ")}[call]
    assert fn(lib, **kw) == -1, kw
    assert needle in _msg(lib) and _msg(lib).startswith(prefix), (kw, _msg(lib))


def test_the_launchers_refuse_their_own_tables(lib):
    for ptr in ("rowptr", "col", "row", "colq", "pos", "info"):
        assert _find(lib, **{ptr: None}) == -1 and _msg(lib) == f"find_edges: null {ptr}", (ptr, _msg(lib))
    for ptr in ("rowptr", "col", "src", "seed", "neg", "info"):
        assert _draw(lib, **{ptr: None}) == -1 and _msg(lib) == f"draw_negatives: null {ptr}", (ptr, _msg(lib))
    for ptr in ("row", "colq", "pos"):
        assert _find(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "find_edges: row, colq and pos must be 8-byte aligned"
    assert _draw(lib, seed=P + 4) == -1 and _msg(lib) == "draw_negatives: seed must be 8-byte aligned"
    for ptr in ("src", "neg"):
        assert _draw(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "draw_negatives: src and neg must be 8-byte aligned"


def test_with_every_pointer_null(lib):
    for name, prefix in zip(NEW, ("find_edges: ", "draw_negatives: ")):
        fn = getattr(lib.lib, name)
        args = [0 if t in (C.c_int, C.c_int64, C.c_uint32) else None for t in fn.argtypes]
        assert fn(*args) < 0 and _msg(lib).startswith(prefix)


def test_the_footprint_names(lib):
    regs, scratch = C.c_int(0), C.c_int(0)
    assert lib.lib.pygat_kernel_footprint(b"k24_nothing", C.byref(regs), C.byref(scratch)) == -1
    assert _msg(lib) == "kernel_footprint: unknown kernel 'k24_nothing' (k24_find, k24_draw)"


def _fake_graph(device="cpu"):
    """A CSRGraph that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    g = object.__new__(pg.CSRGraph)
    g.device, g.n, g.nnz = torch.device(device), 10, 30
    return g


def test_python_signatures_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    for name in ("find_edges", "negative_edges", "link_batch", "LinkBatch"):
        assert name in pg.__all__ and getattr(pg, name).__module__ == "pygat_amd.linkpred"
    assert list(inspect.signature(pg.find_edges).parameters) == ["graph", "row", "col"]
    assert list(inspect.signature(pg.CSRGraph.find_edges).parameters) == ["self", "row", "col"]
    assert list(inspect.signature(pg.CSRGraph.has_edges).parameters) == ["self", "row", "col"]
    assert list(inspect.signature(pg.CSRGraph.reverse_edge_ids).parameters) == ["self"]
    sig = inspect.signature(pg.negative_edges)
    assert list(sig.parameters) == ["graph", "src", "num_neg", "seed", "generator", "hop", "exclude_self", "allow_full"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator", "hop", "exclude_self", "allow_full"))
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["seed"], d["generator"], d["hop"], d["exclude_self"], d["allow_full"]) == (None, None, 0, True, False)
    sig = inspect.signature(pg.link_batch)
    assert list(sig.parameters) == ["graph", "edge_ids", "num_neg", "fanouts", "seed", "generator", "exclude", "edge_weight"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator", "exclude", "edge_weight"))
    assert sig.parameters["exclude"].default == "reverse" and sig.parameters["edge_weight"].default is None
    assert pg.LinkBatch._fields == ("blocks", "seeds", "pos_src", "pos_dst", "neg_dst", "pairs", "labels")
    for fn in (pg.find_edges, pg.negative_edges):
        doc = " ".join(fn.__doc__.split())
        assert "ONE host read" in doc and "stream capture" in doc and "no CPU path" in doc
    doc = " ".join(pg.link_batch.__doc__.split())
    for needle in ("Host reads, all of them", "range check of edge_ids", "negative_edges' ONE host read", "torch.unique", "reverse_edge_ids",
                   "one read per hop", "EdgePattern.from_indices", "stream capture", "self loops", "no CPU path"):
        assert needle in doc, needle

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    ids = torch.arange(4)
    calls = (("find_edges", "row", "n", lambda graph, t: pg.find_edges(graph, t, g(ids))),
             ("find_edges", "col", "n", lambda graph, t: pg.find_edges(graph, g(ids), t)),
             ("find_edges", "row", "n", lambda graph, t: pg.CSRGraph.find_edges(graph, t, g(ids))),
             ("find_edges", "row", "n", lambda graph, t: pg.CSRGraph.has_edges(graph, t, g(ids))),
             ("negative_edges", "src", "n_src", lambda graph, t: pg.negative_edges(graph, t, 5)),
             ("link_batch", "edge_ids", "B", lambda graph, t: pg.link_batch(graph, t, 5, [10])))
    for k, (op, name, size, call) in enumerate(calls):
        if k not in (2, 3):
            with pytest.raises(ValueError, match=f"{op}: a CSRGraph expected, not tuple"):
                call((ids, ids), g(ids))
        for bad in (ids, [0, 1], None):
            with pytest.raises(ValueError, match=f"{op}: {name} must be a tensor on the GPU"):
                call(_fake_graph(), bad)
        for bad in (ids.float(), ids.double(), ids.bool(), ids.to(torch.int16)):
            with pytest.raises(ValueError, match=f"{op}: {name} must be int32 or int64, not torch"):
                call(_fake_graph(), g(bad))
        for bad in (ids.view(2, 2), ids[:0]):
            with pytest.raises(ValueError, match=rf"{op}: {name} \[{size}\] with {size} >= 1 expected"):
                call(_fake_graph(), g(bad))
        first = "row" if op == "find_edges" else name           # (row is looked at before col, and both stand on the CPU here)
        with pytest.raises(ValueError, match=f"{op}: {first} lives on cpu, the graph on cuda:1"):
            call(_fake_graph("cuda:1"), g(ids))
    with pytest.raises(ValueError, match="find_edges: row holds 4 ids and col 3: one pair per index expected"):
        pg.find_edges(_fake_graph(), g(ids), g(ids[:3]))
    for op, call in (("negative_edges", lambda k: pg.negative_edges(_fake_graph(), g(ids), k)),
                     ("link_batch", lambda k: pg.link_batch(_fake_graph(), g(ids), k, [10]))):
        for bad in (0, -1, 2.0, True, "3", None, 2 ** 31):
            with pytest.raises(ValueError, match=f"{op}: num_neg = .* an int >= 1 expected"):
                call(bad)
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError, match="negative_edges: hop = .* an int in \\[0, 2\\^32\\) expected"):
            pg.negative_edges(_fake_graph(), g(ids), 5, hop=bad)
    for name in ("exclude_self", "allow_full"):
        for bad in (0, 1, None, "yes"):
            with pytest.raises(ValueError, match=f"negative_edges: {name} = .* True or False expected"):
                pg.negative_edges(_fake_graph(), g(ids), 5, **{name: bad})
    one = torch.zeros(1, dtype=torch.int64)
    for op, call in (("negative_edges", lambda s: pg.negative_edges(_fake_graph(), g(ids), 5, seed=s)),
                     ("link_batch", lambda s: pg.link_batch(_fake_graph(), g(ids), 5, [10], seed=s))):
        for bad in (one.int(), one.float(), torch.zeros(2, dtype=torch.int64), torch.zeros((), dtype=torch.int64), 7):
            with pytest.raises(ValueError, match=rf"{op}: seed must be an int64 tensor of shape \[1\] on the graph's device cpu"):
                call(bad)
    with pytest.raises(ValueError, match=r"seed must be an int64 tensor of shape \[1\] on the graph's device cuda:0.*on cpu"):
        pg.negative_edges(_fake_graph("cuda:0"), g(ids), 5, seed=one)
    for bad in ([], None, "10", 10):
        with pytest.raises(ValueError, match="link_batch: fanouts: a non-empty list of fanouts"):
            pg.link_batch(_fake_graph(), g(ids), 5, bad)
    for bad in ([0], [10, -1], [2.5], [True]):
        with pytest.raises(ValueError, match="link_batch: fanout = .* an int >= 1, or None for whole rows, expected"):
            pg.link_batch(_fake_graph(), g(ids), 5, bad)
    for bad in ("both", None, 1, "Reverse"):
        with pytest.raises(ValueError, match="link_batch: exclude = .* one of \"none\", \"positive\", \"reverse\" expected"):
            pg.link_batch(_fake_graph(), g(ids), 5, [10], exclude=bad)
    for bad, needle in ((torch.ones(30, dtype=torch.float64), "edge_weight must be float32, not torch.float64"),
                        (torch.ones(29), r"edge_weight \(29,\): one weight per entry of the graph, \[30\], expected"),
                        ([1.0] * 30, "edge_weight must be a float32 tensor \\[graph.nnz\\], not list")):
        with pytest.raises(ValueError, match=f"link_batch: {needle}"):
            pg.link_batch(_fake_graph(), g(ids), 5, [10], edge_weight=bad)
