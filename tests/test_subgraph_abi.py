"""The K23 entry points (csrc/k23_subgraph.hip, additive under ABI 16) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table (as in test_sample_abi.py).  Also here, on the CPU:
the signatures of pygat_amd.induced_subgraph / random_walk and their refusals that need no GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from abi_support import P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_subgraph_workspace_bytes", "pygat_subgraph_count", "pygat_subgraph_fill", "pygat_random_walk")


def _count(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_in=8, nodes=P, sub_nodes=P, index=P, sub_rowptr=P, info=P, ws=P)
    return call(L, "pygat_subgraph_count", a, **kw)


def _fill(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_in=8, n_sub=6, sub_nnz=20, sub_nodes=P, sub_rowptr=P, sub_col=P, edge_rc=P, edge_ids=P, ws=P)
    return call(L, "pygat_subgraph_fill", a, **kw)


def _walk(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_walk=8, start=P, length=4, seed=P, hop=0, walks=P, info=P)
    return call(L, "pygat_random_walk", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    assert lib.lib.pygat_subgraph_workspace_bytes.argtypes == [i, i64, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_subgraph_count.argtypes == [i, i64, p, p, i64, p, p, p, p, p, p, p]
    assert lib.lib.pygat_subgraph_fill.argtypes == [i, i64, p, p, i64, i, i64, p, p, p, p, p, p, p]
    assert lib.lib.pygat_random_walk.argtypes == [i, i64, p, p, i64, p, i, p, u32, p, p, p]
    assert [s for s in lib.SYMBOLS if "subgraph" in s or "walk" in s] == list(NEW)


def test_the_workspace_query(lib):
    n = C.c_size_t(0)
    L = lib.lib
    assert L.pygat_subgraph_workspace_bytes(1000, 10, None) == -1 and _msg(lib) == "subgraph_workspace_bytes: null bytes"
    for bad in ((0, 1), (10, 0), (-1, 1), (10, -1), (10, 1 << 31)):
        assert L.pygat_subgraph_workspace_bytes(*bad, C.byref(n)) == -1 and _msg(lib).startswith("subgraph_workspace_bytes: n="), bad
    assert L.pygat_subgraph_workspace_bytes(1000, 10, C.byref(n)) == 0
    small = n.value
    # an n-sized table and its scan, four lists of min(n_in, n) rows, 1024 partial counts and the scan's tiles
    assert small >= 4 * (2 * 1000 + 1 + 4 * 10 + 1 + 1024) and small % 16 == 0 and small < 4 * (2 * 1000 + 4 * 10 + 1024) + 256
    assert L.pygat_subgraph_workspace_bytes(1000, 5000, C.byref(n)) == 0, "more ids than nodes: repeats"
    assert 4 * (6 * 1000 + 1024) <= n.value < 4 * (6 * 1000 + 1024) + 256, "the rows are bounded by min(n_in, n)"
    assert lib._workspace_bytes("subgraph_workspace_bytes", 1000, 10) == small


@pytest.mark.parametrize("call,kw,needle", [
    ("count", dict(n=0), "n=0 nodes"), ("count", dict(n_in=0), "n_in=0 ids"), ("count", dict(n_in=1 << 31), "n_in=2147483648"),
    ("count", dict(nnz=0), "nnz=0"), ("count", dict(nnz=1 << 31), "2^31"),
    ("fill", dict(n=-2), "n=-2 nodes"), ("fill", dict(n_in=-1), "n_in=-1 ids"), ("fill", dict(nnz=0), "nnz=0"),
    ("fill", dict(n_sub=0), "n_sub=0 rows"), ("fill", dict(n_sub=9), "n_sub=9 rows: 1 <= n_sub <= min(n_in, n) = 8"),
    ("fill", dict(n_in=500, n_sub=101), "min(n_in, n) = 100"), ("fill", dict(sub_nnz=0), "sub_nnz=0 entries"),
    ("fill", dict(sub_nnz=501), "sub_nnz=501 entries: 1 <= sub_nnz <= nnz = 500"),
    ("walk", dict(n=0), "n=0 nodes"), ("walk", dict(nnz=0), "nnz=0"), ("walk", dict(n_walk=0), "n_walk=0"),
    ("walk", dict(n_walk=1 << 31), "n_walk=2147483648"), ("walk", dict(length=0), "length=0"), ("walk", dict(length=-4), "length=-4")])
def test_the_launchers_refuse_the_limits(lib, call, kw, needle):
    fn, prefix = {"count": (_count, "subgraph_count: "), "fill": (_fill, "subgraph_fill: "), "walk": (_walk, "random_walk: ")}[call]
    assert fn(lib, **kw) == -1, kw
    assert needle in _msg(lib) and _msg(lib).startswith(prefix), (kw, _msg(lib))


def test_the_launchers_refuse_their_own_tables(lib):
    for ptr in ("rowptr", "col", "nodes", "sub_nodes", "index", "sub_rowptr", "info", "ws"):
        want = f"subgraph_count: null {'workspace' if ptr == 'ws' else ptr}"
        assert _count(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    for ptr in ("rowptr", "col", "sub_nodes", "sub_rowptr", "sub_col", "edge_rc", "edge_ids", "ws"):
        want = f"subgraph_fill: null {'workspace' if ptr == 'ws' else ptr}"
        assert _fill(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    for ptr in ("rowptr", "col", "start", "seed", "walks", "info"):
        assert _walk(lib, **{ptr: None}) == -1 and _msg(lib) == f"random_walk: null {ptr}", (ptr, _msg(lib))
    for off in (4, 8):
        assert _count(lib, ws=P + off) == -1 and _msg(lib) == "subgraph_count: the workspace must be 16-byte aligned"
        assert _fill(lib, ws=P + off) == -1 and _msg(lib) == "subgraph_fill: the workspace must be 16-byte aligned"
    for ptr in ("nodes", "sub_nodes", "index"):
        assert _count(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "subgraph_count: nodes, sub_nodes and index must be 8-byte aligned"
    for ptr in ("sub_nodes", "edge_rc", "edge_ids"):
        assert _fill(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "subgraph_fill: sub_nodes, edge_rc and edge_ids must be 8-byte aligned"
    assert _walk(lib, seed=P + 4) == -1 and _msg(lib) == "random_walk: seed must be 8-byte aligned"
    for ptr in ("start", "walks"):
        assert _walk(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "random_walk: start and walks must be 8-byte aligned"


def test_with_every_pointer_null(lib):
    for name in NEW:
        fn = getattr(lib.lib, name)
        args = [0 if t in (C.c_int, C.c_int64, C.c_uint32) else None for t in fn.argtypes]
        assert fn(*args) < 0 and _msg(lib).startswith(name[len("pygat_"):] + ": ")


def test_the_footprint_names(lib):
    regs, scratch = C.c_int(0), C.c_int(0)
    assert lib.lib.pygat_kernel_footprint(b"k23_nothing", C.byref(regs), C.byref(scratch)) == -1
    assert "k23_count_rows, k23_list, k23_count_long" in _msg(lib) and "k23_fill_rows, k23_fill_long, k23_walk" in _msg(lib)


def _fake_graph(device="cpu"):
    """A CSRGraph that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    g = object.__new__(pg.CSRGraph)
    g.device, g.n, g.nnz = torch.device(device), 10, 30
    return g


def test_python_signatures_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    for name in ("induced_subgraph", "random_walk", "InducedSubgraph"):
        assert name in pg.__all__ and getattr(pg, name).__module__ == "pygat_amd.subgraph"
    assert list(inspect.signature(pg.induced_subgraph).parameters) == ["graph", "nodes"]
    assert list(inspect.signature(pg.CSRGraph.subgraph).parameters) == ["self", "nodes"]
    sig = inspect.signature(pg.random_walk)
    assert list(sig.parameters) == ["graph", "start", "length", "seed", "generator", "hop"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator", "hop"))
    assert sig.parameters["hop"].default == 0 and sig.parameters["seed"].default is None
    assert pg.InducedSubgraph._fields == ("nodes", "index", "edge_ids", "rowptr", "col", "edge_rc", "n", "nnz", "n_empty_rows")
    assert isinstance(pg.InducedSubgraph.pattern, property) and isinstance(pg.InducedSubgraph.graph, property)
    for fn in (pg.induced_subgraph, pg.random_walk):
        doc = " ".join(fn.__doc__.split())
        assert "ONE host read" in doc and "stream capture" in doc and "no CPU path" in doc

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    ids = torch.arange(4)
    calls = (("induced_subgraph", "nodes", "n_in", lambda graph, t: pg.induced_subgraph(graph, t)),
             ("induced_subgraph", "nodes", "n_in", lambda graph, t: pg.CSRGraph.subgraph(graph, t)),
             ("random_walk", "start", "n_walk", lambda graph, t: pg.random_walk(graph, t, 4)))
    for op, name, size, call in calls:
        if call is not calls[1][3]:
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
        with pytest.raises(ValueError, match=f"{op}: {name} lives on cpu, the graph on cuda:1"):
            call(_fake_graph("cuda:1"), g(ids))
    for bad in (0, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="random_walk: length = .* an int >= 1 expected"):
            pg.random_walk(_fake_graph(), g(ids), bad)
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError, match="random_walk: hop = .* an int in \\[0, 2\\^32\\) expected"):
            pg.random_walk(_fake_graph(), g(ids), 4, hop=bad)
    one = torch.zeros(1, dtype=torch.int64)
    for bad in (one.int(), one.float(), torch.zeros(2, dtype=torch.int64), torch.zeros((), dtype=torch.int64), 7):
        with pytest.raises(ValueError, match=r"random_walk: seed must be an int64 tensor of shape \[1\] on the graph's device cpu"):
            pg.random_walk(_fake_graph(), g(ids), 4, seed=bad)
    with pytest.raises(ValueError, match=r"seed must be an int64 tensor of shape \[1\] on the graph's device cuda:0.*on cpu"):
        pg.random_walk(_fake_graph("cuda:0"), g(ids), 4, seed=one)
