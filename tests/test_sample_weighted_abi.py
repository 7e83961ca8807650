"""pygat_weighted_block, the K22 entry point of the sampler weighted by edge (csrc/k22_sample.hip, additive under ABI 16), refuses bad
arguments on the host before anything is launched: no GPU is needed, and a fake non-null address stands in for every device table
(as in test_sample_abi.py).  Also here, on the CPU: the signatures of pygat_amd.sample_neighbors_weighted / sample_blocks_weighted
and their refusals that need no GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from abi_support import P, call, lib, msg as _msg  # noqa: F401

NAME = "pygat_weighted_block"


def _block(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_dst=8, dst=P, fanout=5, weight=P, seed=P, hop=0, cap=40, src_cap=48, blk_rowptr=P,
             blk_col=P, edge_rc=P, edge_ids=P, src_nodes=P, info=P, ws=P)
    return call(L, "pygat_weighted_block", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    assert NAME in lib.SYMBOLS and hasattr(lib.lib, NAME) and re.search(r"\b" + NAME + r"\(", header)
    fn = lib.lib.pygat_weighted_block
    p, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    assert fn.restype is C.c_int
    assert fn.argtypes == [i, i64, p, p, i, p, i, p, p, u32, i64, i64, p, p, p, p, p, p, p, p]
    # pygat_sample_block's arguments plus the weights, after the fanout
    plain = lib._FUNCS["pygat_sample_block"][1]
    assert lib._FUNCS[NAME][1] == plain[:7] + [("const float*", "weight")] + plain[7:]
    assert [s for s in lib.SYMBOLS if "weighted" in s] == [NAME], "no workspace query of its own: pygat_sample_workspace_bytes serves it"


@pytest.mark.parametrize("kw,needle", [(dict(n=0), "n=0 nodes"), (dict(n=-3), "n=-3 nodes"), (dict(nnz=0), "nnz=0"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(n_dst=0), "n_dst=0"), (dict(n_dst=-1), "n_dst=-1"),
                                       (dict(n_dst=101), "n_dst=101: 1 <= n_dst <= n = 100"), (dict(fanout=0), "fanout=0"),
                                       (dict(fanout=-5), "fanout=-5"), (dict(cap=0), "cap=0"), (dict(cap=1 << 31), "cap=2147483648"),
                                       (dict(src_cap=7), "src_cap=7 is below n_dst=8")])
def test_the_launcher_refuses_the_limits(lib, kw, needle):
    assert _block(lib, **kw) == -1, kw
    assert needle in _msg(lib) and _msg(lib).startswith("weighted_block: "), (kw, _msg(lib))


def test_the_launcher_refuses_its_own_tables(lib):
    for ptr in ("rowptr", "col", "dst", "weight", "seed", "blk_rowptr", "blk_col", "edge_rc", "edge_ids", "src_nodes", "info", "ws"):
        want = f"weighted_block: null {'workspace' if ptr == 'ws' else ptr}"
        assert _block(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    for off in (1, 2, 3):
        assert _block(lib, weight=P + off) == -1 and _msg(lib) == "weighted_block: weight must be 4-byte aligned"
    for off in (4, 8):
        assert _block(lib, ws=P + off) == -1 and _msg(lib) == "weighted_block: the workspace must be 16-byte aligned"
    assert _block(lib, seed=P + 4) == -1 and _msg(lib) == "weighted_block: seed must be 8-byte aligned"
    for ptr in ("dst", "edge_ids", "src_nodes"):
        assert _block(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "weighted_block: dst, edge_ids and src_nodes must be 8-byte aligned"
    assert _block(lib, fanout=2 ** 31 - 1, weight=P + 4, ws=None) == -1 and _msg(lib) == "weighted_block: null workspace"
    fn = lib.lib.pygat_weighted_block
    args = [0 if t in (C.c_int, C.c_int64, C.c_uint32) else None for t in fn.argtypes]
    assert fn(*args) < 0 and _msg(lib).startswith("weighted_block: ")


def _fake_graph(device="cpu"):
    """A CSRGraph that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    g = object.__new__(pg.CSRGraph)
    g.device, g.n, g.nnz = torch.device(device), 10, 30
    return g


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    for name in ("sample_neighbors_weighted", "sample_blocks_weighted"):
        assert name in pg.__all__ and getattr(pg, name).__module__ == "pygat_amd.sampling"
    sig = inspect.signature(pg.sample_neighbors_weighted)
    assert list(sig.parameters) == ["graph", "dst", "fanout", "edge_weight", "seed", "generator", "hop"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator", "hop"))
    assert sig.parameters["edge_weight"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert sig.parameters["hop"].default == 0 and sig.parameters["seed"].default is None
    sig = inspect.signature(pg.sample_blocks_weighted)
    assert list(sig.parameters) == ["graph", "seeds", "fanouts", "edge_weight", "seed", "generator"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator"))
    doc = " ".join(pg.sample_neighbors_weighted.__doc__.split())
    assert "ONE host read" in doc and "stream capture" in doc and "no CPU path" in doc and "NOT checked" in doc

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    dst, w = torch.arange(4), torch.ones(30)
    one = torch.zeros(1, dtype=torch.int64)
    # what the unweighted functions refuse is refused here, by the same code, under the new names
    with pytest.raises(ValueError, match="sample_neighbors_weighted: a CSRGraph expected, not tuple"):
        pg.sample_neighbors_weighted((dst, dst), g(dst), 3, w)
    with pytest.raises(ValueError, match="sample_blocks_weighted: a CSRGraph expected"):
        pg.sample_blocks_weighted(None, g(dst), [3], w)
    with pytest.raises(ValueError, match="sample_neighbors_weighted: dst must be a tensor on the GPU"):
        pg.sample_neighbors_weighted(_fake_graph(), dst, 3, w)
    with pytest.raises(ValueError, match="sample_neighbors_weighted: fanout = 0"):
        pg.sample_neighbors_weighted(_fake_graph(), g(dst), 0, w)
    with pytest.raises(ValueError, match="sample_blocks_weighted: fanout = 0"):
        pg.sample_blocks_weighted(_fake_graph(), g(dst), [5, 0], w)
    with pytest.raises(ValueError, match="sample_blocks_weighted: fanouts: a non-empty list"):
        pg.sample_blocks_weighted(_fake_graph(), g(dst), [], w)
    with pytest.raises(ValueError, match="sample_neighbors_weighted: hop = -1"):
        pg.sample_neighbors_weighted(_fake_graph(), g(dst), 3, w, hop=-1)
    with pytest.raises(ValueError, match="sample_neighbors_weighted: seed must be an int64 tensor"):
        pg.sample_neighbors_weighted(_fake_graph(), g(dst), 3, w, seed=one.int())
    # the weights: type, dtype, shape, layout (the device: tests/test_gpu_sample_weighted.py) -- each before any device work (the
    # graph is a fake and dst lives on the CPU)
    for fn, args, op in ((pg.sample_neighbors_weighted, (g(dst), 3), "sample_neighbors_weighted"),
                         (pg.sample_blocks_weighted, (g(dst), [3, 2]), "sample_blocks_weighted")):
        for bad in (None, [1.0] * 30, 1.0):
            with pytest.raises(ValueError, match=f"{op}: edge_weight must be a float32 tensor \\[graph.nnz\\], not "):
                fn(_fake_graph(), *args, bad, seed=one)
        for bad in (w.double(), w.half(), w.bfloat16(), w.long()):
            with pytest.raises(ValueError, match=f"{op}: edge_weight must be float32, not torch"):
                fn(_fake_graph(), *args, bad, seed=one)
        for bad in (torch.ones(29), torch.ones(31), torch.ones(30, 1), torch.ones(())):
            with pytest.raises(ValueError, match=f"{op}: edge_weight .* one weight per entry of the graph, \\[30\\], expected"):
                fn(_fake_graph(), *args, bad, seed=one)
        with pytest.raises(ValueError, match=f"{op}: edge_weight must be contiguous"):
            fn(_fake_graph(), *args, torch.ones(60)[::2], seed=one)
    with pytest.raises(ValueError, match="dst holds 11 ids but the graph has 10 nodes"):
        pg.sample_neighbors_weighted(_fake_graph(), g(torch.arange(11)), 3, w, seed=one)
