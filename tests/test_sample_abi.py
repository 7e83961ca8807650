"""The K22 entry points (csrc/k22_sample.hip, additive under ABI 16) refuse bad arguments on the host, before anything is launched:
no GPU is needed, and a fake non-null address stands in for every device table (as in test_gatv2_attention_edge_abi.py).  Also here,
on the CPU: the signature of pygat_amd.sample_neighbors / sample_blocks and their refusals that need no GPU."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from abi_support import P, call, lib, msg as _msg  # noqa: F401

NEW = ("pygat_sample_workspace_bytes", "pygat_sample_block")


def _block(L, **kw):
    a = dict(n=100, nnz=500, rowptr=P, col=P, n_dst=8, dst=P, fanout=5, seed=P, hop=0, cap=40, src_cap=48, blk_rowptr=P, blk_col=P,
             edge_rc=P, edge_ids=P, src_nodes=P, info=P, ws=P)
    return call(L, "pygat_sample_block", a, **kw)


def test_additive_under_abi_16(lib):
    assert lib.ABI_VERSION == 16 and lib.lib.pygat_abi_version() == 16
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "pygat_amd.h")).read()
    assert "#define PYGAT_ABI_VERSION 16" in header
    for s in NEW:
        assert s in lib.SYMBOLS and hasattr(lib.lib, s)
        assert re.search(r"\b" + s + r"\(", header), s
        assert getattr(lib.lib, s).restype is C.c_int
    p, i, i64, u32 = C.c_void_p, C.c_int, C.c_int64, C.c_uint32
    assert lib.lib.pygat_sample_workspace_bytes.argtypes == [i, i, C.POINTER(C.c_size_t)]
    assert lib.lib.pygat_sample_block.argtypes == [i, i64, p, p, i, p, i, p, u32, i64, i64, p, p, p, p, p, p, p, p]
    assert [s for s in lib.SYMBOLS if "sample" in s] == list(NEW)


def test_the_workspace_query(lib):
    n = C.c_size_t(0)
    L = lib.lib
    assert L.pygat_sample_workspace_bytes(1000, 10, None) == -1 and _msg(lib) == "sample_workspace_bytes: null bytes"
    for bad in ((0, 1), (10, 0), (10, 11), (-1, 1), (10, -1)):
        assert L.pygat_sample_workspace_bytes(*bad, C.byref(n)) == -1 and _msg(lib).startswith("sample_workspace_bytes: n="), bad
    assert L.pygat_sample_workspace_bytes(1000, 10, C.byref(n)) == 0
    small = n.value
    # two n-sized tables, their scan, four n_dst-sized lists and the scan's tiles, each rounded up to 16 bytes
    assert small >= 4 * (3 * 1000 + 1 + 4 * 10 + 1) and small % 16 == 0 and small < 4 * (3 * 1000 + 4 * 10) + 256
    assert L.pygat_sample_workspace_bytes(1 << 20, 1 << 20, C.byref(n)) == 0 and n.value >= 4 * 7 * (1 << 20)
    assert lib._workspace_bytes("sample_workspace_bytes", 1000, 10) == small


@pytest.mark.parametrize("kw,needle", [(dict(n=0), "n=0 nodes"), (dict(n=-3), "n=-3 nodes"), (dict(nnz=0), "nnz=0"),
                                       (dict(nnz=1 << 31), "2^31"), (dict(n_dst=0), "n_dst=0"), (dict(n_dst=-1), "n_dst=-1"),
                                       (dict(n_dst=101), "n_dst=101: 1 <= n_dst <= n = 100"), (dict(fanout=0), "fanout=0"),
                                       (dict(fanout=-5), "fanout=-5"), (dict(cap=0), "cap=0"), (dict(cap=1 << 31), "cap=2147483648"),
                                       (dict(src_cap=7), "src_cap=7 is below n_dst=8")])
def test_the_launcher_refuses_the_limits(lib, kw, needle):
    assert _block(lib, **kw) == -1, kw
    assert needle in _msg(lib) and _msg(lib).startswith("sample_block: "), (kw, _msg(lib))


def test_the_launcher_refuses_its_own_tables(lib):
    for ptr in ("rowptr", "col", "dst", "seed", "blk_rowptr", "blk_col", "edge_rc", "edge_ids", "src_nodes", "info", "ws"):
        want = f"sample_block: null {'workspace' if ptr == 'ws' else ptr}"
        assert _block(lib, **{ptr: None}) == -1 and _msg(lib) == want, (ptr, _msg(lib))
    for off in (4, 8):
        assert _block(lib, ws=P + off) == -1 and _msg(lib) == "sample_block: the workspace must be 16-byte aligned"
    assert _block(lib, seed=P + 4) == -1 and _msg(lib) == "sample_block: seed must be 8-byte aligned"
    for ptr in ("dst", "edge_ids", "src_nodes"):
        assert _block(lib, **{ptr: P + 4}) == -1 and _msg(lib) == "sample_block: dst, edge_ids and src_nodes must be 8-byte aligned"
    assert _block(lib, fanout=2 ** 31 - 1, ws=None) == -1 and _msg(lib) == "sample_block: null workspace", "INT32_MAX: whole rows"


def test_with_every_pointer_null(lib):
    for name in NEW:
        fn = getattr(lib.lib, name)
        args = [0 if t in (C.c_int, C.c_int64, C.c_uint32) else None for t in fn.argtypes]
        assert fn(*args) < 0 and _msg(lib).startswith(name[len("pygat_"):] + ": ")


def test_the_footprint_names(lib):
    regs, scratch = C.c_int(0), C.c_int(0)
    assert lib.lib.pygat_kernel_footprint(b"k22_nothing", C.byref(regs), C.byref(scratch)) == -1
    assert "k22_select_wave, k22_select_block" in _msg(lib)


def _fake_graph(device="cpu"):
    """A CSRGraph that was never built: enough for the refusals made before any of its tables is touched."""
    import pygat_amd as pg
    g = object.__new__(pg.CSRGraph)
    g.device, g.n, g.nnz = torch.device(device), 10, 30
    return g


def test_python_signature_and_refusals_that_need_no_gpu():
    import pygat_amd as pg
    for name in ("sample_neighbors", "sample_blocks", "SampledBlock"):
        assert name in pg.__all__ and getattr(pg, name).__module__ == "pygat_amd.sampling"
    sig = inspect.signature(pg.sample_neighbors)
    assert list(sig.parameters) == ["graph", "dst", "fanout", "seed", "generator", "hop"]
    assert all(sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("seed", "generator", "hop"))
    assert sig.parameters["hop"].default == 0 and sig.parameters["seed"].default is None
    assert list(inspect.signature(pg.sample_blocks).parameters) == ["graph", "seeds", "fanouts", "seed", "generator"]
    assert pg.SampledBlock._fields == ("pattern", "src_nodes", "dst_nodes", "edge_ids", "n_dst", "n_src", "nnz")
    doc = " ".join(pg.sample_neighbors.__doc__.split())
    assert "ONE host read" in doc and "stream capture" in doc and "no CPU path" in doc

    class OnGpu(torch.Tensor):
        is_cuda = property(lambda self: True)
    g = lambda t: t.as_subclass(OnGpu)  # noqa: E731
    dst = torch.arange(4)
    with pytest.raises(ValueError, match="sample_neighbors: a CSRGraph expected, not tuple"):
        pg.sample_neighbors((dst, dst), g(dst), 3)
    with pytest.raises(ValueError, match="sample_blocks: a CSRGraph expected"):
        pg.sample_blocks(None, g(dst), [3])
    for bad in (dst, [0, 1], None):
        with pytest.raises(ValueError, match="sample_neighbors: dst must be a tensor on the GPU"):
            pg.sample_neighbors(_fake_graph(), bad, 3)
    for bad in (dst.float(), dst.double(), dst.bool(), dst.to(torch.int16)):
        with pytest.raises(ValueError, match="sample_neighbors: dst must be int32 or int64, not torch"):
            pg.sample_neighbors(_fake_graph(), g(bad), 3)
    for bad in (dst.view(2, 2), dst[:0]):
        with pytest.raises(ValueError, match=r"sample_neighbors: dst \[n_dst\] with n_dst >= 1 expected"):
            pg.sample_neighbors(_fake_graph(), g(bad), 3)
    with pytest.raises(ValueError, match="sample_neighbors: dst lives on cpu, the graph on cuda:1"):
        pg.sample_neighbors(_fake_graph("cuda:1"), g(dst), 3)
    for bad in (0, -1, 2.0, True, "3", 2 ** 31):
        with pytest.raises(ValueError, match="sample_neighbors: fanout = .* an int >= 1, or None for whole rows, expected"):
            pg.sample_neighbors(_fake_graph(), g(dst), bad)
    with pytest.raises(ValueError, match="sample_blocks: fanout = 0"):
        pg.sample_blocks(_fake_graph(), g(dst), [5, 0])
    for bad in ([], None, 5):
        with pytest.raises(ValueError, match="sample_blocks: fanouts: a non-empty list"):
            pg.sample_blocks(_fake_graph(), g(dst), bad)
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError, match="sample_neighbors: hop = .* an int in \\[0, 2\\^32\\) expected"):
            pg.sample_neighbors(_fake_graph(), g(dst), 3, hop=bad)
    one = torch.zeros(1, dtype=torch.int64)
    for bad in (one.int(), one.float(), torch.zeros(2, dtype=torch.int64), torch.zeros((), dtype=torch.int64), 7):       # dtype, shape
        with pytest.raises(ValueError, match=r"sample_neighbors: seed must be an int64 tensor of shape \[1\] on the graph's device cpu"):
            pg.sample_neighbors(_fake_graph(), g(dst), 3, seed=bad)
    with pytest.raises(ValueError, match=r"seed must be an int64 tensor of shape \[1\] on the graph's device cuda:0.*on cpu"):      # device
        pg.sample_neighbors(_fake_graph("cuda:0"), g(dst), 3, seed=one)
    with pytest.raises(ValueError, match="sample_blocks: seed must be an int64 tensor"):
        pg.sample_blocks(_fake_graph(), g(dst), [3], seed=one.int())
    # more ids than nodes: a repeat for certain, refused before anything is allocated
    with pytest.raises(ValueError, match="dst holds 11 ids but the graph has 10 nodes"):
        pg.sample_neighbors(_fake_graph(), g(torch.arange(11)), 3, seed=one)
