"""The screening fix-up kernels: the path a C caller gets whose pygat_graph carries no cut-row list (cut_rows == NULL).

The package always builds a list (graph._Pattern._make), so the kernels that find the cut rows themselves -- a wave or work-group
screens FIX_SCREEN slots for the rows they own (csrc/attn_common.h, screen_cut_rows) and merges them in turn -- are reached here
by handing the entry points a copy of the graph struct with the list taken out: cut_rows = NULL, n_cut = n_cut_wide = 0,
slot_begin and slot_meta kept.  The ladder graph at 4-edge slots has cut chains of 2 ... 40+ pieces, so both the one-wave merge
and the work-group merge through LDS run.
No new tolerance: the fp32 level is priced by tests/parity.py's rule as tests/test_gpu_parity.py applies it, the bf16 table by
tests/test_gpu_bf16_table.py's comparison."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity
from bf16_table_case import case, reference
from ladder_case import _ladder_graph
from test_gpu_bf16_table import BF16, FIN, _graph, _run
from test_gpu_parity import check, params, run_level

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import pygat_amd
    return pygat_amd


def _without_list(monkeypatch):
    """From here on every pygat_graph the package hands out is a copy without its cut-row list; -> the copies handed out."""
    from pygat_amd import _lib, graph
    real, handed = graph._Pattern._make, []

    def make(self, slot_edges, snapped):
        st = _lib.Graph()
        C.memmove(C.byref(st), C.byref(real(self, slot_edges, snapped)), C.sizeof(_lib.Graph))
        st.cut_rows, st.n_cut, st.n_cut_wide = None, 0, 0
        handed.append(st)
        return st
    monkeypatch.setattr(graph._Pattern, "_make", make)
    return handed


def _all_screened(handed):
    assert handed, "the level asked for no graph struct: the patch was not in its way"
    for st in handed:
        assert st.cut_rows is None and st.n_cut == 0 and st.n_cut_wide == 0, "a graph with a cut-row list reached the level"
        assert st.slot_begin and st.slot_meta, "slot borders and slot records stay"


@pytest.mark.parametrize("H,Fo", [(1, 16), (8, 16), (8, 64)])   # 4 and 32 lanes per row at one chunk per lane; two chunks per lane
def test_fp32_level_without_a_cut_row_list(pg, monkeypatch, H, Fo):
    """K2's and K4's screening kernels: forward, dX, dW and da against the fp64 oracle, and against the list-driven run.
    The two runs differ in summation order only (the list's packed entries deal a row's pieces to fewer lane groups), every
    logit and so every LeakyReLU branch is the same: their distance is priced per tensor by the rule's own bound for this
    input, max(1e-5, 4 x the fp32 oracle's error)."""
    rowptr, col = _ladder_graph()
    N, Fin, slot = len(rowptr) - 1, 32, 4
    # a chain goes to the whole work-group (through LDS) beyond 64 / LPR x PF pieces: 8 at 8 x 16, 2 at 8 x 64 -- both kinds of merge
    # run there; one head of 16 (16 lane groups, 64 pieces in a round) merges every chain of this graph in one wave
    assert np.diff(rowptr).max() // slot > 32 and (np.diff(rowptr) // slot == 1).any()
    W, a, _ = params(H, Fin, Fo, False, 11)
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(N, Fin, dtype=torch.float64, generator=gen)
    G = torch.randn(N, H * Fo, dtype=torch.float64, generator=gen)
    listed = run_level(pg, x, rowptr, col, W, a, None, True, G, slot=slot)
    with monkeypatch.context() as mp:
        handed = _without_list(mp)
        screened = run_level(pg, x, rowptr, col, W, a, None, True, G, slot=slot)
    _all_screened(handed)
    rep = check(screened, x, rowptr, col, W, a, None, True, G, f"no cut-row list, {H}x{Fo}, {slot}-edge slots")
    own = dict(rep["fp32"], out=parity.err(rep["ref32"]["out"], rep["ref64"]["out"]))
    for name, got, ref in zip(("out", "dX", "dW", "da"), screened, listed):
        d, tol = parity.err(got, ref), max(parity.ATOL, 4.0 * own[name])
        print(f"{H}x{Fo} {name}: screening vs list {d:.2e} (bound {tol:.2e})")
        assert d <= tol, f"{H}x{Fo} {name}: screening and list-driven fix-up differ by {d:.3e} > {tol:.3e}"


@pytest.mark.parametrize("H,Fo", [(8, 16), (2, 4)])   # chunks of 8 and of 4 table elements
def test_bf16_table_without_a_cut_row_list(pg, monkeypatch, H, Fo):
    """K16's fix-up, a wave per FIX_SCREEN slots.  Its list-driven form gives a cut row to one wave as well and merges it by the
    same function with the same arguments, so the two runs are equal bit for bit."""
    rowptr, col = _ladder_graph()
    x, W, a, _ = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=100 * H + Fo)
    o64, o32 = reference(x, rowptr, col, W, a, None, True)
    listed = _run(_graph(rowptr, col, 4), x, W, a, None, True, table_dtype=BF16)
    with monkeypatch.context() as mp:
        handed = _without_list(mp)
        screened = _run(_graph(rowptr, col, 4), x, W, a, None, True, table_dtype=BF16)
    _all_screened(handed)
    e = parity.close_fwd(screened, o64, f"bf16 {H}x{Fo}, no cut-row list", o32)
    print(f"bf16 {H}x{Fo}, no cut-row list: err {e:.2e} (fp32 run {parity.err(o32, o64):.2e})")
    assert torch.equal(screened, listed)
