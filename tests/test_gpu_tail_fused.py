"""The self-loop-only tail's forward folded into the projection (ops.TAIL_FUSED, ABI 15): the projection's epilogue writes the
tail's output instead of Wh, in place of the forward stream (csrc/k12_tail.hip).  The fused runs must compute exactly what the
stream computed: out, dW and da bit for bit."""
import ctypes as C

import pytest
import torch

from tail_case import _iso_csr, _spy

pytestmark = pytest.mark.gpu


def _tail_row_first(graph):
    """First tail row of the degree-ordered pattern the level ran on (None: no tail was found)."""
    tails = [v for k_, v in graph.fwd._alt.items() if isinstance(k_, tuple) and k_[0] == "tail"]
    return tails[0][0] if tails and tails[0] is not None else None


@pytest.mark.parametrize("cfg", [dict(N=20000, Fin=128, iso=0.5, seed=40),     # the headline shape (K = 128: two 16-deep steps a chunk)
                                 dict(N=12345, Fin=64, iso=0.55, seed=41),     # K = 64, an odd row count
                                 dict(N=9001, Fin=128, iso=0.37, seed=42)])
def test_fused_tail_is_bitwise_the_streams_level(cfg, monkeypatch):
    """GATLevelFn with the row map (the level renumbers itself: user_row in the kernels), H 8 x F' 16: TAIL_FUSED on / off."""
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    N, H, Fo, Fin = cfg["N"], 8, 16, cfg["Fin"]
    rowptr, col = _iso_csr(N, cfg["iso"], cfg["seed"])
    g = torch.Generator().manual_seed(cfg["seed"])
    x = torch.randn(N, Fin, generator=g)
    W = torch.randn(H, Fin, Fo, generator=g) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)
    a = torch.randn(H, 2 * Fo, generator=g) * 0.4
    G = torch.randn(N, H * Fo, generator=g)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)          # the a-gradient from the column pass: the tail's Wh rows unread

    def run(fused):
        monkeypatch.setattr(ops, "TAIL_FUSED", fused)
        seen = _spy(monkeypatch)
        graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
        Wd, ad = W.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
        out = pg.GATLevelFn.apply(x.to(dev), Wd, ad, None, graph, 0.2, True)
        out.backward(G.to(dev))
        torch.cuda.synchronize()
        assert graph._ordered is not None
        return out.detach().cpu(), Wd.grad.cpu(), ad.grad.cpu(), seen, _tail_row_first(graph._ordered[0])
    o0, dW0, da0, s0, rf0 = run(False)
    o1, dW1, da1, s1, rf1 = run(True)
    assert rf0 is not None and rf0 == rf1 and N - rf0 >= 0.9 * cfg["iso"] * N
    assert s0 == {"project_tail": 0, "fwd_stream": 1, "bwd_stream": 1}
    assert s1 == {"project_tail": 1, "fwd_stream": 0, "bwd_stream": 1}
    assert torch.equal(o1, o0) and torch.equal(dW1, dW0) and torch.equal(da1, da0)
    assert torch.isfinite(o1).all() and torch.isfinite(dW1).all()


def test_fused_tail_row_first_inside_a_tile(monkeypatch):
    """The first tail row inside a 32-row wave tile of the projection (its epilogue decides per row): first levels on
    InternalOrderView (no row map) for several tail shares, at least one with row_first % 32 != 0."""
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    N, H, Fo, Fin = 16411, 8, 16, 128
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)
    straddled = 0
    for k, iso in enumerate((0.43, 0.51, 0.6)):
        rowptr, col = _iso_csr(N, iso, 50 + k)
        graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
        view = graph.internal_view()
        g = torch.Generator().manual_seed(60 + k)
        x = torch.randn(N, Fin, generator=g).to(dev)[view.to_user.long()].contiguous()
        W = torch.randn(H, Fin, Fo, generator=g) * 0.15
        a = torch.randn(H, 2 * Fo, generator=g) * 0.4
        G = torch.randn(N, H * Fo, generator=g).to(dev)
        res = []
        for fused in (False, True):
            monkeypatch.setattr(ops, "TAIL_FUSED", fused)
            seen = _spy(monkeypatch)
            Wd, ad = W.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
            out = pg.GATLevelFn.apply(x, Wd, ad, None, view, 0.2, True)
            out.backward(G)
            torch.cuda.synchronize()
            assert (seen["project_tail"], seen["fwd_stream"]) == ((1, 0) if fused else (0, 1)), seen
            res.append((out.detach().cpu(), Wd.grad.cpu(), ad.grad.cpu()))
        for p, q in zip(*res):
            assert torch.equal(p, q)
        rf = _tail_row_first(graph.degree_ordered()[0])
        assert rf is not None
        straddled += int(rf % 32 != 0)
    assert straddled >= 1


def test_model_hidden_level_takes_the_forward_half(monkeypatch):
    """pygat_amd.GAT on InternalOrderView: both hidden levels (the second one's input carries a gradient: dx) take the fused
    forward; the model's output and every parameter gradient equal the streams' bit for bit."""
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    N, Fin, C_ = 12000, 64, 5
    rowptr, col = _iso_csr(N, 0.5, 70)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)
    g = torch.Generator().manual_seed(71)
    x = torch.randn(N, Fin, generator=g).to(dev)
    G = torch.randn(N, C_, generator=g).to(dev)
    torch.manual_seed(72)
    model = pg.GAT([Fin, 16, 16, C_], [8, 8, 1], 3, 0.0, 0.2, pg.SpGraphAttentionLayer).to(dev)
    res, seens = [], []
    for fused in (False, True):
        monkeypatch.setattr(ops, "TAIL_FUSED", fused)
        seen = _spy(monkeypatch)
        model.zero_grad(set_to_none=True)
        graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
        y = model(x, graph)
        y.backward(G)
        torch.cuda.synchronize()
        res.append([y.detach().cpu()] + [p.grad.detach().cpu() for p in model.parameters()])
        seens.append(dict(seen))
    assert seens[0] == {"project_tail": 0, "fwd_stream": 2, "bwd_stream": 2}
    assert seens[1] == {"project_tail": 2, "fwd_stream": 0, "bwd_stream": 2}
    for p, q in zip(*res):
        assert torch.equal(p, q)


def test_fused_tail_projection_footprint():
    """The headline projection's tail instantiation as the loaded code object reports it: within the 256 registers of two
    waves per SIMD.  (Its plain instantiation already spills a little: 140 bytes per lane with this compiler.)"""
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    assert lib.pygat_kernel_footprint(b"k1_x3_tail", C.byref(regs), C.byref(scratch)) == 0, lib.pygat_last_error()
    assert 0 < regs.value <= 256 and 0 <= scratch.value <= 256, (regs.value, scratch.value)
