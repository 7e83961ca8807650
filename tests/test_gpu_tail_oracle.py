"""The internal node order and the self-loop-only tail's routes (CSRGraph.degree_ordered, ops.TAIL, ops.TAIL_FUSED) against the
fp64 oracle -- the routes a large graph takes by default:
  A. the projection with the tail in its epilogue (pygat_project_tail_blocked), called directly: prefix rows bitwise the plain
     projection's, tail rows bitwise the tail stream's, both within a K-scaled fp32 bound of fp64, nothing else written;
  B. whole levels on the tail routes (row map, InternalOrderView, no_grad; fused, streamed, C-side fallback) by the parity rule;
  C. a degree-ordered graph handed to a level directly: `out` at the caller's rows, gradients as for the caller's graph;
  D. degenerate tails: every row self-loop-only, a single non-tail edge pair, a tail too short for a slot of its own."""
import numpy as np
import pytest
import torch

import parity
from tail_case import _iso_csr, _spy

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = 0x7FC0DEAD          # a NaN bit pattern no kernel writes


def _sent(*shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda:0").view(torch.float32)


def _bits(t):
    return t.view(torch.int32)


def _dev(*ts):
    return [None if t is None else t.float().to("cuda:0") for t in ts]


# ----------------------------------------------------------------------------------------------------------------------------
# A. pygat_project_tail_blocked against fp64
# (n, Fin, H, F', admitted by try_project_x3_tail): sr_fp = F'; spc 1 / 2 = Fin 64 / 128; NT = min(R / 32, 4) column tiles
A_CASES = [
    (8192, 128, 8, 16, True),     # sr_fp 16, spc 2, NT 4 (R 128, the headline tile), n a multiple of 256
    (10000, 64, 8, 8, True),      # sr_fp 8, spc 1, NT 2 (R 64: the reference's 8 heads x 8)
    (9001, 128, 4, 16, True),     # sr_fp 16, spc 2, NT 2 (R 64)
    (8448, 64, 16, 16, True),     # sr_fp 16, spc 1, NT 4 x 2 column blocks (R 256), n a multiple of 256
    (8300, 128, 32, 16, True),    # sr_fp 16, spc 2, NT 4 x 4 (R 512)
    (8200, 128, 16, 8, True),     # sr_fp 8, spc 2, NT 4 (R 128)
    (8960, 64, 32, 8, True),      # sr_fp 8, spc 1, NT 4 x 2 (R 256)
    (9000, 96, 8, 16, False),     # Fin 96: the plain projection + the tail stream
    (4000, 128, 8, 16, False),    # n < 8192
    (9000, 64, 2, 16, False),     # R = 32 (one column tile)
]


def _row_firsts(n):
    last = ((n - 1) // 256) * 256                  # first row of the last (possibly partial) 256-row tile
    return sorted({0, 1, 45, n // 2 + 3, last + min(37, (n - last) // 2), n - 1})


@pytest.mark.parametrize("case", A_CASES, ids=lambda c: "n{}-fin{}-h{}x{}".format(*c[:4]))
def test_project_tail_against_fp64(case):
    from pygat_amd import _lib
    from pygat_amd._lib import lib, check, padded_width
    n, Fin, H, Fo, fused = case
    Fp = padded_width(Fo)
    assert Fo == Fp
    R = H * Fp
    g = torch.Generator().manual_seed(n + Fin + H)
    x = torch.randn(n, Fin, generator=g).float()
    W = (torch.randn(H, Fin, Fo, generator=g) * (2.0 / (Fin + Fo)) ** 0.5).float()
    a = (torch.randn(H, 2 * Fo, generator=g) * 0.5).float()
    # fp64 reference, once per shape: Wh = x W, s = Wh . a_src, ELU(Wh), and the bounds' magnitudes |x| |W|
    x64, W64, a64 = x.double(), W.double(), a.double()
    Wh64 = torch.einsum("nk,hkf->nhf", x64, W64)
    B = torch.einsum("nk,hkf->nhf", x64.abs(), W64.abs())
    s64 = (Wh64 * a64[None, :, :Fo]).sum(-1)
    Bs = (B * a64[None, :, :Fo].abs()).sum(-1)
    Wh64, B = Wh64.reshape(n, R).cuda(), B.reshape(n, R).cuda()
    s64, Bs = s64.cuda(), Bs.cuda()
    elu64 = torch.where(Wh64 > 0, Wh64, torch.expm1(Wh64.clamp(max=0)))
    tol_wh = 4 * Fin * U * B
    tol_s = 4 * (Fin + Fo) * U * Bs
    tol_out = tol_wh + 8 * U * (1 + elu64.abs())

    xd, Wd, ad = _dev(x, W, a)
    st = torch.cuda.current_stream().cuda_stream
    mode = 0                                                            # split-bf16 (ops.GEMM_MODES)
    ldw = -(-(R + 2 * H) // 4) * 4                                      # as ops._Level, no skip projection
    Wcat = torch.empty(Fin, ldw, dtype=torch.float32, device="cuda:0")
    a_pad = torch.empty(H, 2, Fp, dtype=torch.float32, device="cuda:0")
    check(lib.pygat_pack_params(H, Fin, Fo, Wd.data_ptr(), ad.data_ptr(), None, Wcat.data_ptr(), ldw, a_pad.data_ptr(), st), "pack")
    Wh0, s0 = _sent(n, R), _sent(n, H)
    check(lib.pygat_project_blocked(n, Fin, H, Fo, xd.data_ptr(), Fin, None, Wcat.data_ptr(), ldw, a_pad.data_ptr(), Wh0.data_ptr(),
                                    None, s0.data_ptr(), 1, None, mode, st), "project")
    torch.cuda.synchronize()
    e = (Wh0.double() - Wh64).abs()
    assert bool((e <= tol_wh).all()), f"plain Wh: max err {float(e.max()):.3e}, worst err / bound {float((e / tol_wh).max()):.2f}"
    e = (s0.double() - s64).abs()
    assert bool((e <= tol_s).all()), f"plain s: max err {float(e.max()):.3e}, worst err / bound {float((e / tol_s).max()):.2f}"

    perm = torch.randperm(n, generator=g).to(torch.int32).cuda()
    for rf in _row_firsts(n):
        for urow in (None, perm):
            what = f"{case} row_first {rf} {'map' if urow is not None else 'identity'}"
            up = None if urow is None else urow.data_ptr()
            u = torch.arange(n, device="cuda:0") if urow is None else urow.long()
            ref = _sent(n, R)              # what the plain projection + the forward stream write
            check(lib.pygat_gat_forward_tail(rf, n - rf, H, Fo, _lib.F_ELU, Wh0.data_ptr(), 0, None, ref.data_ptr(), up,
                                             None, None, None, st), "forward_tail")
            Wh, s, out = _sent(n, R), _sent(n, H), _sent(n, R)
            check(lib.pygat_project_tail_blocked(n, Fin, H, Fo, xd.data_ptr(), Fin, None, Wcat.data_ptr(), ldw, a_pad.data_ptr(),
                                                 Wh.data_ptr(), s.data_ptr(), 1, None, mode, rf, up, out.data_ptr(), _lib.F_ELU, st),
                  "project_tail")
            torch.cuda.synchronize()
            # prefix rows: the plain projection's Wh and s, bit for bit
            assert torch.equal(_bits(Wh[:rf]), _bits(Wh0[:rf])), f"{what}: prefix Wh differs from pygat_project_blocked"
            assert torch.equal(_bits(s[:rf]), _bits(s0[:rf])), f"{what}: prefix s differs from pygat_project_blocked"
            # tail rows: the stream's output at their user rows, bit for bit, and within bound of fp64 ELU(x W)
            ut = u[rf:]
            assert torch.equal(_bits(out[ut]), _bits(ref[ut])), f"{what}: tail output differs from the forward stream's"
            e = (out[ut].double() - elu64[rf:]).abs()
            assert bool((e <= tol_out[rf:]).all()), f"{what}: tail output max err {float(e.max()):.3e} against fp64 ELU(x W)"
            # nothing but the tail's user rows of `out`
            other = torch.ones(n, dtype=torch.bool, device="cuda:0")
            other[ut] = False
            assert bool((_bits(out[other]) == SENT).all()), f"{what}: rows of `out` outside the tail's user rows written"
            # the fused epilogue ran (the tail's Wh rows untouched), or the fallback projected every row
            untouched = _bits(Wh[rf:]) == SENT
            if fused:
                assert bool(untouched.all()), f"{what}: the tail's Wh rows were written -- the fused projection did not run"
            else:
                assert not bool(untouched.any()), f"{what}: fallback shape, yet Wh rows of the tail were left unwritten"
                assert torch.equal(_bits(Wh), _bits(Wh0))


# ----------------------------------------------------------------------------------------------------------------------------
# B. whole levels on the tail routes against the oracle
def _level_data(N, Fin, H, Fo, seed, iso=0.5):
    rowptr, col = _iso_csr(N, iso, seed)
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randn(N, Fin, generator=g, dtype=torch.float64).float().double()
    W = (torch.randn(H, Fin, Fo, generator=g, dtype=torch.float64) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)).float().double()
    a = (torch.randn(H, 2 * Fo, generator=g, dtype=torch.float64) * 0.4).float().double()
    G = torch.randn(N, H * Fo, generator=g, dtype=torch.float64).float().double()
    return rowptr, col, x, W, a, G


def _force_tail_routes(monkeypatch):
    from pygat_amd import ops
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES_TAIL", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)


def _graph(rowptr, col):
    import pygat_amd as pg
    return pg.CSRGraph(torch.as_tensor(rowptr, device="cuda:0"), torch.as_tensor(col, device="cuda:0"))


def _heads_params(W, a):
    Wd, ad = _dev(W, a)
    Ws = [Wd[h].clone().requires_grad_(True) for h in range(W.shape[0])]
    As = [ad[h].reshape(1, -1).clone().requires_grad_(True) for h in range(W.shape[0])]
    return Ws, As


# (Fin, H, F') -> expected forward route in training and in inference: "fused" (project_tail, no forward stream), "stream" (the
# forward stream), "c_fallback" (the fused entry point is called, its C side falls back to projection + stream).  A training
# level fuses only where the column pass folds the a-gradient (pygat_gat_backward_col_da_bytes > 0: 8 heads x 16 here);
# elsewhere the a-gradient pass reads the tail's Wh rows, so the projection has to write them.
B_CASES = [((128, 8, 8), "stream", "fused"), ((64, 16, 8), "stream", "fused"), ((64, 4, 16), "stream", "fused"),
           ((128, 8, 16), "fused", "fused"), ((128, 8, 7), "stream", "stream"), ((40, 4, 16), "stream", "c_fallback")]


@pytest.mark.parametrize("shape,train,infer", B_CASES, ids=["x".join(map(str, c[0])) + "-" + c[2] for c in B_CASES])
def test_level_tail_routes_against_oracle(shape, train, infer, monkeypatch):
    import pygat_amd as pg
    Fin, H, Fo = shape
    N = 9100
    rowptr, col, x, W, a, G = _level_data(N, Fin, H, Fo, 200 + Fin + H + Fo, iso=0.45 if Fo == 8 else 0.55)
    _force_tail_routes(monkeypatch)
    fwd = (1, 0) if train in ("fused", "c_fallback") else (0, 1)
    fwd_n = (1, 0) if infer in ("fused", "c_fallback") else (0, 1)
    dev = torch.device("cuda", 0)

    # the row-map route: the level renumbers itself (user_row in the kernels), GATLevelFn
    seen = _spy(monkeypatch)
    graph = _graph(rowptr, col)
    xd, Wd, ad, Gd = _dev(x, W, a, G)
    Wd.requires_grad_(True); ad.requires_grad_(True)
    out = pg.GATLevelFn.apply(xd, Wd, ad, None, graph, 0.2, True)
    out.backward(Gd)
    torch.cuda.synchronize()
    assert graph._ordered is not None
    assert (seen["project_tail"], seen["fwd_stream"], seen["bwd_stream"]) == fwd + (1,), seen
    rep = parity.check_level(out.detach().cpu().numpy(), {"dX": None, "dW": Wd.grad.cpu().numpy(), "da": ad.grad.cpu().numpy()},
                             x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, True, G.numpy(), what=f"row map {shape}",
                             verbose=False)

    # the InternalOrderView route: x given in internal order, gat_level (one parameter tensor per head)
    seen = _spy(monkeypatch)
    view = graph.internal_view()
    to_user, to_int = view.to_user.long(), view.to_internal.long()
    Ws, As = _heads_params(W, a)
    out_i = pg.gat_level(xd[to_user].contiguous(), view, Ws, As, None, 0.2, True)
    out_i.backward(Gd[to_user].contiguous())
    torch.cuda.synchronize()
    assert (seen["project_tail"], seen["fwd_stream"], seen["bwd_stream"]) == fwd + (1,), seen
    dW = torch.stack([w.grad for w in Ws]).cpu().numpy()
    da = torch.stack([v.grad.reshape(-1) for v in As]).cpu().numpy()
    parity.check_level(out_i.detach()[to_int].cpu().numpy(), {"dX": None, "dW": dW, "da": da}, x.numpy(), rowptr, col, W.numpy(),
                       a.numpy(), 0.2, True, G.numpy(), what=f"view {shape}", verbose=False)

    # inference: no a-gradient condition, the fused projection wherever the shape allows it
    seen = _spy(monkeypatch)
    with torch.no_grad():
        out_n = pg.GATLevelFn.apply(xd, Wd.detach(), ad.detach(), None, graph, 0.2, True)
    torch.cuda.synchronize()
    assert (seen["project_tail"], seen["fwd_stream"], seen["bwd_stream"]) == fwd_n + (0,), seen
    parity.close_fwd(out_n.cpu(), rep["ref64"]["out"], f"no_grad {shape} out", rep["ref32"]["out"])


def test_gatv2_level_tail_against_oracle(monkeypatch):
    """GATv2LevelFn renumbering itself, the tail through both streams: out, dW, da against oracle.level_forward_v2."""
    import pygat_amd as pg
    from pygat_amd import gatv2, ops
    from oracle import gat_oracle as O
    N, Fin, H, Fo = 9000, 32, 4, 16
    rowptr, col = _iso_csr(N, 0.5, 90)
    g = torch.Generator().manual_seed(91)
    x = torch.randn(N, Fin, generator=g, dtype=torch.float64).float().double()
    W = (torch.randn(H, 2 * Fin, Fo, generator=g, dtype=torch.float64) * 0.2).float().double()
    a = (torch.randn(H, Fo, generator=g, dtype=torch.float64) * 0.4).float().double()
    G = torch.randn(N, H * Fo, generator=g, dtype=torch.float64).float().double()
    _force_tail_routes(monkeypatch)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(gatv2, "lib", ops.lib)
    graph = _graph(rowptr, col)
    xd, Wd, ad, Gd = _dev(x, W, a, G)
    Wd.requires_grad_(True); ad.requires_grad_(True)
    out = pg.GATv2LevelFn.apply(xd, Wd, ad, None, graph, 0.2, True)
    out.backward(Gd)
    torch.cuda.synchronize()
    assert graph._ordered is not None and (seen["fwd_stream"], seen["bwd_stream"]) == (1, 1), seen
    oracle = lambda W_, a_: O.level_forward_v2(x.to(W_.dtype), (rowptr, col), W_, a_, 0.2, True)  # noqa: E731
    parity.check_autograd(out.detach().cpu(), [Wd.grad.cpu(), ad.grad.cpu()], oracle, [W, a], G, ["dW", "da"], what="v2 tail")


# ----------------------------------------------------------------------------------------------------------------------------
# C. a degree-ordered graph handed in directly: level(x[to_user], g_int) = level(x, g), `out` at the caller's rows
@pytest.mark.parametrize("tail", [True, False], ids=["tail", "no_tail"])
@pytest.mark.parametrize("x_grad", [False, True], ids=["x", "x_grad"])
def test_degree_ordered_graph_handed_in(tail, x_grad, monkeypatch):
    import pygat_amd as pg
    from oracle import gat_oracle as O
    N, Fin, H, Fo = 9000, 64, 4, 16
    rowptr, col, x, W, a, G = _level_data(N, Fin, H, Fo, 300)
    if not tail:
        rowptr, col = (np.asarray(v) for v in O.random_symmetric_csr(N, 8, 301, hub=(4, 1200)))
    _force_tail_routes(monkeypatch)
    seen = _spy(monkeypatch)
    g_int, to_user, to_int = _graph(rowptr, col).degree_ordered()
    to_user, to_int = to_user.long(), to_int.long()
    xd, Wd, ad, Gd = _dev(x, W, a, G)
    xi = xd[to_user].contiguous().requires_grad_(x_grad)
    Wd.requires_grad_(True); ad.requires_grad_(True)
    out = pg.GATLevelFn.apply(xi, Wd, ad, None, g_int, 0.2, True)
    out.backward(Gd)                                     # G at the caller's rows, like `out`
    torch.cuda.synchronize()
    took = seen["project_tail"] + seen["fwd_stream"]
    assert (took == 1 and seen["bwd_stream"] == 1) if tail else (took == 0 and seen["bwd_stream"] == 0), seen
    grads = {"dX": xi.grad[to_int].cpu().numpy() if x_grad else None, "dW": Wd.grad.cpu().numpy(), "da": ad.grad.cpu().numpy()}
    parity.check_level(out.detach().cpu().numpy(), grads, x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, True, G.numpy(),
                       what=f"degree-ordered graph, tail {tail}, dX {x_grad}", verbose=False)

    # gat_level (one tensor per head) on the same graph
    Ws, As = _heads_params(W, a)
    out_h = pg.gat_level(xd[to_user].contiguous(), g_int, Ws, As, None, 0.2, True)
    out_h.backward(Gd)
    torch.cuda.synchronize()
    dW = torch.stack([w.grad for w in Ws]).cpu().numpy()
    da = torch.stack([v.grad.reshape(-1) for v in As]).cpu().numpy()
    parity.check_level(out_h.detach().cpu().numpy(), {"dX": None, "dW": dW, "da": da}, x.numpy(), rowptr, col, W.numpy(), a.numpy(),
                       0.2, True, G.numpy(), what=f"degree-ordered graph, gat_level, tail {tail}", verbose=False)


def test_degree_ordered_graph_gatv2_handed_in(monkeypatch):
    import pygat_amd as pg
    from oracle import gat_oracle as O
    N, Fin, H, Fo = 9000, 32, 4, 16
    rowptr, col = _iso_csr(N, 0.5, 310)
    g = torch.Generator().manual_seed(311)
    x = torch.randn(N, Fin, generator=g, dtype=torch.float64).float().double()
    W = (torch.randn(H, 2 * Fin, Fo, generator=g, dtype=torch.float64) * 0.2).float().double()
    a = (torch.randn(H, Fo, generator=g, dtype=torch.float64) * 0.4).float().double()
    G = torch.randn(N, H * Fo, generator=g, dtype=torch.float64).float().double()
    _force_tail_routes(monkeypatch)
    g_int, to_user, to_int = _graph(rowptr, col).degree_ordered()
    xd, Wd, ad, Gd = _dev(x, W, a, G)
    xi = xd[to_user.long()].contiguous().requires_grad_(True)
    Wd.requires_grad_(True); ad.requires_grad_(True)
    out = pg.GATv2LevelFn.apply(xi, Wd, ad, None, g_int, 0.2, True)
    out.backward(Gd)
    torch.cuda.synchronize()
    oracle = lambda x_, W_, a_: O.level_forward_v2(x_, (rowptr, col), W_, a_, 0.2, True)  # noqa: E731
    parity.check_autograd(out.detach().cpu(), [xi.grad[to_int.long()].cpu(), Wd.grad.cpu(), ad.grad.cpu()], oracle, [x, W, a], G,
                          ["dX", "dW", "da"], what="v2 degree-ordered graph")


def test_degree_ordered_graph_refused_where_the_map_cannot_be_honoured(monkeypatch):
    import pygat_amd as pg
    from pygat_amd.dropout import gat_level_dropout
    N, Fin, H, Fo = 9000, 64, 4, 16
    rowptr, col, x, W, a, G = _level_data(N, Fin, H, Fo, 320)
    graph = _graph(rowptr, col)
    g_int, to_user, _ = graph.degree_ordered()
    xd, Wd, ad = _dev(x, W, a)
    xi = xd[to_user.long()].contiguous()
    Ws, As = _heads_params(W, a)
    with pytest.raises(ValueError, match="internal_view"):
        gat_level_dropout(xi, g_int, Ws, As, None, 0.2, True, 0.5)
    with pytest.raises(ValueError, match="internal_view"):
        pg.GATLevelFn.apply(xi, Wd, ad, None, g_int, 0.2, True, None, (2, lambda *args: None))
    with pytest.raises(ValueError, match="internal_view"):        # a mean over heads: head_mean writes internal rows
        pg.GATLevelFn.apply(xi, Wd, ad, None, g_int, 0.2, False)
    # ... while the unmapped view takes the pipeline
    view = graph.internal_view()
    hand = []
    out = pg.GATLevelFn.apply(xd[view.to_user.long()].contiguous(), Wd, ad, None, view, 0.2, True, None,
                              (2, lambda c, r0, r1, o: hand.append((r0, r1))))
    torch.cuda.synchronize()
    assert hand and hand[0][0] == 0 and hand[-1][1] == N and torch.isfinite(out).all()


# ----------------------------------------------------------------------------------------------------------------------------
# D. degenerate tails
def _identity_csr(N, pair=False):
    rows, cols = np.arange(N), np.arange(N)
    if pair:                                         # one edge pair between nodes 1 and N - 2: two rows of degree 2
        rows, cols = np.concatenate([rows, [1, N - 2]]), np.concatenate([cols, [N - 2, 1]])
    o = np.lexsort((cols, rows))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=N))]).astype(np.int32)
    return rowptr, cols[o].astype(np.int32)


def _short_tail_csr(N, seed):
    """A connected graph (mean degree 12: no node of its own without edges) + a few self-loop-only nodes that do not begin a slot
    of their own (self_loop_tail is None: no tail route, the whole pattern through the fused kernels)."""
    from oracle import gat_oracle as O
    from pygat_amd.graph import slot_edges_for
    for k in (1, 2, 3, 5):
        rp0, c0 = (np.asarray(v, dtype=np.int64) for v in O.random_symmetric_csr(N - k, 12, seed))
        rowptr = np.concatenate([rp0, rp0[-1] + np.arange(1, k + 1)]).astype(np.int32)
        col = np.concatenate([c0, np.arange(N - k, N)]).astype(np.int32)
        g_int = _graph(rowptr, col).degree_ordered()[0]
        if int((np.diff(rowptr) == 1).sum()) >= 1 and g_int.fwd.self_loop_tail(slot_edges_for(64, g_int.slot_edges)) is None:
            return rowptr, col
    raise AssertionError("no self-loop-only tail inside the last slot found")


DEGENERATE = {"identity": lambda N: _identity_csr(N), "one_pair": lambda N: _identity_csr(N, pair=True),
              "short_tail": lambda N: _short_tail_csr(N, 330)}


@pytest.mark.parametrize("kind", list(DEGENERATE))
def test_degenerate_tails_level(kind, monkeypatch):
    """The row-map and the view route of one level (H 8 x F' 8, Fin 64: the fused projection's shape), with and without grad."""
    import pygat_amd as pg
    from pygat_amd.graph import slot_edges_for
    N, Fin, H, Fo = 8500, 64, 8, 8
    rowptr, col = DEGENERATE[kind](N)
    _, _, x, W, a, G = _level_data(N, Fin, H, Fo, 340)
    _force_tail_routes(monkeypatch)
    graph = _graph(rowptr, col)
    t = graph.degree_ordered()[0].fwd.self_loop_tail(slot_edges_for(H * Fo, graph.slot_edges))
    if kind == "one_pair":
        assert t is not None and t[0] > 0
    else:
        assert t is None
    xd, Wd, ad, Gd = _dev(x, W, a, G)
    Wd.requires_grad_(True); ad.requires_grad_(True)
    out = pg.GATLevelFn.apply(xd, Wd, ad, None, graph, 0.2, True)
    out.backward(Gd)
    torch.cuda.synchronize()
    assert graph._ordered is not None
    da = ad.grad.cpu().numpy()
    if kind == "identity":
        # every row its own softmax of one: out = ELU(x W), da = 0 exactly.  The oracle's per-edge de_ij = alpha_ij (dp_ij - D_i)
        # cancels exactly in fp32 too; the row-local backward forms ds_i from the saved output instead, and its fp32 rounding
        # (~1e-7 a row) sums to a few 1e-5 over 8500 rows -- priced here on its own, the rest by the one rule
        assert np.abs(da).max() <= 1e-4, np.abs(da).max()
        da = np.zeros_like(da)
    rep = parity.check_level(out.detach().cpu().numpy(), {"dX": None, "dW": Wd.grad.cpu().numpy(), "da": da},
                             x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, True, G.numpy(), what=f"{kind} row map", verbose=False)
    if kind == "identity":
        Wh = torch.einsum("nk,hkf->nhf", x, W).reshape(N, H * Fo)
        assert np.abs(rep["ref64"]["out"] - torch.nn.functional.elu(Wh).numpy()).max() < 1e-12
        assert np.abs(rep["ref64"]["da"]).max() == 0.0
    with torch.no_grad():
        out_n = pg.GATLevelFn.apply(xd, Wd.detach(), ad.detach(), None, graph, 0.2, True)
    parity.close_fwd(out_n.cpu(), rep["ref64"]["out"], f"{kind} row map no_grad", rep["ref32"]["out"])

    view = graph.internal_view()
    to_user, to_int = view.to_user.long(), view.to_internal.long()
    Ws, As = _heads_params(W, a)
    out_i = pg.gat_level(xd[to_user].contiguous(), view, Ws, As, None, 0.2, True)
    out_i.backward(Gd[to_user].contiguous())
    torch.cuda.synchronize()
    dW = torch.stack([w.grad for w in Ws]).cpu().numpy()
    da = torch.stack([v.grad.reshape(-1) for v in As]).cpu().numpy()
    if kind == "identity":      # (as above)
        assert np.abs(da).max() <= 1e-4, np.abs(da).max()
        da = np.zeros_like(da)
    parity.check_level(out_i.detach()[to_int].cpu().numpy(), {"dX": None, "dW": dW, "da": da}, x.numpy(), rowptr, col, W.numpy(),
                       a.numpy(), 0.2, True, G.numpy(), what=f"{kind} view", verbose=False)
    with torch.no_grad():
        out_in = pg.gat_level(xd[to_user].contiguous(), view, [w.detach() for w in Ws], [v.detach() for v in As], None, 0.2, True)
    parity.close_fwd(out_in[to_int].cpu(), rep["ref64"]["out"], f"{kind} view no_grad", rep["ref32"]["out"])


@pytest.mark.parametrize("kind", list(DEGENERATE))
def test_degenerate_tails_model(kind, monkeypatch):
    """A 2-level pygat_amd.GAT that runs in internal order (_internal_order_pays): logits and every parameter gradient."""
    import pygat_amd as pg
    from oracle import gat_oracle as O
    N, Fin, C_ = 8500, 64, 5
    rowptr, col = DEGENERATE[kind](N)
    _force_tail_routes(monkeypatch)
    graph = _graph(rowptr, col)
    g = torch.Generator().manual_seed(350)
    x = torch.randn(N, Fin, generator=g).cuda()
    G = torch.randn(N, C_, generator=g, dtype=torch.float64).float().double()
    torch.manual_seed(351)
    model = pg.GAT([Fin, 8, C_], [8, 1], 2, 0.0, 0.2, pg.SpGraphAttentionLayer).cuda()
    assert model._internal_order_pays(x, graph, 0.0)
    y = model(x, graph)
    y.backward(G.float().cuda())
    torch.cuda.synchronize()
    with torch.no_grad():
        y_n = model(x, graph)
    levels = [(torch.stack([h.W.detach().cpu().double() for h in hs]), torch.stack([h.a.detach().cpu().double().reshape(-1) for h in hs]))
              for hs in model.gat_layers]
    got = []
    for hs in model.gat_layers:
        got += [torch.stack([h.W.grad.cpu() for h in hs]), torch.stack([h.a.grad.cpu().reshape(-1) for h in hs])]
    x64 = x.cpu().double()
    if kind == "identity":      # da1 = 0 exactly; the row-local backward's fp32 rounding priced on its own (test_degenerate_tails_level)
        assert float(got[1].abs().max()) <= 1e-4, float(got[1].abs().max())
        got[1] = None

    def oracle(W1, a1, W2, a2):
        return O.model_forward(x64.to(W1.dtype), (rowptr, col), [{"W": W1, "a": a1, "skip": None}, {"W": W2, "a": a2, "skip": None}], 0.2)
    leaves = [levels[0][0], levels[0][1], levels[1][0], levels[1][1]]
    _, (y64, _) = parity.check_autograd(y.detach().cpu(), got, oracle, leaves, G, ["dW1", "da1", "dW2", "da2"], what=f"{kind} model")
    parity.close_fwd(y_n.cpu(), y64, f"{kind} model no_grad", oracle(*[t.float() for t in leaves]).detach())
