"""return_attention: the per-edge attention coefficients of the GAT and GATv2 levels (csrc/k13_attention.hip) against an fp64
restatement of the oracle's sparse_head_forward / sparse_head_forward_v2 (s, t, e, m, Z in float64 on the CPU; the same
restatement in float32 prices the small coefficients).  Criteria, per alpha [E, H]:
  * parity.close_fwd against fp64 (absolute 1e-5: alpha <= 1);
  * log alpha by parity.close_grad (fp32 restatement as the own-precision yardstick) on the edges with alpha64 > 1e-30;
  * every row sums to 1 within (deg_i + 4) 2^-23; every single-edge row is exactly 1.0; finite and >= 0.
Rows of alpha follow the edge order of the graph the caller passed (CSRGraph.edge_index()), whatever node order the level ran in.
Asking for the attention changes no output and no gradient bit (torch.equal)."""
import numpy as np
import pytest
import torch

import parity
from pattern_device import DEV, _graph
from pattern_graphs import SHAPES, SID, SLOPE, _asym_graph, _hub_graph, _params
from tail_case import _iso_csr

pytestmark = pytest.mark.gpu


def _leaky(z):
    return torch.where(z > 0, z, SLOPE * z)


def _src(rowptr):
    rp = torch.as_tensor(np.asarray(rowptr), dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])


def _softmax_rows(e, src, N):
    """e [E, H] -> alpha = exp(e - m[src]) / Z[src] (layers.py:145-150), per head."""
    H = e.shape[1]
    m = torch.full((N, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, src[:, None].expand(-1, H), e, "amax", include_self=True)
    p = torch.exp(e - m[src])
    Z = torch.zeros(N, H, dtype=e.dtype).index_add(0, src, p)
    return p / Z[src]


def alpha_v1(x, rowptr, col, W, a, dtype, mask_x=None, mask_wh=None):
    """x [N, Fin], W [H, Fin, F'], a [H, 2F'] -> alpha [E, H] (oracle.sparse_head_forward, layers.py:132-150)."""
    src, col = _src(rowptr), torch.as_tensor(np.asarray(col), dtype=torch.int64)
    H, _, Fo = W.shape
    es = []
    for h in range(H):
        xh = x.to(dtype) if mask_x is None else x.to(dtype) * mask_x[h].to(dtype)
        Wh = xh @ W[h].to(dtype)
        if mask_wh is not None:
            Wh = Wh * mask_wh[h].to(dtype)
        ah = a[h].reshape(-1).to(dtype)
        es.append(_leaky((Wh @ ah[:Fo])[src] + (Wh @ ah[Fo:])[col]))
    return _softmax_rows(torch.stack(es, 1), src, x.shape[0])


def alpha_v2(x, rowptr, col, W, a, dtype, mask_x=None, mask_whi=None, mask_whj=None):
    """x [N, Fin], W [H, 2Fin, F'], a [H, F'] -> alpha [E, H] (oracle.sparse_head_forward_v2, layers.py:266-290)."""
    src, col = _src(rowptr), torch.as_tensor(np.asarray(col), dtype=torch.int64)
    H, Fin2, Fo = W.shape
    Fin = Fin2 // 2
    es = []
    for h in range(H):
        xh = x.to(dtype) if mask_x is None else x.to(dtype) * mask_x[h].to(dtype)
        Whi, Whj = xh @ W[h, :Fin].to(dtype), xh @ W[h, Fin:].to(dtype)
        if mask_whi is not None:
            Whi, Whj = Whi * mask_whi[h].to(dtype), Whj * mask_whj[h].to(dtype)
        es.append(_leaky(Whi[src] + Whj[col]) @ a[h].reshape(-1).to(dtype))
    return _softmax_rows(torch.stack(es, 1), src, x.shape[0])


def check_alpha(got, rowptr, a64, a32=None, what="alpha"):
    assert not got.requires_grad and got.dtype == torch.float32, what
    g = got.detach().double().cpu()
    assert g.shape == a64.shape, (what, g.shape, a64.shape)
    assert torch.isfinite(g).all() and (g >= 0).all(), f"{what}: non-finite or negative coefficients"
    parity.close_fwd(g, a64, what)
    if a32 is not None:
        sel = a64 > 1e-30
        parity.close_grad(torch.log(g[sel]), torch.log(a64[sel]), torch.log(a32.double()[sel]), what + " log")
    src = _src(rowptr)
    deg = torch.as_tensor(np.diff(np.asarray(rowptr)), dtype=torch.float64)
    sums = torch.zeros(len(deg), g.shape[1], dtype=torch.float64).index_add(0, src, g)
    bound = ((deg + 4) * 2.0 ** -23)[:, None]
    live = (deg > 0)[:, None]
    assert ((sums - 1).abs() <= bound)[live.expand_as(sums)].all(), f"{what}: a row sum is off by {(sums - 1).abs().max():.3e}"
    single = (deg == 1)[src]
    assert (g[single] == 1.0).all(), f"{what}: a single-edge row is not exactly 1"


def _run_v1(x, W, a, graph, concat, S=None, **kw):
    import pygat_amd as pg
    H = W.shape[0]
    return pg.gat_level(x.to(DEV), graph, [W[h].to(DEV) for h in range(H)], [a[h].to(DEV) for h in range(H)],
                        None if S is None else [S[h].to(DEV) for h in range(H)], SLOPE, concat, **kw)


def _run_v2(x, W, a, graph, concat, S=None, **kw):
    from pygat_amd.gatv2 import gatv2_level
    H = W.shape[0]
    return gatv2_level(x.to(DEV), graph, [W[h].to(DEV) for h in range(H)], [a[h].to(DEV) for h in range(H)],
                       None if S is None else [S[h].to(DEV) for h in range(H)], SLOPE, concat, **kw)


# ------------------------------------------------------------------------------------------------------- v1 and GATv2, lane shapes
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_v1_lane_shapes(shape, concat, skip):
    H, Fo = shape
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=H * 100 + Fo)
    with torch.no_grad():
        out, al = _run_v1(x, W, a, _graph(rowptr, col), concat, S if skip else None, return_attention=True)
    assert al.shape == (len(col), H) and out.shape[0] == len(rowptr) - 1
    check_alpha(al, rowptr, alpha_v1(x, rowptr, col, W, a, torch.float64), alpha_v1(x, rowptr, col, W, a, torch.float32),
                f"v1 {shape}")


@pytest.mark.parametrize("shape", [(1, 7), (8, 16), (4, 64)], ids=["1x7", "8x16", "4x64"])
def test_v1_asymmetric_pattern(shape):
    H, Fo = shape
    rowptr, col = _asym_graph()
    x, W, a, _ = _params(len(rowptr) - 1, 32, H, Fo, seed=7)
    with torch.no_grad():
        _, al = _run_v1(x, W, a, _graph(rowptr, col), True, return_attention=True)
    check_alpha(al, rowptr, alpha_v1(x, rowptr, col, W, a, torch.float64), alpha_v1(x, rowptr, col, W, a, torch.float32), "v1 asym")


@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_v2_lane_shapes(shape, concat):
    H, Fo = shape
    rowptr, col = _hub_graph(seed=5)
    x, W, a, S = _params(len(rowptr) - 1, 40, H, Fo, seed=H * 10 + Fo, v2=True)
    with torch.no_grad():
        _, al = _run_v2(x, W, a, _graph(rowptr, col), concat, S if concat else None, return_attention=True)
    check_alpha(al, rowptr, alpha_v2(x, rowptr, col, W, a, torch.float64), alpha_v2(x, rowptr, col, W, a, torch.float32),
                f"v2 {shape}")


def test_v2_asymmetric_pattern():
    rowptr, col = _asym_graph(seed=9)
    x, W, a, _ = _params(len(rowptr) - 1, 24, 4, 16, seed=9, v2=True)
    with torch.no_grad():
        _, al = _run_v2(x, W, a, _graph(rowptr, col), True, return_attention=True)
    check_alpha(al, rowptr, alpha_v2(x, rowptr, col, W, a, torch.float64), alpha_v2(x, rowptr, col, W, a, torch.float32), "v2 asym")


# ------------------------------------------------------------------------------------------------------------------ layer classes
def _dense_adj(N=300, seed=11):
    rng = np.random.default_rng(seed)
    adj = torch.zeros(N, N)
    r, c = rng.integers(0, N, 5 * N), rng.integers(0, N, 5 * N)
    adj[r, c] = torch.from_numpy(rng.uniform(-1, 1, r.size)).float()     # negative entries: in `nonzero`, not in `positive`
    adj[torch.arange(N), torch.arange(N)] = 1.0
    adj[3, :] = 0.0; adj[3, 3] = 1.0                                     # a single-edge row
    return adj


def _csr_of(mask):
    rr, cc = mask.nonzero(as_tuple=True)
    rowptr = np.concatenate([[0], np.cumsum(torch.bincount(rr, minlength=mask.shape[0]).numpy())]).astype(np.int32)
    return rowptr, cc.numpy().astype(np.int32)


@pytest.mark.parametrize("cls", ["GraphAttentionLayer", "SpGraphAttentionLayer", "SpGraphAttentionLayerV2", "GraphAttentionLayerV2"])
def test_layer_classes_dense_adj(cls):
    import pygat_amd as pg
    from pygat_amd import gatv2
    torch.manual_seed(0)
    adj = _dense_adj()
    N, Fin, Fo = adj.shape[0], 20, 12
    layer = (getattr(pg, cls, None) or getattr(gatv2, cls))(Fin, Fo, dropout=0.5, alpha=SLOPE, concat=True).to(DEV).eval()
    x = torch.randn(N, Fin)
    with torch.no_grad():
        out, al = layer(x.to(DEV), adj.to(DEV), return_attention=True)
        ref_out = layer(x.to(DEV), adj.to(DEV))
    assert torch.equal(out, ref_out) and al.shape[1] == 1
    mode = layer.pattern_mode
    rowptr, col = _csr_of(adj > 0 if mode == "positive" else adj != 0)
    g = pg.as_graph(adj.to(DEV), mode)
    assert torch.equal(g.edge_index().cpu(), torch.stack([_src(rowptr), torch.as_tensor(col, dtype=torch.int64)]))
    W, a = layer.W.detach().cpu()[None], layer.a.detach().cpu().reshape(1, -1)
    if cls == "GraphAttentionLayerV2":             # uniform attention: 1 / deg_i (gatv2.py module docstring)
        deg = torch.as_tensor(np.diff(rowptr), dtype=torch.float64)
        a64 = (1.0 / deg)[_src(rowptr)][:, None]
        check_alpha(al, rowptr, a64, None, cls)
        assert torch.equal(al.cpu().double(), (1.0 / deg.float()).double()[_src(rowptr)][:, None])
        return
    # GraphAttentionLayer: the reference's attention[adj > 0] (layers.py:41-43) = the softmax rows over the positive pattern
    fn = alpha_v2 if "V2" in cls else alpha_v1
    check_alpha(al, rowptr, fn(x, rowptr, col, W, a, torch.float64), fn(x, rowptr, col, W, a, torch.float32), cls)


# --------------------------------------------------------------------------------------------------- renumbered and tail routes
def _force(monkeypatch, fused):
    from pygat_amd import ops
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES_TAIL", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "TAIL_FUSED", fused)


ROUTE_N = 9000


@pytest.fixture(scope="module")
def iso():
    rowptr, col = _iso_csr(ROUTE_N, 0.55, 21)
    x, W, a, _ = _params(ROUTE_N, 128, 8, 16, seed=21)
    a64 = alpha_v1(x, rowptr, col, W, a, torch.float64)
    a32 = alpha_v1(x, rowptr, col, W, a, torch.float32)
    return rowptr, col, x, W, a, a64, a32


@pytest.mark.parametrize("fused", [True, False], ids=["tail_fused", "tail_stream"])
@pytest.mark.parametrize("route", ["level_renumbers", "internal_view", "degree_ordered"])
def test_routes(iso, route, fused, monkeypatch):
    from pygat_amd import ops
    _force(monkeypatch, fused)
    rowptr, col, x, W, a, a64, a32 = iso
    graph = _graph(rowptr, col)
    calls = {"n": 0}
    real = ops.lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name == "pygat_project_tail_blocked":
                def wrapped(*args):
                    calls["n"] += 1
                    return fn(*args)
                return wrapped
            return fn
    monkeypatch.setattr(ops, "lib", Spy())
    if route == "level_renumbers":
        with torch.no_grad():
            out, al = _run_v1(x, W, a, graph, True, return_attention=True)
        check_alpha(al, rowptr, a64, a32, route)
        assert torch.equal(graph.edge_index().cpu(), torch.stack([_src(rowptr), torch.as_tensor(col, dtype=torch.int64)]))
    else:
        g2 = graph.internal_view() if route == "internal_view" else graph.degree_ordered()[0]
        to_user = graph.degree_ordered()[1].long().cpu()
        xi = x[to_user]
        with torch.no_grad():
            out, al = _run_v1(xi, W, a, g2, True, return_attention=True)
        # alpha follows the graph passed: its edge k = (p, q) in internal ids is the caller's edge (to_user[p], to_user[q])
        ei = g2.edge_index().cpu()
        rp2 = g2.fwd.rowptr.cpu().numpy()
        assert torch.equal(ei[0], _src(rp2))
        key_user = (to_user[ei[0]] * ROUTE_N + to_user[ei[1]])
        key_ref = _src(rowptr) * ROUTE_N + torch.as_tensor(col, dtype=torch.int64)
        order = torch.argsort(key_ref)
        pos = order[torch.searchsorted(key_ref[order], key_user)]
        assert torch.equal(key_ref[pos], key_user)
        check_alpha(al, rp2, a64[pos], a32[pos], route)
    assert (calls["n"] > 0) == fused, calls


@pytest.mark.parametrize("fused", [True, False], ids=["tail_fused", "tail_stream"])
def test_two_level_model_internal_order(fused, monkeypatch):
    import pygat_amd as pg
    _force(monkeypatch, fused)
    rowptr, col = _iso_csr(ROUTE_N, 0.55, 23)
    torch.manual_seed(1)
    model = pg.GAT(nfeat=[64, 16, 6], nheads=[8, 1], nlayers=2, dropout=0.5, alpha=SLOPE,
                   layer_type=pg.SpGraphAttentionLayer).to(DEV).eval()
    graph = _graph(rowptr, col)
    assert model._internal_order_pays(torch.zeros(ROUTE_N, 64, device=DEV), graph, 0.0)
    x = torch.randn(ROUTE_N, 64)
    with torch.no_grad():
        out, alphas = model(x.to(DEV), graph, return_attention=True)
        ref_out = model(x.to(DEV), graph)
    assert torch.equal(out, ref_out) and len(alphas) == 2
    W1 = torch.stack([getattr(model, f"attention_layer_1_head_{h}").W.detach().cpu() for h in range(1, 9)])
    a1 = torch.stack([getattr(model, f"attention_layer_1_head_{h}").a.detach().cpu().reshape(-1) for h in range(1, 9)])
    check_alpha(alphas[0], rowptr, alpha_v1(x, rowptr, col, W1, a1, torch.float64), alpha_v1(x, rowptr, col, W1, a1, torch.float32),
                "model level 1")
    # level 2 on the fp64 restatement of level 1's output
    from oracle import gat_oracle as O
    h1 = O.level_forward(x.double(), (torch.as_tensor(rowptr, dtype=torch.int64), torch.as_tensor(col, dtype=torch.int64)),
                         W1.double(), a1.double(), SLOPE, True)
    W2 = model.attention_layer_2_head_1.W.detach().cpu()[None]
    a2 = model.attention_layer_2_head_1.a.detach().cpu().reshape(1, -1)
    check_alpha(alphas[1], rowptr, alpha_v1(h1, rowptr, col, W2, a2, torch.float64), None, "model level 2")
    assert alphas[1].shape == (len(col), 1)


# ---------------------------------------------------------------------------------------------------------- train-mode dropout
def test_v1_dropout_masks():
    from pygat_amd.dropout import draw_masks, gat_level_dropout
    rowptr, col = _hub_graph(seed=8)
    N, Fin, H, Fo = len(rowptr) - 1, 32, 8, 16
    x, W, a, _ = _params(N, Fin, H, Fo, seed=8)
    masks = draw_masks(0.4, H, N, Fin, Fo, len(col), DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    Wd = [W[h].to(DEV).requires_grad_(True) for h in range(H)]
    Ad = [a[h].to(DEV).requires_grad_(True) for h in range(H)]
    out, al = gat_level_dropout(x.to(DEV), _graph(rowptr, col), Wd, Ad, None, SLOPE, True, 0.4, masks=masks, return_attention=True)
    out2 = gat_level_dropout(x.to(DEV), _graph(rowptr, col), Wd, Ad, None, SLOPE, True, 0.4, masks=masks)
    assert torch.equal(out, out2)
    mx, mw = masks["x"].cpu(), masks["wh"].cpu()
    check_alpha(al, rowptr, alpha_v1(x, rowptr, col, W, a, torch.float64, mx, mw), alpha_v1(x, rowptr, col, W, a, torch.float32, mx, mw),
                "v1 dropout")


def test_v2_dropout_masks():
    from pygat_amd.gatv2 import draw_masks_v2
    rowptr, col = _hub_graph(seed=6)
    N, Fin, H, Fo = len(rowptr) - 1, 24, 4, 16
    x, W, a, _ = _params(N, Fin, H, Fo, seed=6, v2=True)
    masks = draw_masks_v2(0.3, H, N, Fin, Fo, len(col), DEV, generator=torch.Generator(device=DEV).manual_seed(4))
    _, al = _run_v2(x, W, a, _graph(rowptr, col), True, masks=masks, return_attention=True)
    mk = {k: v.cpu() for k, v in masks.items()}
    check_alpha(al, rowptr, alpha_v2(x, rowptr, col, W, a, torch.float64, mk["x"], mk["whi"], mk["whj"]),
                alpha_v2(x, rowptr, col, W, a, torch.float32, mk["x"], mk["whi"], mk["whj"]), "v2 dropout")


# ------------------------------------------------------------------------------------------------------------------- invariance
def _grads_v1(x, W, a, S, graph, concat, ra, x_grad=True, kind="v1", masks=None):
    H = W.shape[0]
    xd = x.to(DEV).requires_grad_(x_grad)
    Ws = [W[h].to(DEV).requires_grad_(True) for h in range(H)]
    As = [a[h].to(DEV).requires_grad_(True) for h in range(H)]
    Ss = None if S is None else [S[h].to(DEV).requires_grad_(True) for h in range(H)]
    if kind == "v1":
        import pygat_amd as pg
        r = pg.gat_level(xd, graph, Ws, As, Ss, SLOPE, concat, return_attention=ra)
    else:
        from pygat_amd.gatv2 import gatv2_level
        r = gatv2_level(xd, graph, Ws, As, Ss, SLOPE, concat, masks=masks, return_attention=ra)
    out = r[0] if ra else r
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    leaves = ([xd] if x_grad else []) + Ws + As + (Ss or [])
    return [out.detach()] + list(torch.autograd.grad(out, leaves, G))


@pytest.mark.parametrize("case", ["v1-8x16-skip", "v1-4x64-mean", "v1-1x7", "v2-8x16", "v2-4x64-mean", "v2-4x16-masks"])
def test_invariance_training(case):
    kind = case.split("-")[0]
    H, Fo = map(int, case.split("-")[1].split("x"))
    concat, skip = "mean" not in case, "skip" in case
    rowptr, col = _hub_graph(seed=12)
    N = len(rowptr) - 1
    x, W, a, S = _params(N, 32, H, Fo, seed=12, v2=kind == "v2")
    masks = None
    if case.endswith("masks"):
        from pygat_amd.gatv2 import draw_masks_v2
        masks = draw_masks_v2(0.3, H, N, 32, Fo, len(col), DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    graph = _graph(rowptr, col)
    a_ = _grads_v1(x, W, a, S if skip else None, graph, concat, False, kind=kind, masks=masks)
    b_ = _grads_v1(x, W, a, S if skip else None, graph, concat, True, kind=kind, masks=masks)
    for k, (u, v) in enumerate(zip(a_, b_)):
        assert torch.equal(u, v), (case, k)


@pytest.mark.parametrize("fused", [True, False], ids=["tail_fused", "tail_stream"])
def test_invariance_headline_tail_route(fused, monkeypatch):
    """8 heads x 16 on the renumbered route: training with the tail folded into the projection (dX off: the level renumbers
    only without a gradient into x), and no_grad."""
    _force(monkeypatch, fused)
    rowptr, col = _iso_csr(ROUTE_N, 0.55, 25)
    x, W, a, _ = _params(ROUTE_N, 128, 8, 16, seed=25)
    graph = _graph(rowptr, col)
    a_ = _grads_v1(x, W, a, None, graph, True, False, x_grad=False)
    b_ = _grads_v1(x, W, a, None, graph, True, True, x_grad=False)
    for k, (u, v) in enumerate(zip(a_, b_)):
        assert torch.equal(u, v), k
    with torch.no_grad():
        o1 = _run_v1(x, W, a, graph, True)
        o2, al = _run_v1(x, W, a, graph, True, return_attention=True)
    assert torch.equal(o1, o2)
    o3, al2 = _run_v2(x, torch.cat([W, W], 1), a[:, :16].contiguous(), graph, True, return_attention=True)
    o4 = _run_v2(x, torch.cat([W, W], 1), a[:, :16].contiguous(), graph, True)
    assert torch.equal(o3.detach(), o4.detach())


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refused_combinations():
    import pygat_amd as pg
    from pygat_amd.graphed import FusedEpoch, GraphedLevel
    rowptr, col = _hub_graph(N=200, seed=2)
    graph = _graph(rowptr, col)
    x, W, a, _ = _params(200, 16, 2, 8, seed=2)
    Ws, As = [W[h].to(DEV) for h in range(2)], [a[h].to(DEV) for h in range(2)]
    with pytest.raises(ValueError, match="return_attention"):
        pg.gat_level(x.to(DEV), graph, Ws, As, None, SLOPE, True, pipeline=(2, lambda *a_: None), return_attention=True)
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.0, alpha=SLOPE, head_parallel=True).to(DEV)
    with pytest.raises(ValueError, match="return_attention"):
        model(x.to(DEV), graph, return_attention=True)
    from pygat_amd.dist import gat_level_head_parallel
    with pytest.raises(ValueError, match="return_attention"):
        gat_level_head_parallel(x.to(DEV), graph, Ws, As, None, SLOPE, True, return_attention=True)
    gl = GraphedLevel(graph, x.to(DEV), W.to(DEV), a.to(DEV), warmup=1)
    with pytest.raises(ValueError, match="return_attention"):
        gl.forward(return_attention=True)
    with pytest.raises(ValueError, match="return_attention"):
        gl(return_attention=True)
    with pytest.raises(ValueError, match="return_attention"):
        FusedEpoch.run(object.__new__(FusedEpoch), return_attention=True)


# ------------------------------------------------------------------------------------------------------------------- full size
def test_fullsize_config5_v1():
    """Config 5 (R-MAT 2^20 nodes, 10.7 M edges, 8 heads x 16, Fin 128) against fp64 formed on the device, row chunk by chunk."""
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    rp_h, col_h = rmat_csr_numpy(20, 5_000_000, seed=1)
    rowptr, col = torch.from_numpy(rp_h).to(DEV), torch.from_numpy(col_h).to(DEV)
    graph = pg.CSRGraph(rowptr, col)
    H, Fo, Fin = 8, 16, 128
    g = torch.Generator(device=DEV).manual_seed(2)
    X = torch.randn(graph.n, Fin, generator=g, device=DEV)
    W = torch.randn(H, Fin, Fo, generator=g, device=DEV) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)
    a = torch.randn(H, 2 * Fo, generator=g, device=DEV) * (1.414 * (2.0 / (1 + 2 * Fo)) ** 0.5)
    with torch.no_grad():
        out, al = pg.gat_level(X, graph, list(W), list(a), None, SLOPE, True, return_attention=True)
        ref = pg.gat_level(X, graph, list(W), list(a), None, SLOPE, True)
    assert torch.equal(out, ref)
    del out, ref
    Wh = torch.einsum("nf,hfo->nho", X.double(), W.double())
    s = torch.einsum("nho,ho->nh", Wh, a[:, :Fo].double())
    t = torch.einsum("nho,ho->nh", Wh, a[:, Fo:].double())
    del Wh
    rp = rowptr.long()
    deg = rp[1:] - rp[:-1]
    worst, chunk = 0.0, 1 << 17
    for r0 in range(0, graph.n, chunk):
        r1 = min(graph.n, r0 + chunk)
        e0, e1 = int(rp[r0]), int(rp[r1])
        src = torch.repeat_interleave(torch.arange(r0, r1, device=DEV), deg[r0:r1]) - r0
        e = _leaky(s[r0:r1][src] + t[col[e0:e1].long()])
        m = torch.full((r1 - r0, H), -float("inf"), dtype=torch.float64, device=DEV).scatter_reduce(
            0, src[:, None].expand(-1, H), e, "amax", include_self=True)
        p = torch.exp(e - m[src])
        Z = torch.zeros(r1 - r0, H, dtype=torch.float64, device=DEV).index_add(0, src, p)
        a64 = p / Z[src]
        got = al[e0:e1].double()
        worst = max(worst, float((got - a64).abs().max()))
        sums = torch.zeros(r1 - r0, H, dtype=torch.float64, device=DEV).index_add(0, src, got)
        bound = ((deg[r0:r1].double() + 4) * 2.0 ** -23)[:, None]
        assert ((sums - 1).abs() <= bound).all(), f"rows [{r0}, {r1}): row sum off by {(sums - 1).abs().max():.3e}"
        assert (got[(deg[r0:r1] == 1)[src]] == 1.0).all()
    assert torch.isfinite(al).all() and (al >= 0).all()
    assert worst <= parity.ATOL, worst
