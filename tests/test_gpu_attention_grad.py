"""return_attention="grad": the attention coefficients of the GAT level as a differentiable output (csrc/k14_alpha_grad.hip).

Ground truth is torch autograd in fp64 on the CPU through alpha_grad_case.level_ref, a restatement of the oracle's
sparse_head_forward that returns (out, alpha).  Loss L = <out, G> + <alpha, A>, G and A ~ N(0, 1), seeded.  Pricing is
parity.check_autograd: `out` and alpha by close_fwd, dX / dW / da / dW_skip by close_grad, i.e. max(1e-5, 4 x the fp32 run's own
error).  check_autograd has no treatment of the LeakyReLU kink, so every case asserts, on its fp64 run, that NO (edge, head) has a
logit in the rounding band |z| <= parity.KINK_TAU (|s_i| + |t_j|); the seeds below were chosen on the CPU so that this holds."""
import numpy as np
import pytest
import torch

import parity
from alpha_grad_case import kink_count, level_ref, src_of
from long_row_cases import nine_hubs, three_chunk_hub
from pattern_device import DEV, _graph
from pattern_graphs import SHAPES, SID, SLOPE, _asym_graph, _hub_graph, _params
from tail_case import _iso_csr
from test_gpu_attention import _force

pytestmark = pytest.mark.gpu

# seeds of _params per case: the first from the case's base seed on whose fp64 run no logit lies in the kink band
LANE_SEED = {(1, 7): 107, (8, 8): 808, (8, 16): 816, (4, 64): 464, (4, 256): 656, (16, 64): 1664}
ASYM_SEED = {(1, 7): 7, (8, 16): 7, (4, 64): 7}
ROUTE_SEED, MODEL_SEED, DROPOUT_SEED, SPARSE_SEED = 21, 4, 10, 31
ODD_SEED = {(3, 8): 308, (6, 16): 616}
MODEL_INT_SEED = 1
LONG_ROW_CASES = {"nine_hubs-8x16": (nine_hubs, (8, 16), 816), "nine_hubs-3x8": (nine_hubs, (3, 8), 308),
                  "three_chunk_hub-8x16": (three_chunk_hub, (8, 16), 817)}
ROUTE_N = 9000


def _leaves(x, W, a, S, x_grad=True):
    H = W.shape[0]
    xd = x.to(DEV).requires_grad_(x_grad)
    Ws = [W[h].to(DEV).requires_grad_(True) for h in range(H)]
    As = [a[h].to(DEV).requires_grad_(True) for h in range(H)]
    Ss = None if S is None else [S[h].to(DEV).requires_grad_(True) for h in range(H)]
    return xd, Ws, As, Ss


def _stacked(grads, H, x_grad, skip):
    """autograd.grad's flat tuple -> [dX?, dW [H,..], da [H,..], dW_skip?]"""
    g = list(grads)
    out = [g.pop(0)] if x_grad else []
    out.append(torch.stack(g[:H])); out.append(torch.stack([v.reshape(-1) for v in g[H:2 * H]]))
    if skip:
        out.append(torch.stack(g[2 * H:3 * H]))
    return out


def _GA(out_shape, E, H, seed=5):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(out_shape, generator=g, dtype=torch.float64), torch.randn(E, H, generator=g, dtype=torch.float64)


def _run_level(graph, x, W, a, S, concat, x_grad=True, mode="grad", fn=None, **kw):
    import pygat_amd as pg
    xd, Ws, As, Ss = _leaves(x, W, a, S, x_grad)
    r = (fn or pg.gat_level)(xd, graph, Ws, As, Ss, SLOPE, concat, return_attention=mode, **kw)
    leaves = ([xd] if x_grad else []) + Ws + As + (Ss or [])
    return r, leaves


def _check(what, rowptr, col, x, W, a, S, concat, graph=None, x_grad=True, masks=None, nan_single=False, out_rows=None, **kw):
    """One level in "grad" mode against level_ref; -> the HIP gradients."""
    H = W.shape[0]
    mk = None if masks is None else {k: v.cpu() for k, v in masks.items()}
    assert kink_count(x, rowptr, col, W, a, SLOPE, None if mk is None else mk["x"], None if mk is None else mk["wh"]) == 0, \
        f"{what}: an input with a logit inside the kink band -- choose another seed"
    graph = graph if graph is not None else _graph(rowptr, col)
    (out, al), leaves = _run_level(graph, x, W, a, S, concat, x_grad, **kw)
    assert al.requires_grad and al.shape == (len(col), H) and al.dtype == torch.float32
    if out_rows is not None:
        out = out.index_select(0, out_rows.to(DEV))
    G, A = _GA(tuple(out.shape), len(col), H)
    A_dev = A.clone()
    if nan_single:      # the gradient rows of single-edge rows must not be read; their true contribution is exactly zero
        single = (torch.as_tensor(np.diff(np.asarray(rowptr))) == 1)[src_of(rowptr)]
        assert int(single.sum()) > 0
        A_dev[single] = float("nan")
        A[single] = 0.0
    grads = torch.autograd.grad([out, al], leaves, [G.float().to(DEV), A_dev.float().to(DEV)])
    got = _stacked(grads, H, x_grad, S is not None)
    for g_ in got:
        assert torch.isfinite(g_).all(), what

    def fn(*lv):
        lv = list(lv)
        xx = lv.pop(0) if x_grad else x.to(lv[0].dtype)
        o, al_ = level_ref(xx, rowptr, col, lv[0], lv[1], lv[2] if S is not None else None, SLOPE, concat,
                           *((mk["x"], mk["wh"], mk["att"]) if mk is not None else ()))
        return torch.cat([o.reshape(-1), al_.reshape(-1)])
    leaves64 = ([x] if x_grad else []) + [W, a] + ([S] if S is not None else [])
    names = (["dX"] if x_grad else []) + ["dW", "da"] + (["dW_skip"] if S is not None else [])
    rep, _ = parity.check_autograd(torch.cat([out.reshape(-1), al.reshape(-1)]), got, fn, [t.double() for t in leaves64],
                                   torch.cat([G.reshape(-1), A.reshape(-1)]), names, what)
    print(what, {k: f"{v:.2e}" for k, v in rep.items()})
    return got


# ----------------------------------------------------------------------------------------------------------------- lane shapes
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_lane_shapes(shape, concat, skip):
    H, Fo = shape
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[shape])
    _check(f"grad {shape} concat={concat} skip={skip}", rowptr, col, x, W, a, S if skip else None, concat)


@pytest.mark.parametrize("shape", [(3, 8), (6, 16)], ids=["3x8", "6x16"])
def test_heads_not_a_power_of_two(shape):
    """H does not divide 64: 63 / 60 working lanes per wave and the shuffle-loop sum of csrc/k14_alpha_grad.hip head_sum, in the
    wave-per-row launch and (hub rows of 699 edges) in the long-row launch."""
    H, Fo = shape
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=ODD_SEED[shape])
    _check(f"grad {shape}", rowptr, col, x, W, a, None, True)
    rowptr, col = _asym_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=ODD_SEED[shape])
    _check(f"grad asym {shape}", rowptr, col, x, W, a, S, False, nan_single=True)


@pytest.mark.parametrize("case", list(LONG_ROW_CASES))
def test_long_row_slots_and_chunks(case):
    """The long-row rule of csrc/long_rows.h beyond one hub: nine_hubs fills every slot of a chunk in the row and the column pass
    (3 x 8: the shuffle-loop head_sum inside the long launch), three_chunk_hub merges a row's records from three chunks.  Two runs
    give the same bits."""
    pattern, (H, Fo), seed = LONG_ROW_CASES[case]
    rowptr, col = pattern()
    x, W, a, _ = _params(len(rowptr) - 1, 48, H, Fo, seed=seed)
    runs = [_check(f"grad {case}", rowptr, col, x, W, a, None, True) for _ in range(2)]
    for u, v in zip(*runs):
        assert torch.equal(u, v)


@pytest.mark.parametrize("shape", [(1, 7), (8, 16), (4, 64)], ids=["1x7", "8x16", "4x64"])
def test_asymmetric_pattern(shape):
    H, Fo = shape
    rowptr, col = _asym_graph()
    x, W, a, _ = _params(len(rowptr) - 1, 32, H, Fo, seed=ASYM_SEED[shape])
    _check(f"grad asym {shape}", rowptr, col, x, W, a, None, True, nan_single=True)


# ------------------------------------------------------------------------------------------------- which output the loss uses
def _hub_case():
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, 8, 16, seed=LANE_SEED[(8, 16)])
    return rowptr, col, x, W, a, S


def test_alpha_only_loss():
    """G = 0, and a loss that never touches `out`: the same gradients, both right."""
    rowptr, col, x, W, a, S = _hub_case()
    graph = _graph(rowptr, col)
    _, A = _GA((1,), len(col), 8)
    (out, al), leaves = _run_level(graph, x, W, a, S, True)
    g0 = torch.autograd.grad([out, al], leaves, [torch.zeros_like(out), A.float().to(DEV)])
    (out, al), leaves = _run_level(graph, x, W, a, S, True)
    g1 = torch.autograd.grad((al * A.float().to(DEV)).sum(), leaves)
    for u, v in zip(g0, g1):
        assert torch.equal(u, v)

    def fn(x_, W_, a_, S_):
        return level_ref(x_, rowptr, col, W_, a_, S_, SLOPE, True)[1].reshape(-1)
    parity.check_autograd(al.reshape(-1), _stacked(g1, 8, True, True), fn, [t.double() for t in (x, W, a, S)], A.reshape(-1),
                          ["dX", "dW", "da", "dW_skip"], "alpha-only loss")
    assert float(_stacked(g1, 8, True, True)[3].abs().max()) == 0.0      # alpha does not depend on the skip projection


def test_out_only_loss_is_the_plain_backward(monkeypatch):
    """A loss on `out` alone in "grad" mode: the gradients of return_attention=False bit for bit, and the launch sequence of
    return_attention=True (nothing of K14 runs)."""
    from pygat_amd import ops
    rowptr, col, x, W, a, S = _hub_case()
    graph = _graph(rowptr, col)
    seen = []
    real = ops.lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("pygat_") or name in ("pygat_last_error", "pygat_head_group", "pygat_padded_width"):
                return fn

            def wrapped(*args):
                seen.append(name)
                return fn(*args)
            return wrapped
    monkeypatch.setattr(ops, "lib", Spy())
    res, seq = {}, {}
    for mode in (False, True, "grad"):
        seen.clear()
        r, leaves = _run_level(graph, x, W, a, S, True, mode=mode)
        out = r[0] if mode else r
        G, _ = _GA(tuple(out.shape), 1, 1)
        res[mode] = [out.detach()] + list(torch.autograd.grad(out, leaves, G.float().to(DEV)))
        seq[mode] = list(seen)
    for u, v in zip(res[False], res["grad"]):
        assert torch.equal(u, v)
    assert seq["grad"] == seq[True] and not any("alpha_grad" in s for s in seq["grad"])
    assert [s for s in seq[True] if s != "pygat_gat_attention"] == seq[False]


def test_values_equal_detached_and_deterministic():
    rowptr, col, x, W, a, S = _hub_case()
    graph = _graph(rowptr, col)
    (o1, a1), _ = _run_level(graph, x, W, a, None, True, mode=True)
    assert not a1.requires_grad
    runs = []
    for _ in range(2):
        (o2, a2), leaves = _run_level(graph, x, W, a, None, True)
        assert torch.equal(o1, o2.detach()) and torch.equal(a1, a2.detach())
        G, A = _GA(tuple(o2.shape), len(col), 8)
        runs.append(torch.autograd.grad([o2, a2], leaves, [G.float().to(DEV), A.float().to(DEV)]))
    for u, v in zip(*runs):
        assert torch.equal(u, v)
    (o3, a3), _ = _run_level(graph, x.detach(), W, a, None, True, x_grad=False)
    assert a3.requires_grad
    with torch.no_grad():      # (the inference forward: compared with the detached coefficients of the same forward)
        (_, a4), _ = _run_level(graph, x, W, a, None, True)
        (_, a5), _ = _run_level(graph, x, W, a, None, True, mode=True)
    assert not a4.requires_grad and torch.equal(a4, a5)


# --------------------------------------------------------------------------------------------------- renumbered and tail routes
@pytest.fixture(scope="module")
def iso():
    rowptr, col = _iso_csr(ROUTE_N, 0.55, 21)
    x, W, a, _ = _params(ROUTE_N, 128, 8, 16, seed=ROUTE_SEED)
    return rowptr, col, x, W, a


@pytest.mark.parametrize("fused", [True, False], ids=["tail_fused", "tail_stream"])
@pytest.mark.parametrize("route", ["level_renumbers", "internal_view", "degree_ordered"])
def test_routes(iso, route, fused, monkeypatch):
    _force(monkeypatch, fused)
    rowptr, col, x, W, a = iso
    graph = _graph(rowptr, col)
    if route == "level_renumbers":
        _check(f"grad {route}", rowptr, col, x, W, a, None, True, graph=graph, x_grad=False, nan_single=fused)
        return
    g2 = graph.internal_view() if route == "internal_view" else graph.degree_ordered()[0]
    to_user = graph.degree_ordered()[1].long().cpu()
    # the level sees the internal graph and x in internal order: alpha follows that graph's edges; a graph with a row map
    # (degree_ordered) writes `out` at the caller's rows
    _check(f"grad {route}", g2.fwd.rowptr.cpu().numpy(), g2.fwd.col.cpu().numpy(), x[to_user], W, a, None, True, graph=g2,
           x_grad=False, out_rows=to_user if route == "degree_ordered" else None)


# ------------------------------------------------------------------------------------------------------------------ the model
def _entropy(al):
    return -(al * torch.log(al.clamp_min(1e-30))).sum()


def test_two_level_model_entropy_penalty():
    import os
    import pygat_amd as pg
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "cora_csr.npz"))
    rowptr, col = d["rowptr"], d["col"]
    N, Fin = len(rowptr) - 1, 64
    torch.manual_seed(MODEL_SEED)
    model = pg.GAT(nfeat=[Fin, 8, 7], nheads=[8, 1], nlayers=2, dropout=0.0, alpha=SLOPE, layer_type=pg.SpGraphAttentionLayer).to(DEV)
    x = torch.randn(N, Fin, generator=torch.Generator().manual_seed(MODEL_SEED))
    heads1 = [getattr(model, f"attention_layer_1_head_{h}") for h in range(1, 9)]
    W1 = torch.stack([h.W.detach().cpu() for h in heads1]); a1 = torch.stack([h.a.detach().cpu().reshape(-1) for h in heads1])
    W2 = model.attention_layer_2_head_1.W.detach().cpu()[None]; a2 = model.attention_layer_2_head_1.a.detach().cpu().reshape(1, -1)
    with torch.no_grad():
        h1 = level_ref(x.double(), rowptr, col, W1.double(), a1.double(), None, SLOPE, True)[0]
    assert kink_count(x, rowptr, col, W1, a1, SLOPE) == 0 and kink_count(h1, rowptr, col, W2, a2, SLOPE) == 0, "choose another seed"
    graph = _graph(rowptr, col)
    out, alphas = model(x.to(DEV), graph, return_attention="grad")
    assert len(alphas) == 2 and all(al.requires_grad for al in alphas)
    G = torch.randn(out.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    lam = 0.1
    loss = (out * G.float().to(DEV)).sum() + lam * (_entropy(alphas[0]) + _entropy(alphas[1]))
    loss.backward()
    got = [torch.stack([h.W.grad for h in heads1]), torch.stack([h.a.grad.reshape(-1) for h in heads1]),
           model.attention_layer_2_head_1.W.grad[None], model.attention_layer_2_head_1.a.grad.reshape(1, -1)]

    def fn(W1_, a1_, W2_, a2_):
        xx = x.to(W1_.dtype)
        h, al1 = level_ref(xx, rowptr, col, W1_, a1_, None, SLOPE, True)
        o, al2 = level_ref(h, rowptr, col, W2_, a2_, None, SLOPE, False)
        return torch.cat([o.reshape(-1), _entropy(al1)[None], _entropy(al2)[None]])
    got_y = torch.cat([out.detach().reshape(-1), _entropy(alphas[0].detach())[None], _entropy(alphas[1].detach())[None]])
    rep, _ = parity.check_autograd(got_y, got, fn, [t.double() for t in (W1, a1, W2, a2)],
                                   torch.cat([G.reshape(-1), torch.tensor([lam, lam], dtype=torch.float64)]),
                                   ["dW1", "da1", "dW2", "da2"], "model + entropy penalty")
    print(rep)


@pytest.mark.parametrize("fused", [True, False], ids=["tail_fused", "tail_stream"])
def test_two_level_model_internal_order(fused, monkeypatch):
    """The model runs on internal_view(): every level's AttentionTarget carries order = (caller graph, to_internal), and the
    incoming gradient of alpha is in the caller's edge order like alpha itself."""
    import pygat_amd as pg
    _force(monkeypatch, fused)
    rowptr, col = _iso_csr(ROUTE_N, 0.55, 23)
    torch.manual_seed(MODEL_INT_SEED)
    model = pg.GAT(nfeat=[64, 16, 6], nheads=[8, 1], nlayers=2, dropout=0.5, alpha=SLOPE, layer_type=pg.SpGraphAttentionLayer).to(DEV).eval()
    x = torch.randn(ROUTE_N, 64, generator=torch.Generator().manual_seed(MODEL_INT_SEED))
    graph = _graph(rowptr, col)
    assert model._internal_order_pays(torch.zeros(ROUTE_N, 64, device=DEV), graph, 0.0)
    heads1 = [getattr(model, f"attention_layer_1_head_{h}") for h in range(1, 9)]
    W1 = torch.stack([h.W.detach().cpu() for h in heads1]); a1 = torch.stack([h.a.detach().cpu().reshape(-1) for h in heads1])
    W2 = model.attention_layer_2_head_1.W.detach().cpu()[None]; a2 = model.attention_layer_2_head_1.a.detach().cpu().reshape(1, -1)
    with torch.no_grad():
        h1 = level_ref(x.double(), rowptr, col, W1.double(), a1.double(), None, SLOPE, True)[0]
    assert kink_count(x, rowptr, col, W1, a1, SLOPE) == 0 and kink_count(h1, rowptr, col, W2, a2, SLOPE) == 0, "choose another seed"
    out, alphas = model(x.to(DEV), graph, return_attention="grad")
    with torch.no_grad():
        _, detached = model(x.to(DEV), graph, return_attention=True)
    assert all(al.requires_grad for al in alphas) and alphas[0].shape == (len(col), 8) and alphas[1].shape == (len(col), 1)
    G, A1 = _GA(tuple(out.shape), len(col), 8)
    _, A2 = _GA((1,), len(col), 1, seed=6)
    torch.autograd.backward([out, alphas[0], alphas[1]], [t.float().to(DEV) for t in (G, A1, A2)])
    got = [torch.stack([h.W.grad for h in heads1]), torch.stack([h.a.grad.reshape(-1) for h in heads1]),
           model.attention_layer_2_head_1.W.grad[None], model.attention_layer_2_head_1.a.grad.reshape(1, -1)]

    def fn(W1_, a1_, W2_, a2_):
        h, al1 = level_ref(x.to(W1_.dtype), rowptr, col, W1_, a1_, None, SLOPE, True)
        o, al2 = level_ref(h, rowptr, col, W2_, a2_, None, SLOPE, False)
        return torch.cat([o.reshape(-1), al1.reshape(-1), al2.reshape(-1)])
    rep, _ = parity.check_autograd(torch.cat([out.detach().reshape(-1)] + [al.detach().reshape(-1) for al in alphas]), got, fn,
                                   [t.double() for t in (W1, a1, W2, a2)], torch.cat([t.reshape(-1) for t in (G, A1, A2)]),
                                   ["dW1", "da1", "dW2", "da2"], "model on internal_view")
    print(rep)


# ---------------------------------------------------------------------------------------------- dropout level, sparse features
def test_dropout_level_explicit_masks():
    from pygat_amd.dropout import draw_masks, gat_level_dropout
    rowptr, col = _hub_graph(seed=8)
    N, Fin, H, Fo, p = len(rowptr) - 1, 32, 8, 8, 0.6
    x, W, a, S = _params(N, Fin, H, Fo, seed=DROPOUT_SEED)
    masks = draw_masks(p, H, N, Fin, Fo, len(col), "cpu", generator=torch.Generator().manual_seed(3))
    masks = {k: v.to(DEV) for k, v in masks.items()}

    def level(xd, graph, Ws, As, Ss, slope, concat, return_attention):
        return gat_level_dropout(xd, graph, Ws, As, Ss, slope, concat, p, masks=masks, return_attention=return_attention)
    _check("grad dropout masks", rowptr, col, x, W, a, None, True, masks=masks, fn=level)
    _check("grad dropout masks, skip, mean", rowptr, col, x, W, a, S, False, masks=masks, fn=level)


def test_dropout_level_seeded_runs():
    """In-kernel masks from a seed (the same seed = the same masks): the backward is linear in A = dL/d alpha, A moves every
    gradient, and a loss on `out` alone is the run without the coefficients bit for bit."""
    from pygat_amd.dropout import gat_level_dropout
    rowptr, col, x, W, a, _ = _hub_case()
    graph = _graph(rowptr, col)

    def run(scale, mode="grad"):
        xd, Ws, As, _ = _leaves(x, W, a, None)
        r = gat_level_dropout(xd, graph, Ws, As, None, SLOPE, True, 0.6, generator=torch.Generator(device=DEV).manual_seed(1),
                              return_attention=mode)
        out = r[0] if mode else r
        G, A = _GA(tuple(out.shape), len(col), 8)
        if scale is None:
            return out.detach(), torch.autograd.grad(out, [xd] + Ws + As, G.float().to(DEV))
        assert r[1].requires_grad
        return out.detach(), torch.autograd.grad([out, r[1]], [xd] + Ws + As, [G.float().to(DEV), (scale * A).float().to(DEV)])
    o0, g0 = run(0.0)
    o1, g1 = run(1.0)
    o2, g2 = run(2.0)
    op, gp = run(None, mode=False)
    on, gn = run(None)
    assert torch.equal(o0, o1) and torch.equal(o0, op)
    for u, v, w in zip(gp, gn, g0):
        assert torch.equal(u, v)                       # no incoming alpha gradient: the plain backward
        assert parity.err(w, u) <= 1e-6 * max(1.0, float(u.abs().max()))     # A = 0 adds exact zeros (up to the sign of a zero)
    for k, (u0, u1, u2) in enumerate(zip(g0, g1, g2)):
        assert torch.isfinite(u1).all()
        d1, d2 = (u1 - u0).double(), (u2 - u1).double()
        scale = float(d1.abs().max())
        assert scale > 1e-3 * max(1.0, float(u0.abs().max())), (k, "A does not reach this gradient")
        assert float((d2 - d1).abs().max()) <= 1e-3 * scale + 1e-5, (k, "not linear in A")


def test_sparse_first_level_features():
    from pygat_amd.features import prepare_features
    rowptr, col = _hub_graph()
    N, Fin, H, Fo = len(rowptr) - 1, 256, 8, 16
    x, W, a, S = _params(N, Fin, H, Fo, seed=SPARSE_SEED)
    x = x * (torch.rand(N, Fin, generator=torch.Generator().manual_seed(SPARSE_SEED)) < 0.05)

    def level(x_, graph, Ws, As, Ss, slope, concat, return_attention):
        import pygat_amd as pg
        xs = prepare_features(x_)
        assert xs is not None
        return pg.gat_level(x_, graph, Ws, As, Ss, slope, concat, xs=xs, return_attention=return_attention)
    _check("grad sparse x", rowptr, col, x, W, a, S, True, x_grad=False, fn=level)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import pygat_amd as pg
    from pygat_amd import gatv2
    from pygat_amd.dist import gat_level_head_parallel
    from pygat_amd.graphed import FusedEpoch, GraphedLevel
    rowptr, col = _hub_graph(N=200, seed=2)
    graph = _graph(rowptr, col)
    x, W, a, _ = _params(200, 16, 2, 8, seed=2)
    xd = x.to(DEV)
    Ws, As = [W[h].to(DEV) for h in range(2)], [a[h].to(DEV) for h in range(2)]
    W2, a2 = [torch.cat([w, w]) for w in Ws], [v[:8].contiguous() for v in As]
    with pytest.raises(ValueError, match="grad"):
        gatv2.gatv2_level(xd, graph, W2, a2, None, SLOPE, True, return_attention="grad")
    assert len(gatv2.gatv2_level(xd, graph, W2, a2, None, SLOPE, True, return_attention=True)) == 2
    adj = torch.zeros(200, 200, device=DEV)
    adj[src_of(rowptr).to(DEV), torch.as_tensor(col, dtype=torch.int64, device=DEV)] = 1.0
    for cls in (gatv2.SpGraphAttentionLayerV2, gatv2.GraphAttentionLayerV2):
        layer = cls(16, 8, dropout=0.0, alpha=SLOPE).to(DEV)
        with pytest.raises(ValueError, match="grad"):
            layer(xd, adj, return_attention="grad")
        assert len(layer(xd, adj, return_attention=True)) == 2
    many = 65
    with pytest.raises(ValueError, match="at most 64 heads"):      # refused in the forward, not by the launcher in the backward
        pg.gat_level(xd, graph, [Ws[0]] * many, [As[0]] * many, None, SLOPE, True, return_attention="grad")
    with pytest.raises(ValueError, match="False, True or"):
        pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, return_attention="yes")
    with pytest.raises(ValueError, match="return_attention"):
        pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, pipeline=(2, lambda *a_: None), return_attention="grad")
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.0, alpha=SLOPE, head_parallel=True).to(DEV)
    with pytest.raises(ValueError, match="return_attention"):
        model(xd, graph, return_attention="grad")
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.0, alpha=SLOPE, layer_type=gatv2.SpGraphAttentionLayerV2).to(DEV)
    with pytest.raises(ValueError, match="grad"):
        model(xd, graph, return_attention="grad")
    with pytest.raises(ValueError, match="return_attention"):
        gat_level_head_parallel(xd, graph, Ws, As, None, SLOPE, True, return_attention="grad")
    gl = GraphedLevel(graph, xd, W.to(DEV), a.to(DEV), warmup=1)
    with pytest.raises(ValueError, match="return_attention"):
        gl.forward(return_attention="grad")
    with pytest.raises(ValueError, match="return_attention"):
        FusedEpoch.run(object.__new__(FusedEpoch), return_attention="grad")
    # the layer classes of the GAT (v1) level take it
    layer = pg.SpGraphAttentionLayer(16, 8, dropout=0.0, alpha=SLOPE).to(DEV)
    out, al = layer(xd, adj, return_attention="grad")
    assert al.requires_grad and al.shape == (len(col), 1)
    torch.autograd.grad(al.square().sum(), [layer.W, layer.a])


def test_new_kernels_have_no_scratch():
    import ctypes as C
    from pygat_amd._lib import lib
    for name in ("k14_rows_long", "k14_cols_long", "k14_rows_wave", "k14_cols_wave", "k14_apply"):
        regs, scratch = C.c_int(-1), C.c_int(-1)
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and 0 < regs.value <= 64, (name, regs.value, scratch.value)
