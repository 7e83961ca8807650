"""gat_level(..., edge_logit=u): a per-edge term in the attention logit, z_ij = s_i + t_j + u_ij, and its gradient du_ij = dz_ij
(csrc/k15_edge_logit.hip).

Ground truth is torch autograd in fp64 on the CPU through edge_logit_case.level_ref (alpha_grad_case.level_ref with the u term),
u a leaf.  Loss L = <out, G>, G ~ N(0, 1), seeded; u ~ 0.5 N(0, 1), seeded.  Pricing is parity.check_autograd: `out` and alpha by
close_fwd, dX / dW / da / dW_skip / du by close_grad, i.e. max(1e-5, 4 x the fp32 run's own error).  check_autograd has no
treatment of the LeakyReLU kink, so every case asserts, on its fp64 run, that NO (edge, head) has a logit in the rounding band
|z| <= parity.KINK_TAU (|s_i| + |t_j| + |u_ij|); the seeds below were chosen on the CPU so that this holds."""
import os

import numpy as np
import pytest
import torch

import parity
from alpha_grad_case import kink_count as plain_kink_count
from alpha_grad_case import level_ref as plain_ref
from alpha_grad_case import src_of
from edge_logit_case import edge_logits, kink_count, level_ref
from long_row_cases import nine_hubs, three_chunk_hub
from pattern_device import DEV, _graph
from pattern_graphs import SHAPES, SID, SLOPE, _asym_graph, _hub_graph, _params

pytestmark = pytest.mark.gpu

# seeds of _params / edge_logits per case: the first from the case's base seed on whose fp64 run no logit lies in the kink band
LANE_SEED = {(1, 7): 107, (8, 8): 808, (8, 16): 816, (4, 64): 465, (4, 256): 658, (16, 64): 1664}
ODD_SEED = {(3, 8): 308, (6, 16): 616}
ODD_ASYM_SEED = {(3, 8): 308, (6, 16): 616}
ASYM_SEED = {(1, 7): 7, (8, 16): 7, (4, 64): 7}
ZERO_SEED, MASK_SEED, MODEL_SEED = 816, 816, 5
# pattern, (H, F'), concat, skip, seed
LONG_ROW_CASES = {"nine_hubs-8x16-concat": (nine_hubs, (8, 16), True, False, 816), "nine_hubs-4x64-mean-skip": (nine_hubs, (4, 64), False, True, 464),
                  "three_chunk_hub-8x16-concat": (three_chunk_hub, (8, 16), True, False, 816)}


def _leaves(x, W, a, S, u, x_grad=True):
    H = W.shape[0]
    xd = x.to(DEV).requires_grad_(x_grad)
    Ws = [W[h].to(DEV).requires_grad_(True) for h in range(H)]
    As = [a[h].to(DEV).requires_grad_(True) for h in range(H)]
    Ss = None if S is None else [S[h].to(DEV).requires_grad_(True) for h in range(H)]
    return xd, Ws, As, Ss, u.to(DEV).requires_grad_(True)


def _stacked(grads, H, x_grad, skip):
    """autograd.grad's flat tuple -> [dX?, dW [H,..], da [H,..], dW_skip?, du]"""
    g = list(grads)
    out = [g.pop(0)] if x_grad else []
    out.append(torch.stack(g[:H])); out.append(torch.stack([v.reshape(-1) for v in g[H:2 * H]]))
    if skip:
        out.append(torch.stack(g[2 * H:3 * H]))
    out.append(g[-1])
    return out


def _G(shape, seed=5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _run(graph, x, W, a, S, u, concat, x_grad=True, ra=False):
    import pygat_amd as pg
    xd, Ws, As, Ss, ud = _leaves(x, W, a, S, u, x_grad)
    r = pg.gat_level(xd, graph, Ws, As, Ss, SLOPE, concat, edge_logit=ud, return_attention=ra)
    return r, ([xd] if x_grad else []) + Ws + As + (Ss or []) + [ud]


def _check(what, rowptr, col, x, W, a, S, u, concat, graph=None, x_grad=True, ra=False, u_dev=None):
    """One level with the edge term against level_ref; u_dev: what the device sees when it differs from the oracle's u (NaN rows).
    -> (the HIP gradients, out, alpha | None)."""
    H = W.shape[0]
    assert kink_count(x, rowptr, col, W, a, u, SLOPE) == 0, f"{what}: an input with a logit inside the kink band -- choose another seed"
    graph = graph if graph is not None else _graph(rowptr, col)
    r, leaves = _run(graph, x, W, a, S, u if u_dev is None else u_dev, concat, x_grad, ra)
    out, al = r if ra else (r, None)
    if ra:
        assert not al.requires_grad and al.shape == (len(col), H) and al.dtype == torch.float32
    G = _G(tuple(out.shape))
    grads = torch.autograd.grad(out, leaves, G.float().to(DEV))
    got = _stacked(grads, H, x_grad, S is not None)
    for g_ in got:
        assert torch.isfinite(g_).all(), what
    assert torch.isfinite(out).all(), what

    def fn(*lv):
        lv = list(lv)
        xx = lv.pop(0) if x_grad else x.to(lv[0].dtype)
        o, al_ = level_ref(xx, rowptr, col, lv[0], lv[1], lv[2] if S is not None else None, SLOPE, concat, lv[-1])
        return torch.cat([o.reshape(-1), al_.reshape(-1)]) if ra else o.reshape(-1)
    leaves64 = ([x] if x_grad else []) + [W, a] + ([S] if S is not None else []) + [u]
    names = (["dX"] if x_grad else []) + ["dW", "da"] + (["dW_skip"] if S is not None else []) + ["du"]
    got_y = torch.cat([out.reshape(-1), al.reshape(-1)]) if ra else out.reshape(-1)
    G64 = torch.cat([G.reshape(-1), torch.zeros(len(col) * H, dtype=torch.float64)]) if ra else G.reshape(-1)
    rep, _ = parity.check_autograd(got_y.detach(), got, fn, [t.double() for t in leaves64], G64, names, what)
    print(what, {k: f"{v:.2e}" for k, v in rep.items()})
    return got, out.detach(), al


def _single_rows(rowptr):
    return (torch.as_tensor(np.diff(np.asarray(rowptr))) == 1)[src_of(rowptr)]


# ----------------------------------------------------------------------------------------------------------------- lane shapes
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("shape", SHAPES, ids=SID)
def test_lane_shapes(shape, concat, skip):
    """Hub rows of 699 edges: the long-row launch and its partial records, in all three passes (the pattern is symmetric)."""
    H, Fo = shape
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[shape])
    u = edge_logits(len(col), H, LANE_SEED[shape] + 1)
    _check(f"edge {shape} concat={concat} skip={skip}", rowptr, col, x, W, a, S if skip else None, u, concat)


@pytest.mark.parametrize("shape", [(3, 8), (6, 16)], ids=["3x8", "6x16"])
def test_heads_that_do_not_divide_64(shape):
    """Lane groups with idle lanes (6 of 8, 24 of 32 chunks)."""
    H, Fo = shape
    rowptr, col = _hub_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=ODD_SEED[shape])
    _check(f"edge {shape}", rowptr, col, x, W, a, None, edge_logits(len(col), H, ODD_SEED[shape] + 1), True)
    rowptr, col = _asym_graph()
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=ODD_ASYM_SEED[shape])
    _check(f"edge asym {shape}", rowptr, col, x, W, a, S, edge_logits(len(col), H, ODD_ASYM_SEED[shape] + 1), False)


@pytest.mark.parametrize("case", list(LONG_ROW_CASES))
def test_long_row_slots_and_chunks(case):
    """The long-row rule of csrc/long_rows.h beyond one hub, in all three passes (both patterns are symmetric): nine_hubs fills
    every slot of a chunk, three_chunk_hub merges a row's records from three chunks.  Two runs give the same bits."""
    pattern, (H, Fo), concat, skip, seed = LONG_ROW_CASES[case]
    rowptr, col = pattern()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=seed)
    u = edge_logits(len(col), H, seed + 1)
    runs = [_check(f"edge {case}", rowptr, col, x, W, a, S if skip else None, u, concat, graph=graph) for _ in range(2)]
    (g1, o1, _), (g2, o2, _) = runs
    assert torch.equal(o1, o2)
    for p, q in zip(g1, g2):
        assert torch.equal(p, q)


@pytest.mark.parametrize("shape", [(1, 7), (8, 16), (4, 64)], ids=["1x7", "8x16", "4x64"])
def test_asymmetric_pattern(shape):
    """The explicit transpose with perm_t addressing u and du; the u rows of single-edge rows are never read (NaN there) and their
    du is exactly 0."""
    H, Fo = shape
    rowptr, col = _asym_graph()
    graph = _graph(rowptr, col)
    assert not graph.symmetric and graph.bwd is not graph.fwd
    x, W, a, _ = _params(len(rowptr) - 1, 32, H, Fo, seed=ASYM_SEED[shape])
    u = edge_logits(len(col), H, ASYM_SEED[shape] + 1)
    single = _single_rows(rowptr)
    assert int(single.sum()) > 0
    u[single] = 0.0                      # (the oracle's value there is immaterial: alpha = 1)
    u_dev = u.clone()
    u_dev[single] = float("nan")
    got, out, al = _check(f"edge asym {shape}", rowptr, col, x, W, a, None, u, True, graph=graph, ra=True, u_dev=u_dev)
    assert float(got[-1][single.to(DEV)].abs().max()) == 0.0
    assert (al[single.to(DEV)] == 1.0).all()


# ------------------------------------------------------------------------------------------------------------- broadcast forms
def test_broadcast_forms():
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[(8, 16)])
    u1 = edge_logits(len(col), 1, LANE_SEED[(8, 16)] + 1)
    full = u1.expand(-1, H).contiguous()
    got, out, _ = _check("edge broadcast, expanded", rowptr, col, x, W, a, S, full, True, graph=graph)
    G = _G(tuple(out.shape)).float().to(DEV)
    for form in (u1, u1[:, 0].contiguous()):
        r, leaves = _run(graph, x, W, a, S, form, True)
        assert torch.equal(r.detach(), out)
        g = _stacked(torch.autograd.grad(r, leaves, G), H, True, True)
        for p, q in zip(g[:-1], got[:-1]):
            assert torch.equal(p, q)
        assert g[-1].shape == form.shape

        def fn(u_):
            return level_ref(x.double(), rowptr, col, W.double(), a.double(), S.double(), SLOPE, True,
                             u_.reshape(-1, 1).expand(-1, H))[0].reshape(-1)
        parity.check_autograd(r.detach().reshape(-1), [g[-1]], fn, [form.double()], _G(tuple(out.shape)).reshape(-1), ["du (head sum)"],
                              f"edge broadcast {tuple(form.shape)}")


# -------------------------------------------------------------------------------------------------------------------- u = 0
def test_zero_logit_is_the_plain_level():
    import pygat_amd as pg
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=ZERO_SEED)
    u = torch.zeros(len(col), H)
    got, out, _ = _check("edge u=0", rowptr, col, x, W, a, S, u, True, graph=graph)      # (du against the fp64 dz)
    # the plain level, priced against the same fp64 truth
    xd, Ws, As, Ss, _ = _leaves(x, W, a, S, u)
    o2 = pg.gat_level(xd, graph, Ws, As, Ss, SLOPE, True)
    G = _G(tuple(o2.shape))
    g2 = _stacked(list(torch.autograd.grad(o2, [xd] + Ws + As + Ss, G.float().to(DEV))) + [None], H, True, True)[:-1]

    def fn(x_, W_, a_, S_):
        return level_ref(x_, rowptr, col, W_, a_, S_, SLOPE, True, u.to(x_.dtype))[0].reshape(-1)
    for res, o in ((got[:-1], out), (g2, o2.detach())):
        parity.check_autograd(o.reshape(-1), res, fn, [t.double() for t in (x, W, a, S)], G.reshape(-1),
                              ["dX", "dW", "da", "dW_skip"], "u=0 against the plain truth")


# ------------------------------------------------------------------------------------------------------------ soft edge mask
def test_soft_edge_mask_prunes_the_pattern():
    import pygat_amd as pg
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    N = len(rowptr) - 1
    src = src_of(rowptr).numpy()
    c = np.asarray(col, dtype=np.int64)
    key = np.minimum(src, c) * N + np.maximum(src, c)
    uniq, inv = np.unique(key, return_inverse=True)
    masked = (np.random.default_rng(MASK_SEED).random(len(uniq)) < 0.3)[inv] & (src != c)      # mirrored: the pattern stays symmetric
    assert 0.2 < masked.mean() < 0.4
    keep = ~masked
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(src[keep], minlength=N))]).astype(np.int32)
    col2 = np.asarray(col)[keep].astype(np.int32)
    x, W, a, _ = _params(N, 48, H, Fo, seed=MASK_SEED)
    assert plain_kink_count(x, rp2, col2, W, a, SLOPE) == 0, "choose another seed"
    mt = torch.as_tensor(masked)
    u = torch.zeros(len(col), H)
    u[mt] = -1e4
    (out, al), leaves = _run(_graph(rowptr, col), x, W, a, None, u, True, ra=True)
    G = _G(tuple(out.shape))
    got = _stacked(torch.autograd.grad(out, leaves, G.float().to(DEV)), H, True, False)
    assert float(al[mt.to(DEV)].abs().max()) == 0.0
    assert float(got[-1][mt.to(DEV)].abs().max()) == 0.0

    def fn(x_, W_, a_):
        return plain_ref(x_, rp2, col2, W_, a_, None, SLOPE, True)[0].reshape(-1)
    parity.check_autograd(out.detach().reshape(-1), got[:-1], fn, [t.double() for t in (x, W, a)], G.reshape(-1), ["dX", "dW", "da"],
                          "soft mask against the pruned pattern")
    xd, Ws, As, _, _ = _leaves(x, W, a, None, u)
    o2 = pg.gat_level(xd, _graph(rp2, col2), Ws, As, None, SLOPE, True)
    g2 = _stacked(list(torch.autograd.grad(o2, [xd] + Ws + As, G.float().to(DEV))) + [None], H, True, False)[:-1]
    parity.check_autograd(o2.detach().reshape(-1), g2, fn, [t.double() for t in (x, W, a)], G.reshape(-1), ["dX", "dW", "da"],
                          "the plain level on the pruned pattern")


# ------------------------------------------------------------------------------------------------------------------ the model
def test_learned_edge_term_two_level_model():
    import pygat_amd as pg
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "cora_csr.npz"))
    rowptr, col = d["rowptr"], d["col"]
    N, Fin, E = len(rowptr) - 1, 64, len(d["col"])
    torch.manual_seed(MODEL_SEED)
    model = pg.GAT(nfeat=[Fin, 8, 7], nheads=[8, 1], nlayers=2, dropout=0.0, alpha=SLOPE, layer_type=pg.SpGraphAttentionLayer).to(DEV)
    g = torch.Generator().manual_seed(MODEL_SEED)
    x = torch.randn(N, Fin, generator=g)
    attr = torch.randn(E, 4, generator=g)
    We1, We2 = 0.25 * torch.randn(4, 8, generator=g), 0.25 * torch.randn(4, 1, generator=g)
    heads1 = [getattr(model, f"attention_layer_1_head_{h}") for h in range(1, 9)]
    W1 = torch.stack([h.W.detach().cpu() for h in heads1]); a1 = torch.stack([h.a.detach().cpu().reshape(-1) for h in heads1])
    W2 = model.attention_layer_2_head_1.W.detach().cpu()[None]; a2 = model.attention_layer_2_head_1.a.detach().cpu().reshape(1, -1)
    with torch.no_grad():
        h1 = level_ref(x.double(), rowptr, col, W1.double(), a1.double(), None, SLOPE, True, (attr @ We1).double())[0]
    assert kink_count(x, rowptr, col, W1, a1, attr @ We1, SLOPE) == 0 and kink_count(h1, rowptr, col, W2, a2, attr @ We2, SLOPE) == 0, \
        "choose another seed"
    graph = _graph(rowptr, col)
    We1d, We2d = We1.to(DEV).requires_grad_(True), We2.to(DEV).requires_grad_(True)
    attr_d = attr.to(DEV)
    out = model(x.to(DEV), graph, edge_logits=[attr_d @ We1d, attr_d @ We2d])
    G = _G(tuple(out.shape), seed=2)
    (out * G.float().to(DEV)).sum().backward()
    got = [torch.stack([h.W.grad for h in heads1]), torch.stack([h.a.grad.reshape(-1) for h in heads1]),
           model.attention_layer_2_head_1.W.grad[None], model.attention_layer_2_head_1.a.grad.reshape(1, -1), We1d.grad, We2d.grad]

    def fn(W1_, a1_, W2_, a2_, E1_, E2_):
        xx, at = x.to(W1_.dtype), attr.to(W1_.dtype)
        h, _ = level_ref(xx, rowptr, col, W1_, a1_, None, SLOPE, True, at @ E1_)
        return level_ref(h, rowptr, col, W2_, a2_, None, SLOPE, False, at @ E2_)[0].reshape(-1)
    rep, _ = parity.check_autograd(out.detach().reshape(-1), got, fn, [t.double() for t in (W1, a1, W2, a2, We1, We2)], G.reshape(-1),
                                   ["dW1", "da1", "dW2", "da2", "dWe1", "dWe2"], "model with learned edge terms")
    print(rep)


# ------------------------------------------------------------------------------------------------------------ attention export
def test_attention_export():
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[(8, 16)])
    u = edge_logits(len(col), H, LANE_SEED[(8, 16)] + 1)
    _, out, al = _check("edge attention export", rowptr, col, x, W, a, S, u, True, graph=graph, ra=True)
    sums = torch.zeros(len(rowptr) - 1, H, dtype=torch.float64).index_add(0, src_of(rowptr), al.double().cpu())
    assert float((sums - 1).abs().max()) <= 1e-6
    r, _ = _run(graph, x, W, a, S, u, True)
    assert torch.equal(r.detach(), out)


# -------------------------------------------------------------------------------------------------- determinism and isolation
def test_two_runs_are_bit_equal():
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[(8, 16)])
    u = edge_logits(len(col), H, 3)
    runs = []
    for _ in range(2):
        out, leaves = _run(graph, x, W, a, S, u, True)
        runs.append([out.detach()] + list(torch.autograd.grad(out, leaves, _G(tuple(out.shape)).float().to(DEV))))
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_call_sequences(monkeypatch):
    """edge_logit=None: the launches of the call without the argument, none of them K15's; with edge_logit: neither K2 nor K4."""
    import pygat_amd as pg
    from pygat_amd import ops
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = _params(len(rowptr) - 1, 48, H, Fo, seed=LANE_SEED[(8, 16)])
    u = edge_logits(len(col), H, 3)
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
    seq = {}
    for key, kw in (("absent", {}), ("none", {"edge_logit": None}), ("given", {"edge_logit": u.to(DEV)})):
        seen.clear()
        xd, Ws, As, Ss, _ = _leaves(x, W, a, S, u)
        out = pg.gat_level(xd, graph, Ws, As, Ss, SLOPE, True, **kw)
        torch.autograd.grad(out, [xd] + Ws + As + Ss, _G(tuple(out.shape)).float().to(DEV))
        seq[key] = list(seen)
    print(seq["none"])
    assert seq["none"] == seq["absent"] and not any("gat_edge" in s for s in seq["none"])
    # the plain level on a small symmetric graph, a loss on `out`: projection, K2, K3a, K4, da, dW, dW_skip, dX
    plain = ["pygat_pack_params_heads", "pygat_project_blocked", "pygat_gat_forward", "pygat_gat_backward_prepare", "pygat_gat_backward_col"]
    assert [s for s in seq["none"] if s in plain] == plain
    assert "pygat_gat_edge_forward" in seq["given"] and "pygat_gat_edge_backward_rows" in seq["given"] \
        and "pygat_gat_edge_backward_cols" in seq["given"]
    assert not any(s in ("pygat_gat_forward", "pygat_gat_backward_col") for s in seq["given"])


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import pygat_amd as pg
    from pygat_amd import gatv2, ops
    from pygat_amd.dist import gat_level_head_parallel
    from pygat_amd.dropout import gat_level_dropout
    from pygat_amd.graphed import GraphedLevel
    rowptr, col = _hub_graph(N=200, seed=2)
    graph = _graph(rowptr, col)
    x, W, a, _ = _params(200, 16, 2, 8, seed=2)
    xd = x.to(DEV)
    Ws, As = [W[h].to(DEV) for h in range(2)], [a[h].to(DEV) for h in range(2)]
    u = edge_logits(len(col), 2, 1).to(DEV)
    lvl = lambda **kw: pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, edge_logit=u, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="edge_logit.*pipeline"):
        lvl(pipeline=(2, lambda *a_: None))
    with pytest.raises(ValueError, match="edge_logit.*xs"):
        lvl(xs=object())
    with pytest.raises(ValueError, match="edge_logit.*attention_order"):
        lvl(return_attention=True, attention_order=(graph, None))
    with pytest.raises(ValueError, match="edge_logit.*grad"):
        lvl(return_attention="grad")
    with pytest.raises(ValueError, match="edge_logit.*bwd_heads"):
        ops._edge_logit_level(xd, graph, Ws, As, None, SLOPE, True, u, False, None, None, None, bwd_heads=(0, 1))
    with pytest.raises(ValueError, match="edge_logit"):
        pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, edge_logit=u[:-1])
    with pytest.raises(ValueError, match="edge_logit"):
        pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, edge_logit=torch.zeros(len(col), 3, device=DEV))
    for g2 in (graph.internal_view(), graph.degree_ordered()[0]):
        with pytest.raises(ValueError, match="edge_logit"):
            pg.gat_level(xd, g2, Ws, As, None, SLOPE, True, edge_logit=u)
    with pytest.raises(ValueError, match="edge_logit"):
        gat_level_head_parallel(xd, graph, Ws, As, None, SLOPE, True, edge_logit=u)
    with pytest.raises(ValueError, match="edge_logit"):
        gat_level_dropout(xd, graph, Ws, As, None, SLOPE, True, 0.5, edge_logit=u)
    gl = GraphedLevel(graph, xd, W.to(DEV), a.to(DEV), warmup=1)
    with pytest.raises(ValueError, match="edge_logit"):
        gl.forward(edge_logit=u)
    W2, a2 = [torch.cat([w, w]) for w in Ws], [v[:8].contiguous() for v in As]
    with pytest.raises(ValueError, match="edge_logit"):
        gatv2.gatv2_level(xd, graph, W2, a2, None, SLOPE, True, edge_logit=u)
    adj = torch.zeros(200, 200, device=DEV)
    adj[src_of(rowptr).to(DEV), torch.as_tensor(col, dtype=torch.int64, device=DEV)] = 1.0
    for cls in (gatv2.SpGraphAttentionLayerV2, gatv2.GraphAttentionLayerV2):
        layer = cls(16, 8, dropout=0.0, alpha=SLOPE).to(DEV)
        with pytest.raises(ValueError, match="edge_logit"):
            layer(xd, adj, edge_logit=u[:, :1])
    us = [u, u[:, :1]]
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.0, alpha=SLOPE, head_parallel=True).to(DEV)
    with pytest.raises(ValueError, match="edge_logits"):
        model(xd, graph, edge_logits=us)
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.0, alpha=SLOPE, layer_type=gatv2.SpGraphAttentionLayerV2).to(DEV)
    with pytest.raises(ValueError, match="edge_logits"):
        model(xd, graph, edge_logits=us)
    model = pg.GAT(nfeat=[16, 8, 3], nheads=[2, 1], nlayers=2, dropout=0.5, alpha=SLOPE, layer_type=pg.SpGraphAttentionLayer).to(DEV)
    with pytest.raises(ValueError, match="edge_logits"):
        model.train()(xd, graph, edge_logits=us)
    with pytest.raises(ValueError, match="edge_logit.*grad"):
        model.eval()(xd, graph, edge_logits=us, return_attention="grad")
    # what is taken: the layer classes of the v1 level, a None entry per level, the detached coefficients
    out, alphas = model.eval()(xd, graph, edge_logits=[None, u[:, 0]], return_attention=True)
    assert out.shape == (200, 3) and alphas[1].shape == (len(col), 1)
    layer = pg.SpGraphAttentionLayer(16, 8, dropout=0.0, alpha=SLOPE).to(DEV)
    ul = u[:, :1].clone().requires_grad_(True)
    out, al = layer(xd, adj, return_attention=True, edge_logit=ul)
    assert al.shape == (len(col), 1) and not al.requires_grad
    assert torch.autograd.grad(out.sum(), ul)[0].shape == ul.shape


def _k15_names():
    names = ["k15_att"]
    for op in ("fwd", "rows", "cols"):
        for kind in ("long", "row"):
            names += [f"k15_{op}_{kind}_l{lpr}v1" for lpr in (1, 2, 4, 8, 16, 32, 64)] + [f"k15_{op}_{kind}_l64v{v}" for v in (2, 3, 4)]
    return names


def test_new_kernels_have_no_scratch():
    import ctypes as C
    from pygat_amd._lib import lib
    for name in _k15_names():
        regs, scratch = C.c_int(-1), C.c_int(-1)
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and 0 < regs.value <= 128, (name, regs.value, scratch.value)
    assert lib.pygat_kernel_footprint(b"k15_fwd_row_l3v1", C.byref(regs), C.byref(scratch)) == -1
