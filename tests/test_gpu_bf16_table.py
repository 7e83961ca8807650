"""gat_level(..., table_dtype=torch.bfloat16): the inference forward on a bf16 feature table (csrc/k16_bf16_forward.hip).

The contract is "the fp32 level applied to Whq = round-to-nearest-even(x W)".  bf16_table_case builds inputs whose projection is
exact in fp32 in any summation order, so the kernel's table equals the CPU's bit for bit, and restates the level on Whq through
alpha_grad_case.level_ref.  Pricing is the one rule of tests/parity.py on the level output (parity.close_fwd: max(1e-5, 4 x the
fp32 run's own error)), as tests/test_gpu_edge_logit.py applies it: every case is drawn from a seed on whose fp64 run no logit
lies in the rounding band of the LeakyReLU kink.  No new tolerance."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import parity
from alpha_grad_case import src_of
from bf16_table_case import SLOPE, case, exact_inputs, hub_graph, reference, table
from pattern_device import DEV
from pattern_graphs import SHAPES, _asym_graph

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
FIN = 40
LANE_SHAPES = SHAPES + [s for s in [(8, 16), (2, 4), (1, 3), (3, 7), (6, 121), (8, 128), (4, 256)] if s not in SHAPES]
LID = ["x".join(map(str, s)) for s in LANE_SHAPES]


def _graph(rowptr, col, slot_edges=None):
    import pygat_amd as pg
    return pg.CSRGraph(torch.as_tensor(np.asarray(rowptr), device=DEV), torch.as_tensor(np.asarray(col), device=DEV), slot_edges)


def _run(graph, x, W, a, S, concat, **kw):
    import pygat_amd as pg
    H = W.shape[0]
    with torch.no_grad():
        return pg.gat_level(x.to(DEV), graph, [W[h].to(DEV) for h in range(H)], [a[h].to(DEV) for h in range(H)],
                            None if S is None else [S[h].to(DEV) for h in range(H)], SLOPE, concat, **kw)


def _check(what, rowptr, col, x, W, a, S, concat, graphs):
    o64, o32 = reference(x, rowptr, col, W, a, S, concat)
    outs = []
    for tag, graph in graphs:
        out = _run(graph, x, W, a, S, concat, table_dtype=BF16)
        assert out.dtype == torch.float32 and not out.requires_grad
        e = parity.close_fwd(out, o64, f"{what} [{tag}]", o32)
        print(f"{what} [{tag}]: err {e:.2e} (fp32 run {parity.err(o32, o64):.2e})")
        outs.append(out)
    return outs


def _pieces(rowptr, ts):
    """Slots the longest row meets at slot length ts (a lower bound on the pieces of its cut chain)."""
    return int(np.diff(np.asarray(rowptr)).max()) // ts


# ----------------------------------------------------------------------------------------------------------------- lane shapes
@pytest.mark.parametrize("skip", [False, True], ids=["noskip", "skip"])
@pytest.mark.parametrize("concat", [True, False], ids=["concat", "mean"])
@pytest.mark.parametrize("shape", LANE_SHAPES, ids=LID)
def test_lane_shapes(shape, concat, skip):
    """Every chunk mapping (8 elements per lane, 4 at padded F' = 4; one and two chunks per lane; idle lanes), rows of one edge,
    rows cut into two pieces and the hub cut into more than FIX_WIDE = 32 (slot length 4) resp. a few (64) pieces."""
    H, Fo = shape
    rowptr, col = hub_graph()
    assert _pieces(rowptr, 4) > 32 and 2 <= _pieces(rowptr, 64) <= 8
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=100 * H + Fo)
    graphs = [("default", _graph(rowptr, col)), ("slot 4", _graph(rowptr, col, 4)), ("slot 64", _graph(rowptr, col, 64))]
    outs = _check(f"bf16 {shape} concat={concat} skip={skip}", rowptr, col, x, W, a, S if skip else None, concat, graphs)
    if concat and not skip:      # a row with one edge: out_i = ELU(Whq_i), exactly
        lone = torch.as_tensor(np.diff(rowptr) == 1)
        whq = torch.cat(list(table(x, W, check_stats=False)), 1)[lone]
        assert torch.equal(outs[0].cpu()[lone][whq > 0], whq[whq > 0])


def test_asymmetric_pattern():
    H, Fo = 8, 16
    rowptr, col = _asym_graph()
    assert int((np.diff(rowptr) == 1).sum()) > 0
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=7)
    _check("bf16 asym", rowptr, col, x, W, a, S, True, [("default", _graph(rowptr, col)), ("slot 64", _graph(rowptr, col, 64))])


def test_head_windows():
    """H x padded F' = 12 x 128 = 1536 > 1024: two passes (8 + 4 heads), the tables addressed with the level's strides."""
    H, Fo = 12, 128
    rowptr, col = hub_graph()
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=12128)
    for concat in (True, False):
        _check(f"bf16 windows concat={concat}", rowptr, col, x, W, a, S, concat, [("default", _graph(rowptr, col))])


def test_determinism_and_none_is_the_plain_level():
    H, Fo = 8, 16
    rowptr, col = hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=816)
    r1 = _run(graph, x, W, a, S, True, table_dtype=BF16)
    r2 = _run(graph, x, W, a, S, True, table_dtype=BF16)
    assert torch.equal(r1, r2)
    plain = _run(graph, x, W, a, S, True)
    assert torch.equal(_run(graph, x, W, a, S, True, table_dtype=None), plain)
    assert not torch.equal(plain, r1)      # (the table IS rounded: the two levels differ)


def test_none_launches_what_the_plain_call_launches(monkeypatch):
    from pygat_amd import ops
    H, Fo = 8, 16
    rowptr, col = hub_graph()
    graph = _graph(rowptr, col)
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=816)
    seen, real = [], ops.lib

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
    for key, kw in (("absent", {}), ("none", {"table_dtype": None}), ("bf16", {"table_dtype": BF16})):
        seen.clear()
        _run(graph, x, W, a, S, True, **kw)
        seq[key] = list(seen)
    assert seq["none"] == seq["absent"] and not any("bf16" in s for s in seq["none"])
    assert "pygat_gat_pack_bf16" in seq["bf16"] and "pygat_gat_forward_bf16" in seq["bf16"] and "pygat_gat_forward" not in seq["bf16"]


def test_cora_topology():
    d = np.load(os.path.join(os.path.dirname(__file__), "golden", "cora_csr.npz"))
    rowptr, col = d["rowptr"], d["col"]
    H, Fo = 8, 8
    x, W, a, S = case(len(rowptr) - 1, FIN, H, Fo, rowptr, col, seed=88)
    _check("bf16 cora 8x8", rowptr, col, x, W, a, None, True, [("default", _graph(rowptr, col))])


# ------------------------------------------------------------------------------------------------------------------ the model
def test_two_level_model_is_its_levels():
    """Level 2's input is not exact, so the model is pinned to the level (bit for bit), not to the CPU restatement."""
    import pygat_amd as pg
    rowptr, col = hub_graph()
    graph = _graph(rowptr, col)
    torch.manual_seed(5)
    model = pg.GAT(nfeat=[FIN, 16, 7], nheads=[8, 2], nlayers=2, dropout=0.6, alpha=SLOPE, layer_type=pg.SpGraphAttentionLayer,
                   skip_connection=True).to(DEV).eval()
    x = torch.randn(len(rowptr) - 1, FIN, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        out = model(x, graph, table_dtype=BF16)
        h = x
        for lvl, heads in enumerate(model.gat_layers):
            h = pg.gat_level(h, graph, [m.W for m in heads], [m.a for m in heads], [m.skip_projection for m in heads], SLOPE,
                             lvl == 0, table_dtype=BF16)
        plain = model(x, graph)
    assert out.shape == (len(rowptr) - 1, 7) and torch.equal(out, h)
    with torch.no_grad():
        assert torch.equal(model(x, graph, table_dtype=None), plain) and not torch.equal(out, plain)
    layer = pg.SpGraphAttentionLayer(FIN, 16, dropout=0.0, alpha=SLOPE).to(DEV)
    adj = torch.zeros(len(rowptr) - 1, len(rowptr) - 1, device=DEV)
    adj[src_of(rowptr).to(DEV), torch.as_tensor(col, dtype=torch.int64, device=DEV)] = 1.0
    with torch.no_grad():
        o1 = layer(x, adj, table_dtype=BF16)
        o2 = pg.gat_level(x, graph, [layer.W], [layer.a], None, SLOPE, True, table_dtype=BF16)
    assert torch.equal(o1, o2)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    import pygat_amd as pg
    from pygat_amd import gatv2, ops
    from pygat_amd.graphed import FusedEpoch, GraphedLevel
    rowptr, col = hub_graph(N=200, seed=2, hub_deg=100)
    graph = _graph(rowptr, col)
    x, W, a, S = exact_inputs(200, 16, 2, 8, seed=2)      # (nothing is computed from them but the two last calls)
    xd = x.to(DEV)
    Ws, As = [W[h].to(DEV) for h in range(2)], [a[h].to(DEV) for h in range(2)]
    launched, real = [], ops.lib

    class Spy:      # nothing may be launched by a refused call
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("pygat_") or name in ("pygat_last_error", "pygat_head_group", "pygat_padded_width"):
                return fn

            def wrapped(*args):
                launched.append(name)
                return fn(*args)
            return wrapped
    lvl = lambda **kw: pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, **{"table_dtype": BF16, **kw})   # noqa: E731
    gl = GraphedLevel(graph, xd, W.to(DEV), a.to(DEV), warmup=1)
    monkeypatch.setattr(ops, "lib", Spy())
    with torch.no_grad():
        for bad in (torch.float16, torch.float32, "bf16"):
            with pytest.raises(ValueError, match="table_dtype"):
                lvl(table_dtype=bad)
        with pytest.raises(ValueError, match="table_dtype.*pipeline"):
            lvl(pipeline=(2, lambda *a_: None))
        with pytest.raises(ValueError, match="table_dtype.*xs"):
            lvl(xs=object())
        for ra in (True, "grad"):
            with pytest.raises(ValueError, match="table_dtype.*return_attention"):
                lvl(return_attention=ra)
        with pytest.raises(ValueError, match="table_dtype.*attention_order"):
            lvl(attention_order=(graph, None))
        with pytest.raises(ValueError, match="table_dtype.*edge_logit"):
            lvl(edge_logit=torch.zeros(len(col), 2, device=DEV))
        for g2 in (graph.internal_view(), graph.degree_ordered()[0]):
            with pytest.raises(ValueError, match="table_dtype.*row map"):
                pg.gat_level(xd, g2, Ws, As, None, SLOPE, True, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype.*column-blocked"):
            pg.gat_level(xd.reshape(200, 1, 16).transpose(0, 1).contiguous(), graph, Ws, As, None, SLOPE, True, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype"):
            gl.forward(table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype"):
            gl(table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype"):
            FusedEpoch.run(object.__new__(FusedEpoch), table_dtype=BF16)
        W2, a2 = [torch.cat([w, w]) for w in Ws], [v[:8].contiguous() for v in As]
        with pytest.raises(ValueError, match="table_dtype"):
            gatv2.gatv2_level(xd, graph, W2, a2, None, SLOPE, True, table_dtype=BF16)
        adj = torch.zeros(200, 200, device=DEV)
        adj[src_of(rowptr).to(DEV), torch.as_tensor(col, dtype=torch.int64, device=DEV)] = 1.0
        for cls in (gatv2.SpGraphAttentionLayerV2, gatv2.GraphAttentionLayerV2):
            with pytest.raises(ValueError, match="table_dtype"):
                cls(16, 8, dropout=0.0, alpha=SLOPE).to(DEV)(xd, adj, table_dtype=BF16)
        mk = lambda **kw: pg.GAT(**{"nfeat": [16, 8, 3], "nheads": [2, 1], "nlayers": 2, "dropout": 0.0, "alpha": SLOPE,   # noqa: E731
                                    "layer_type": pg.SpGraphAttentionLayer, **kw}).to(DEV)
        with pytest.raises(ValueError, match="table_dtype.*head_parallel"):
            mk(head_parallel=True)(xd, graph, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype.*level_fn"):
            mk(level_fn=lambda *a_: None)(xd, graph, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype.*v1"):
            mk(layer_type=gatv2.SpGraphAttentionLayerV2)(xd, graph, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype.*dropout"):
            mk(dropout=0.5).train()(xd, graph, table_dtype=BF16)
        with pytest.raises(ValueError, match="table_dtype.*return_attention"):
            mk()(xd, graph, table_dtype=BF16, return_attention=True)
        with pytest.raises(ValueError, match="table_dtype.*edge_logits"):
            mk()(xd, graph, table_dtype=BF16, edge_logits=[torch.zeros(len(col), device=DEV), None])
        with pytest.raises(ValueError, match="table_dtype.*dropout"):
            pg.SpGraphAttentionLayer(16, 8, dropout=0.5, alpha=SLOPE).to(DEV).train()(xd, adj, table_dtype=BF16)
    # no backward: autograd on and anything that requires grad
    for which in range(4):
        leaves = [xd.clone(), Ws[0].clone(), As[0].clone(), S[0].to(DEV)]
        leaves[which].requires_grad_(True)
        with pytest.raises(ValueError, match="inference only"):
            pg.gat_level(leaves[0], graph, [leaves[1], Ws[1]], [leaves[2], As[1]], [leaves[3], S[1].to(DEV)], SLOPE, True, table_dtype=BF16)
    with pytest.raises(ValueError, match="inference only"):
        mk().eval()(xd, graph, table_dtype=BF16)      # (parameters require grad, autograd is on)
    assert launched == [], launched
    # what is taken: parameters that require grad under no_grad, detached parameters with autograd on
    Wg = [w.clone().requires_grad_(True) for w in Ws]
    with torch.no_grad():
        o1 = pg.gat_level(xd, graph, Wg, As, None, SLOPE, True, table_dtype=BF16)
    o2 = pg.gat_level(xd, graph, [w.detach() for w in Wg], As, None, SLOPE, True, table_dtype=BF16)
    assert torch.equal(o1, o2) and not o2.requires_grad and "pygat_gat_forward_bf16" in launched


# ------------------------------------------------------------------------------------------------------------------- footprint
def _k16_names():
    names = ["k16_pack"]
    for kind in ("fwd", "fix"):
        names += [f"k16_{kind}_c{cw}l{lpr}v1" for cw in (4, 8) for lpr in (1, 2, 4, 8, 16, 32, 64)] + [f"k16_{kind}_c8l64v2"]
    return names


def test_new_kernels_have_no_scratch():
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    for name in _k16_names():
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and regs.value > 0, (name, regs.value, scratch.value)
    # 8 heads x 16: 16 chunks of 8 elements = 16 lanes per row, one chunk per lane; four waves per SIMD like K2 and K15
    assert lib.pygat_kernel_footprint(b"k16_fwd_c8l16v1", C.byref(regs), C.byref(scratch)) == 0
    assert scratch.value == 0 and 0 < regs.value <= 128, (regs.value, scratch.value)
    for bad in (b"k16_fwd_c8l3v1", b"k16_fwd_c4l64v2", b"k16_fwd_c6l8v1", b"k16_nope"):
        assert lib.pygat_kernel_footprint(bad, C.byref(regs), C.byref(scratch)) == -1
