"""pygat_amd.spmm / SpecialSpmm (csrc/k17_spmm.hip): the reference's sparse-region SpMM (layers.py:70-95) with heads, and its two
gradients.

Ground truth is torch autograd in fp64 on the CPU through spmm_case.spmm_ref (an index_add over the entries).  Loss L = <out, G>,
G ~ N(0, 1), seeded.  Pricing is parity.check_autograd, unchanged: out by close_fwd, dvalues / db by close_grad, i.e. max(1e-5, 4 x
the fp32 run's own error).  The main cases use row-softmax values (the op's real use), one uses N(0, 1) values.  Every case's inputs
come from `_inputs` with a fixed seed; each was run on the CPU with the fp32 ground-truth run standing in for the device (`run=`
of `_check`) and passes there.  The device and both ground-truth runs are fed the same fp32-rounded numbers."""
import ctypes as C
import importlib

import pytest
import torch

import parity
from alpha_grad_case import kink_count, level_ref
from long_row_cases import nine_hubs, three_chunk_hub
from pattern_device import DEV, _graph
from pattern_graphs import COMPOSE_SEED, SHAPES, SID, SLOPE, _asym_graph, _hub_graph, _params, _rect_coo, _repeat_coo
from spmm_case import coo_of, f32, normal, softmax_values, spmm_ref

pytestmark = pytest.mark.gpu


def _inputs(row, n_rows, n_cols, H, F, seed, heads=True, values="softmax"):
    """-> (values [E, H] | [E], b [M, H, F] | [M, F], G like out), float64 holding fp32-representable numbers."""
    v = softmax_values(row, n_rows, H, seed) if values == "softmax" else normal((row.numel(), H), seed)
    b = normal((n_cols, H, F), seed + 1)
    G = normal((n_rows, H, F), seed + 2)
    if not heads:
        assert H == 1
        v, b, G = v[:, 0], b[:, 0], G[:, 0]
    return f32(v), f32(b), f32(G)


def _device_run(pattern, v, b, G, fn=None):
    """-> (out, dvalues, db) on the device."""
    import pygat_amd as pg
    vd, bd = v.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    out = (fn or pg.spmm)(pattern, vd, bd)
    dv, db = torch.autograd.grad(out, [vd, bd], G.float().to(DEV))
    return out.detach(), dv, db


def _check(what, row, col, shape, v, b, G, pattern=None, run=None):
    """One product and both gradients against the ground truth; run: what stands in for the device (the CPU rehearsal of a seed)."""
    import pygat_amd as pg
    if run is None:
        if pattern is None:
            pattern = pg.EdgePattern.from_indices(torch.stack([row, col]).to(DEV), shape)
        out, dv, db = _device_run(pattern, v, b, G)
    else:
        out, dv, db = run(v, b, G)
    assert out.shape == G.shape and dv.shape == v.shape and db.shape == b.shape, what
    rep, (y64, g64) = parity.check_autograd(out.reshape(-1), [dv, db], lambda v_, b_: spmm_ref(row, col, shape[0], v_, b_).reshape(-1),
                                            [v, b], G.reshape(-1), ["dvalues", "db"], what)
    print(what, {k: f"{e:.2e}" for k, e in rep.items()})
    return out, dv, db


def fp32_stand_in(row, col, n_rows):
    """The fp32 ground-truth run in the device's place: the rehearsal that a seed's inputs pass the pricing at all."""
    def run(v, b, G):
        vv, bb = v.float().requires_grad_(True), b.float().requires_grad_(True)
        out = spmm_ref(row, col, n_rows, vv, bb)
        dv, db = torch.autograd.grad(out, [vv, bb], G.float())
        return out.detach(), dv, db
    return run


def _hub_coo():
    rowptr, col = _hub_graph()
    return coo_of(rowptr, col) + (len(rowptr) - 1,)


def _asym_coo():
    rowptr, col = _asym_graph()
    return coo_of(rowptr, col) + (len(rowptr) - 1,)


def _big_hub_coo():
    rowptr, col = three_chunk_hub()
    return coo_of(rowptr, col) + (len(rowptr) - 1,)


# ---------------------------------------------------------------------------------------------------------------------- drop-in
@pytest.mark.parametrize("F", [1, 7, 8, 64, 256, 1024])
def test_drop_in(F):
    """The reference's call, indices from a dense adjacency's nonzero().t(): bit-equal to spmm, gradients (None, ., None, .)."""
    import pygat_amd as pg
    row, col, N = _hub_coo()
    adj = torch.zeros(N, N, device=DEV)
    adj[row.to(DEV), col.to(DEV)] = 1.0
    indices = adj.nonzero().t()
    assert torch.equal(indices.cpu(), torch.stack([row, col]))
    v, b, G = _inputs(row, N, N, 1, F, seed=100 + F, heads=False)
    spmm_mod = pg.SpecialSpmm()
    drop = lambda pattern, vd, bd: spmm_mod(indices, vd, torch.Size([N, N]), bd)   # noqa: E731
    got = _device_run(None, v, b, G, fn=drop)
    ours = _check(f"drop-in F={F}", row, col, (N, N), v, b, G)
    for p, q in zip(got, ours):
        assert torch.equal(p, q)
    # the backward's own return: gradients for values and b only
    vd, bd = v.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    out = pg.SpecialSpmmFunction.apply(indices, vd, torch.Size([N, N]), bd)
    grads = pg.SpecialSpmmFunction.backward(out.grad_fn, G.float().to(DEV))
    assert len(grads) == 4 and grads[0] is None and grads[2] is None
    assert torch.equal(grads[1], ours[1]) and torch.equal(grads[3], ours[2])
    # the [N, 1] ones vector of layers.py:150: the row sums of the values
    ones = torch.ones(N, 1, device=DEV)
    rs = spmm_mod(indices, v.float().to(DEV), torch.Size([N, N]), ones)
    parity.close_fwd(rs, spmm_ref(row, col, N, v, torch.ones(N, 1, dtype=torch.float64)), "row sum")


# ------------------------------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("shape", SHAPES + [(3, 8), (6, 16)], ids=SID + ["3x8", "6x16"])
def test_heads(shape):
    """Hub rows and columns of 699 entries (the long-row launch, forward and db) and the explicit transpose; 16-byte chunks, and
    single floats at F = 7."""
    H, F = shape
    row, col, N = _hub_coo()
    _check(f"heads hub {shape}", row, col, (N, N), *_inputs(row, N, N, H, F, seed=200 + H * F))
    row, col, N = _asym_coo()
    _check(f"heads asym {shape}", row, col, (N, N), *_inputs(row, N, N, H, F, seed=300 + H * F))


def test_scalar_lanes_with_heads():
    """F = 7 with heads: 56 floats on 64 lanes, 8 x 13 = 104 on two floats per lane, 64 x 9 = 576 in three windows of 256."""
    row, col, N = _hub_coo()
    for H, F in ((8, 7), (8, 13), (64, 9)):
        _check(f"scalar {H}x{F}", row, col, (N, N), *_inputs(row, N, N, H, F, seed=400 + H * F))


def test_normal_values():
    row, col, N = _hub_coo()
    _check("N(0,1) values", row, col, (N, N), *_inputs(row, N, N, 8, 16, seed=500, values="normal"))


def test_rows_and_columns_of_several_chunks():
    """A row and a column of >= 4 097 entries: three chunks merged in order, in the forward and in db."""
    row, col, N = _big_hub_coo()
    _check("three chunks 8x16", row, col, (N, N), *_inputs(row, N, N, 8, 16, seed=600))
    _check("three chunks 1x7", row, col, (N, N), *_inputs(row, N, N, 1, 7, seed=601, heads=False))


@pytest.mark.parametrize("shape", [(8, 16), (1, 7)], ids=["8x16", "1x7"])
def test_every_slot_of_a_chunk(shape):
    """long_row_cases.nine_hubs: nine rows (and columns) of 521 entries back to back fill slots 1-4, 0-4 and 0-1 of three chunks,
    in the forward and in db; 1 x 7 without a head axis.  Two runs give the same bits."""
    import pygat_amd as pg
    H, F = shape
    rowptr, col = nine_hubs()
    row, col, N = coo_of(rowptr, col) + (len(rowptr) - 1,)
    pattern = pg.EdgePattern.from_indices(torch.stack([row, col]).to(DEV), (N, N))
    v, b, G = _inputs(row, N, N, H, F, seed=1200 + H * F, heads=H > 1)
    first = _check(f"nine hubs {shape}", row, col, (N, N), v, b, G, pattern=pattern)
    for p, q in zip(first, _device_run(pattern, v, b, G)):
        assert torch.equal(p, q)


def test_graph_pattern_matches_indices():
    """CSRGraph.edge_pattern(): entry order = edge_index(); the graph's own mirror permutation / transpose serve db."""
    import pygat_amd as pg
    for name, (rowptr, col) in (("hub", _hub_graph()), ("asym", _asym_graph())):
        graph = _graph(rowptr, col)
        pattern = graph.edge_pattern()
        assert pattern is graph.edge_pattern() and pattern.has_transpose and pattern.perm is None
        assert torch.equal(pattern.edge_rc.t().long(), graph.edge_index())
        r, c = coo_of(rowptr, col)
        N = len(rowptr) - 1
        v, b, G = _inputs(r, N, N, 8, 16, seed=650)
        got = _check(f"graph pattern {name}", r, c, (N, N), v, b, G, pattern=pattern)
        ours = _device_run(pg.EdgePattern.from_indices(graph.edge_index(), (N, N)), v, b, G)
        for p, q in zip(got, ours):
            assert torch.equal(p, q)


# ------------------------------------------------------------------------------------------------------------------ rectangular
def test_rectangular_with_empty_rows_and_columns():
    row, col = _rect_coo()
    out, dv, db = _check("rectangular", row, col, (300, 500), *_inputs(row, 300, 500, 4, 8, seed=700))
    assert out.shape == (300, 4, 8) and db.shape == (500, 4, 8)
    assert float(out[0::3].abs().max()) == 0.0, "a row without entries must be exactly 0"
    assert float(db[0::4].abs().max()) == 0.0, "db of a column without entries must be exactly 0"
    assert float(out.abs().max()) > 0 and float(db.abs().max()) > 0


def test_unsorted_entries_with_repeats():
    row, col, N, pairs = _repeat_coo()
    assert pairs.shape[0] > 100 and bool((row[1:] < row[:-1]).any())
    out, dv, db = _check("repeats", row, col, (N, N), *_inputs(row, N, N, 8, 16, seed=800))
    assert torch.equal(dv[pairs[:, 0].to(DEV)], dv[pairs[:, 1].to(DEV)]), "dvalues of a repeated pair must be equal"


# ------------------------------------------------------------------------------------------------------------------ composition
def test_composition_with_a_level():
    """y = spmm(graph.edge_pattern(), alpha, table), alpha the differentiable coefficients of a level; the loss uses y only."""
    import pygat_amd as pg
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    N, E = len(rowptr) - 1, len(col)
    r, c = coo_of(rowptr, col)
    x, W, a, _ = _params(N, 48, H, Fo, seed=COMPOSE_SEED)
    assert kink_count(x, rowptr, col, W, a, SLOPE) == 0, "an input with a logit inside the kink band -- choose another seed"
    table, G = f32(normal((N, H, Fo), 900)), f32(normal((N, H, Fo), 901))
    graph = _graph(rowptr, col)
    xd = x.to(DEV).requires_grad_(True)
    Ws = [W[h].to(DEV).requires_grad_(True) for h in range(H)]
    As = [a[h].to(DEV).requires_grad_(True) for h in range(H)]
    td = table.float().to(DEV).requires_grad_(True)
    out, alpha = pg.gat_level(xd, graph, Ws, As, None, SLOPE, True, return_attention="grad")
    assert alpha.requires_grad and alpha.shape == (E, H)
    y = pg.spmm(graph.edge_pattern(), alpha, td.view(N, H, Fo))
    grads = torch.autograd.grad(y, [xd] + Ws + As + [td], G.float().to(DEV))
    got = [grads[0], torch.stack(grads[1:1 + H]), torch.stack([g.reshape(-1) for g in grads[1 + H:1 + 2 * H]]), grads[-1]]

    def fn(x_, W_, a_, t_):
        _, al = level_ref(x_, rowptr, col, W_, a_, None, SLOPE, True)
        return spmm_ref(r, c, N, al, t_).reshape(-1)
    rep, _ = parity.check_autograd(y.detach().reshape(-1), got, fn, [x.double(), W.double(), a.double(), table], G.reshape(-1),
                                   ["dX", "dW", "da", "dtable"], "level + spmm")
    print("level + spmm", {k: f"{e:.2e}" for k, e in rep.items()})


# ---------------------------------------------------------------------------------------------------- determinism and launches
def test_two_runs_are_bit_equal():
    import pygat_amd as pg
    row, col, N = _big_hub_coo()
    pattern = pg.EdgePattern.from_indices(torch.stack([row, col]).to(DEV), (N, N))
    v, b, G = _inputs(row, N, N, 8, 16, seed=1000)
    runs = [_device_run(pattern, v, b, G) for _ in range(2)]
    for p, q in zip(*runs):
        assert torch.equal(p, q)
    v, b, G = _inputs(row, N, N, 1, 7, seed=1001, heads=False)
    runs = [_device_run(pattern, v, b, G) for _ in range(2)]
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    spmm_mod = importlib.import_module("pygat_amd.spmm")     # (the package attribute of that name is the function)
    row, col, N = _asym_coo()
    v, b, G = _inputs(row, N, N, 8, 16, seed=1100)
    seen = []
    real = spmm_mod.lib

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("pygat_") or name == "pygat_last_error":
                return fn

            def wrapped(*args):
                seen.append(name)
                return fn(*args)
            return wrapped
    monkeypatch.setattr(spmm_mod, "lib", Spy())
    Gd = G.float().to(DEV)
    indices = torch.stack([row, col]).to(DEV)

    def run(v_grad, b_grad):
        pattern = pg.EdgePattern.from_indices(indices, (N, N))
        seen.clear()
        vd, bd = v.float().to(DEV).requires_grad_(v_grad), b.float().to(DEV).requires_grad_(b_grad)
        out = pg.spmm(pattern, vd, bd)
        torch.autograd.grad(out, [t for t in (vd, bd) if t.requires_grad], Gd)
        return list(seen), pattern
    seq, pattern = run(True, True)
    assert seq == ["pygat_spmm_forward", "pygat_spmm_grad_values", "pygat_spmm_forward"] and pattern.has_transpose
    seq, pattern = run(False, True)
    assert seq == ["pygat_spmm_forward", "pygat_spmm_forward"] and pattern.has_transpose
    seq, pattern = run(True, False)
    assert seq == ["pygat_spmm_forward", "pygat_spmm_grad_values"] and not pattern.has_transpose


# --------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import pygat_amd as pg
    row, col, N = _asym_coo()
    E = row.numel()
    indices = torch.stack([row, col]).to(DEV)
    pattern = pg.EdgePattern.from_indices(indices, (N, N))
    v, b = torch.rand(E, device=DEV), torch.rand(N, 8, device=DEV)
    with pytest.raises(ValueError, match="GPU"):
        pg.spmm(pattern, v.cpu(), b)
    with pytest.raises(ValueError, match="GPU"):
        pg.spmm(pattern, v, b.cpu())
    with pytest.raises(ValueError, match="GPU"):
        pg.SpecialSpmm()(indices.cpu(), v, torch.Size([N, N]), b)
    with pytest.raises(ValueError, match="GPU"):
        pg.EdgePattern.from_indices(indices.cpu(), (N, N))
    with pytest.raises(ValueError, match="float32"):
        pg.spmm(pattern, v.double(), b)
    with pytest.raises(ValueError, match="float32"):
        pg.spmm(pattern, v, b.half())
    with pytest.raises(ValueError, match="H \\* F <= 1024"):
        pg.spmm(pattern, v, torch.rand(N, 1028, device=DEV))
    with pytest.raises(ValueError, match="H \\* F <= 1024"):
        pg.spmm(pattern, torch.rand(E, 4, device=DEV), torch.rand(N, 4, 257, device=DEV))
    with pytest.raises(ValueError, match="H <= 64"):
        pg.spmm(pattern, torch.rand(E, 65, device=DEV), torch.rand(N, 65, 4, device=DEV))
    bad = indices.clone()
    bad[1, 5] = N
    with pytest.raises(ValueError, match="outside the shape"):
        pg.EdgePattern.from_indices(bad, (N, N))
    bad[1, 5] = -1
    with pytest.raises(ValueError, match="outside the shape"):
        pg.SpecialSpmm()(bad, v, torch.Size([N, N]), b)
    with pytest.raises(ValueError, match="outside the shape"):
        pg.EdgePattern.from_indices(indices, (N, N - 1))
    with pytest.raises(ValueError, match="values \\[E, H\\] with b \\[M, H, F\\]"):
        pg.spmm(pattern, torch.rand(E, 2, device=DEV), b)
    with pytest.raises(ValueError, match="values \\[E, H\\] with b \\[M, H, F\\]"):
        pg.spmm(pattern, v, torch.rand(N, 2, 8, device=DEV))
    with pytest.raises(ValueError, match="values \\[E\\] and b \\[M, F\\]"):
        pg.SpecialSpmm()(indices, torch.rand(E, 2, device=DEV), torch.Size([N, N]), torch.rand(N, 2, 8, device=DEV))
    with pytest.raises(ValueError, match=f"{E - 1} rows but the pattern has {E} entries"):
        pg.spmm(pattern, v[:-1], b)
    with pytest.raises(ValueError, match=f"{N + 1} rows but the pattern has {N} columns"):
        pg.spmm(pattern, v, torch.rand(N + 1, 8, device=DEV))
    # an uncached pattern under stream capture: a ValueError, not an aborted capture; a cached one is taken
    pg.clear_pattern_cache()
    fresh = indices.clone()
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            pg.SpecialSpmm()(fresh, v, torch.Size([N, N]), b)
    torch.cuda.synchronize()
    want = pg.SpecialSpmm()(fresh, v, torch.Size([N, N]), b)      # builds and caches the pattern of `fresh`
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = pg.SpecialSpmm()(fresh, v, torch.Size([N, N]), b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    pg.clear_pattern_cache()


def test_pattern_cache():
    import pygat_amd as pg
    spmm_mod = importlib.import_module("pygat_amd.spmm")     # (the package attribute of that name is the function)
    row, col, N = _asym_coo()
    indices = torch.stack([row, col]).to(DEV)
    v, b = torch.rand(row.numel(), device=DEV), torch.rand(N, 8, device=DEV)
    pg.clear_pattern_cache()
    want = pg.SpecialSpmm()(indices, v, torch.Size([N, N]), b)
    assert len(spmm_mod._patterns) == 1
    pg.SpecialSpmm()(indices, v, torch.Size([N, N]), b)
    assert len(spmm_mod._patterns) == 1                           # the same tensor, untouched: the same pattern
    indices[:, :2] = indices[:, :2].flip(1)                       # written in place: the version counter moves, a new pattern
    got = pg.SpecialSpmm()(indices, v, torch.Size([N, N]), b)
    assert len(spmm_mod._patterns) == 2
    r2, c2 = indices[0].cpu(), indices[1].cpu()
    parity.close_fwd(got, spmm_ref(r2, c2, N, v.double().cpu(), b.double().cpu()), "after an in-place edit")
    assert want.shape == got.shape
    for k in range(spmm_mod.PATTERN_CACHE_SIZE + 3):              # bounded
        pg.SpecialSpmm()(indices.clone(), v, torch.Size([N, N]), b)
    assert len(spmm_mod._patterns) == spmm_mod.PATTERN_CACHE_SIZE
    pg.clear_pattern_cache()
    assert len(spmm_mod._patterns) == 0


# -------------------------------------------------------------------------------------------------------------------- footprint
def _k17_names():
    names = ["k17_sddmm_c4", "k17_sddmm_c1"]
    for kind in ("long", "row"):
        for cw, wide in ((4, (2, 3, 4)), (1, (2, 4))):
            names += [f"k17_spmm_{kind}_c{cw}l{lpr}v1" for lpr in (1, 2, 4, 8, 16, 32, 64)]
            names += [f"k17_spmm_{kind}_c{cw}l64v{v}" for v in wide]
    return names


def test_new_kernels_have_no_scratch():
    from pygat_amd._lib import lib
    for name in _k17_names():
        regs, scratch = C.c_int(-1), C.c_int(-1)
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and 0 < regs.value <= 128, (name, regs.value, scratch.value)
    for bad in (b"k17_spmm_row_c4l3v1", b"k17_spmm_row_c1l64v3", b"k17_spmm_row_c2l8v1", b"k17_sddmm_c2", b"k17_spmm_row_c4l8v1x"):
        assert lib.pygat_kernel_footprint(bad, C.byref(regs), C.byref(scratch)) == -1, bad
