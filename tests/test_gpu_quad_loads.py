"""Quad-distributed loads of the headline edge walks (csrc/k2_forward.hip, csrc/k4_backward_col.hip: PYGAT_K2_QUAD_LOADS,
PYGAT_K4_QUAD_LOADS, PYGAT_K4_QUAD_PREFETCH): lane q of a head's DPP quad loads edge q's record, s_i and (s, m, 1/Z, D) record for the whole round and
quad_bcast hands them round.

Every case runs the training level at H = 8, F' = 16, Fin = 32 (K2: gat_fwd_kernel<32,1,false,true,true,4,128>; K4:
gat_bwd_col_kernel<32,1,false,4,128,true> with the a-gradient fold at ops.DA_MIN_BYTES = 0, <32,1,false,4,128> otherwise)
with gradients for W and a, against the fp64 oracle under the one rule of tests/parity.py, and twice: the two runs must be
bit-identical.  The patterns are symmetric with self loops, N <= 400, from seeded generators, and aim at what a load
distributed over a quad can get wrong: the clamp of a last round filled in part, a row change on every edge, a row cut over
many slots (both lane groups of a wave, the wide fix-up), a last slot of one edge, and lane groups of unequal length (one
group's lanes switched off while the other still broadcasts).

Slot lengths: the row-snapped borders (pygat_slot_bounds) move a border by less than slot_edges / 2, so 4-edge slots come out
with 3, 4 or 5 edges (the last one with 1..4) and 64-edge slots with 33..95.  The lengths 1, 2, 3, 5, 6 and 7 are therefore
asserted where they can occur: 2, 3 and 5 at slot_edges 4, 5, 6 and 7 at slot_edges 8 (which the partly-filled pattern runs in
addition to 4 and 64), 1 as the last slot of `one_edge_last_slot`; at 64 every residue 1, 2, 3 of the length modulo 4.
"""
import numpy as np
import pytest
import torch

from oracle import gat_oracle as O
from parity import check_level

pytestmark = pytest.mark.gpu

H, FO, FIN = 8, 16, 32


@pytest.fixture(scope="module")
def pg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import pygat_amd
    return pygat_amd


# ------------------------------------------------------------------- patterns
def _sym_csr(N, r, c):
    """Symmetric pattern + self loops from undirected pairs (r, c)."""
    r = np.asarray(r, dtype=np.int64); c = np.asarray(c, dtype=np.int64)
    rr = np.concatenate([r, c, np.arange(N)]); cc = np.concatenate([c, r, np.arange(N)])
    key = np.unique(rr * N + cc)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // N, minlength=N))]).astype(np.int32)
    return rowptr, (key % N).astype(np.int32)


def partly_filled():
    """Degrees 1..9 mixed."""
    rowptr, col = O.random_symmetric_csr(300, 3.2, 2)
    deg = np.diff(rowptr)
    assert set(range(1, 10)) <= set(deg.tolist())
    return rowptr, col


def row_change_every_edge():
    """200 rows with only their self loop, then 100 pairs: rows of degree 2."""
    i = np.arange(100)
    rowptr, col = _sym_csr(400, 200 + 2 * i, 201 + 2 * i)
    deg = np.diff(rowptr)
    assert (deg[:200] == 1).all() and (deg[200:] == 2).all()
    return rowptr, col


def one_hub():
    """One row of degree >= 150 among short rows."""
    rowptr, col = O.random_symmetric_csr(300, 2.0, 7, hub=(140, 180))
    deg = np.diff(rowptr)
    assert deg.max() >= 150 and np.sort(deg)[-2] < 16
    return rowptr, col


def one_edge_last_slot():
    """nnz = 1 modulo 64 and a last row with only its self loop: the last slot has one edge at slot_edges 4 and 64."""
    rng = np.random.default_rng(11)
    n0 = 200
    r, c = rng.integers(0, n0, 300), rng.integers(0, n0, 300)
    rowptr, _ = _sym_csr(n0, r, c)
    extra = (1 - int(rowptr[-1])) % 64
    extra = extra if extra > 0 else 64                 # isolated nodes behind the others: one edge each
    rowptr, col = _sym_csr(n0 + extra, r, c)
    assert int(rowptr[-1]) % 64 == 1 and rowptr[-1] - rowptr[-2] == 1 and len(rowptr) - 1 <= 400
    return rowptr, col


def unequal_lane_groups():
    """Row 0 has 95 edges (itself and nodes 1..94, which have nothing else): the border at edge 64 moves to its end, slot 0
    gets 95 edges and slot 1, the other lane group of the wave, 34.  Rows of 5 edges at multiples of 4 do the same to 4-edge slots
    (5 against 3), and the isolated nodes at the end leave a last wave with one lane group only or a last slot shorter than its
    neighbour."""
    rng = np.random.default_rng(13)
    r = [np.zeros(94, dtype=np.int64)]; c = [np.arange(1, 95)]
    base = 95
    for _ in range(30):                                 # stars of 4 leaves: a row of 5 edges, then 4 rows of 2
        r.append(np.full(4, base)); c.append(base + 1 + np.arange(4)); base += 5
    rr, cc = rng.integers(base, 330, 120), rng.integers(base, 330, 120)
    r.append(rr); c.append(cc)
    return _sym_csr(333, np.concatenate(r), np.concatenate(c))


PATTERNS = {"partly_filled": partly_filled, "row_change_every_edge": row_change_every_edge, "one_hub": one_hub,
            "one_edge_last_slot": one_edge_last_slot, "unequal_lane_groups": unequal_lane_groups}
CASES = [(name, slot) for name in PATTERNS for slot in ((4, 8, 64) if name == "partly_filled" else (4, 64))]


def slot_lengths(g, slot):
    """Edges per slot of the row-snapped slots the level walks (pygat_slot_bounds through graph._Pattern)."""
    g.fwd.ref(slot)
    sb = g.fwd._alt[(slot, True)][1].cpu().numpy().astype(np.int64)
    return np.diff(sb)


def check_slots(name, slot, g, rowptr):
    ln = slot_lengths(g, slot)
    assert ln.min() >= 1 and ln.sum() == rowptr[-1]
    have = set(ln.tolist())
    if name == "partly_filled":
        want = {4: {2, 3, 5}, 8: {5, 6, 7}}.get(slot)
        if want is not None:
            assert want <= have, (slot, sorted(have))
        else:
            assert {1, 2, 3} <= set((ln % 4).tolist()), sorted(have)
    elif name == "row_change_every_edge":
        assert ln[0] == slot                                                # whole rounds of four one-edge rows
    elif name == "one_hub":
        deg = np.diff(rowptr)
        assert deg.max() // slot >= 2                                        # a row cut over several slots ...
        if slot == 4:
            assert deg.max() // slot > 32                                    # ... at 4-edge slots over more than 32: the wide fix-up
    elif name == "one_edge_last_slot":
        assert ln[-1] == 1, ln[-4:]
    elif name == "unequal_lane_groups":
        rounds = -(-ln // 4)
        pairs = rounds[: len(rounds) // 2 * 2].reshape(-1, 2)                # slots 2w and 2w + 1 share wave w
        gap = int(np.abs(pairs[:, 0] - pairs[:, 1]).max())
        assert gap >= (10 if slot == 64 else 1), (slot, gap)
        if slot == 64:
            assert ln[0] == 95 and ln[1] <= 36
    return ln


def run_level(pg, g, x64, W, a, G64):
    dev = "cuda:0"
    x = x64.float().to(dev)
    Wd = W.float().to(dev).requires_grad_(True)
    ad = a.float().to(dev).requires_grad_(True)
    out = pg.GATLevelFn.apply(x, Wd, ad, None, g, 0.2, True)
    out.backward(G64.float().to(dev))
    torch.cuda.synchronize()
    return out.detach(), Wd.grad, ad.grad


@pytest.mark.parametrize("name,slot", CASES, ids=[f"{n}-slot{s}" for n, s in CASES])
def test_quad_loads_level(pg, monkeypatch, name, slot):
    rowptr, col = PATTERNS[name]()
    N = len(rowptr) - 1
    assert N <= 400
    dev = "cuda:0"
    g = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev), slot_edges=slot)
    assert g.symmetric
    ln = check_slots(name, slot, g, rowptr)
    gen = torch.Generator().manual_seed(17)
    W = torch.randn(H, FIN, FO, generator=gen, dtype=torch.float64) * (1.414 * (2.0 / (FIN + FO)) ** 0.5)
    a = torch.randn(H, 2 * FO, generator=gen, dtype=torch.float64) * (1.414 * (2.0 / (1 + 2 * FO)) ** 0.5)
    x = torch.randn(N, FIN, dtype=torch.float64, generator=gen)
    G = torch.randn(N, H * FO, dtype=torch.float64, generator=gen)
    from pygat_amd._lib import lib
    assert lib.pygat_gat_backward_col_da_bytes(g.bwd.ref(slot), H, FO, H) > 0     # the column pass can take da along here
    res = {}
    for tag, minb in (("fold", 0), ("pass", pg.ops.DA_MIN_BYTES)):            # da in the column pass + fold / by the pass of its own
        monkeypatch.setattr(pg.ops, "DA_MIN_BYTES", minb)
        first = run_level(pg, g, x, W, a, G)
        again = run_level(pg, g, x, W, a, G)
        for t, u, what in zip(first, again, ("out", "dW", "da")):
            assert torch.equal(t, u), f"{name} slot {slot} {tag}: {what} differs between two runs"
        out, dW, da = first
        check_level(out, {"dX": None, "dW": dW, "da": da}, x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, True,
                          G.numpy(), None, what=f"{name}, {slot}-edge slots ({len(ln)} of {ln.min()}..{ln.max()} edges), da by {tag}")
        res[tag] = first
        monkeypatch.undo()
    assert torch.equal(res["fold"][0], res["pass"][0]) and torch.equal(res["fold"][1], res["pass"][1])   # out, dW: da's route changes neither


@pytest.mark.parametrize("slot", [4, 64])
def test_quad_loads_run_time_strides(pg, slot):
    """6 heads x 16: rows of 96 floats on 32 lanes with heads of one quad -- the instantiations with run-time strides, whose
    last two quads hold no column: gat_fwd_kernel<32,1,false,true,true,4> (quad loads) and gat_bwd_col_kernel<32,1,false,4>
    (quad loads at PYGAT_K4_QUAD_LOADS=2 only)."""
    rowptr, col = one_hub()
    N, Hh = len(rowptr) - 1, 6
    g = pg.CSRGraph(torch.as_tensor(rowptr, device="cuda:0"), torch.as_tensor(col, device="cuda:0"), slot_edges=slot)
    gen = torch.Generator().manual_seed(19)
    W = torch.randn(Hh, FIN, FO, generator=gen, dtype=torch.float64) * (1.414 * (2.0 / (FIN + FO)) ** 0.5)
    a = torch.randn(Hh, 2 * FO, generator=gen, dtype=torch.float64) * (1.414 * (2.0 / (1 + 2 * FO)) ** 0.5)
    x = torch.randn(N, FIN, dtype=torch.float64, generator=gen)
    G = torch.randn(N, Hh * FO, dtype=torch.float64, generator=gen)
    first = run_level(pg, g, x, W, a, G)
    again = run_level(pg, g, x, W, a, G)
    for t, u, what in zip(first, again, ("out", "dW", "da")):
        assert torch.equal(t, u), f"6 x 16, slot {slot}: {what} differs between two runs"
    out, dW, da = first
    check_level(out, {"dX": None, "dW": dW, "da": da}, x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, True, G.numpy(), None,
                what=f"6 x 16 on one_hub, {slot}-edge slots")
