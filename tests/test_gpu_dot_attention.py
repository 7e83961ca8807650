"""pygat_amd.dot_attention and pygat_amd.edge_dot (csrc/k19_dot_attention.hip, pygat_amd/dot_attention.py): softmax(scale q_i . k_j)
-weighted sums of v_j over the entries of every row of a pattern, per head, fused; its score as an op of its own; their gradients.

Ground truth, inputs and the seeded cases live in dot_attention_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>, pricing
by parity.check_autograd unchanged (out by close_fwd, dq, dk, dv by close_grad).  Every seeded case is rehearsed on the CPU, the fp32
ground-truth run standing in for the device, by tests/test_dot_attention_abi.py and passes there; no case is built here."""
import importlib

import pytest
import torch

import dot_attention_case as case
import parity
from edge_softmax_case import edge_softmax_ref
from pattern_device import DEV, FWD, ROWS, SDDMM, SPMM, _pattern, degree, device_run, no_scratch, spied, to_leaves, two_runs_bit_equal

pytestmark = pytest.mark.gpu

K19 = [f"k19_{d}_{kind}_l{l}v{v}" for d in ("fwd", "bwd") for kind in ("long", "row")
       for l, v in ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))]


def _fused(pattern, c):
    import pygat_amd as pg
    return lambda q, k, v: pg.dot_attention(pattern, q, k, v) if c.fed_scale is None else pg.dot_attention(pattern, q, k, v, c.fed_scale)


def _from_parts(pattern, c):
    import pygat_amd as pg
    return lambda q, k, v: pg.spmm(pattern, pg.edge_softmax(pattern, pg.edge_dot(pattern, q, k, c.scale)), v)


def _device_run(pattern, c, fn=None):
    """-> (out, dq, dk, dv) on the device."""
    return device_run(pattern, c, fn or _fused)


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    _, y64 = c.price(*res)
    return (c,) + res + (y64,)


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-") + case.case_names("sharp-"))
def test_lane_shapes(name):
    """Every lane shape -- 1 to 256 chunks of 4 floats per row: LPR 1..64 with idle lanes at 6, 24 and 48 chunks, VEC 2, 3 and 4, one
    head on the whole wave -- and tensors without a head axis, on the hub pattern (a row of 699 entries: the long-row launches) and
    the asymmetric one (rows of one entry); "indices" patterns carry a permutation, "graph" patterns none."""
    _run_case(name)


# -------------------------------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("name", case.case_names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks, scores of std 3: a few entries dominate a hub row, so a wrong merge of the
    (m, Z, acc) records moves out far beyond 1e-5.  The coefficients the row pass implies -- edge_softmax of edge_dot, on the device
    -- add up to 1 in every row."""
    import pygat_amd as pg
    c = _run_case(name)[0]
    pattern = _pattern(c)
    qd, kd = c.q.float().to(DEV), c.k.float().to(DEV)
    alpha = pg.edge_softmax(pattern, pg.edge_dot(pattern, qd, kd, c.scale))

    def sums(a):
        return torch.zeros(c.shape[0], c.H, dtype=torch.float64).index_add(0, c.row, a.detach().double().cpu())
    own = float((sums(edge_softmax_ref(c.row, c.shape[0], c.scores(torch.float32))) - 1.0).abs().max())
    e = float((sums(alpha) - 1.0).abs().max())
    print(name, f"row sums off by {e:.2e} (fp32 ground truth {own:.2e})")
    assert e <= max(1e-5, 4.0 * own), (name, e, own)


# ----------------------------------------------------------------------------------------------------------------- exact scores
@pytest.mark.parametrize("name", case.case_names("exact-"))
def test_whole_number_scores(name):
    """q and k on an integer grid, scale 1: every score is exact in any summation order, so the online rescale and the record merge
    are priced without score rounding in the way."""
    _run_case(name)


# ------------------------------------------------------------------------------------------------- rectangular, unsorted, repeats
@pytest.mark.parametrize("name", case.case_names("rect-"))
def test_rectangular_with_empty_rows_and_columns(name):
    c, out, dq, dk, dv, _ = _run_case(name)
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    no_col = (torch.bincount(c.col, minlength=c.shape[1]) == 0).to(DEV)
    assert int(no_row.sum()) == 100 and int(no_col.sum()) == 125
    for t in (out[no_row], dq[no_row], dk[no_col], dv[no_col]):
        assert float(t.abs().max()) == 0.0
    assert bool((out[~no_row].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("repeats-"))
def test_unsorted_entries_with_repeats(name):
    """A repeated (row, col) pair is two entries of the softmax (the ground truth counts it twice; the pricing would not pass
    otherwise)."""
    c = _run_case(name)[0]
    pairs = c.pairs
    assert pairs.shape[0] > 100 and bool((c.row[1:] < c.row[:-1]).any())
    assert torch.equal(c.row[pairs[:, 0]], c.row[pairs[:, 1]]) and torch.equal(c.col[pairs[:, 0]], c.col[pairs[:, 1]])


# -------------------------------------------------------------------------------------------------------------- one-entry rows
@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    c, out, dq, dk, dv, _ = _run_case(name)
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    assert torch.equal(out[rows], c.v.float().to(DEV)[cols]), "out_i == v_j bit for bit"
    assert float(dq[rows].abs().max()) == 0.0
    assert bool((dq[(deg > 1).to(DEV)].abs().amax(dim=(1, 2)) > 0.0).all())


# ---------------------------------------------------------------------------------------------------------------- reproducible
@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    two_runs_bit_equal(case.cases()[name], _device_run)


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax(edge_dot(q, k, scale)), v) and dot_attention on the same inputs: both pass the pricing against the same
    fp64 run, outputs and all three gradients."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("dot-"))
def test_edge_dot(name):
    """The score alone against (q[row] * k[col]).sum(-1) * scale: 16-byte lanes at 8x16, the single-float path of the SDDMM at 3x7,
    tensors without a head axis."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    qd, kd = to_leaves(c.leaves)
    u = pg.edge_dot(pattern, qd, kd, c.fed_scale)
    assert u.dtype == torch.float32 and u.shape == c.G.shape and u.requires_grad
    c.price(u.detach(), *torch.autograd.grad(u, [qd, kd], c.G.float().to(DEV)))


# ------------------------------------------------------------------------------------------------------------------ in a module
@pytest.mark.parametrize("name", case.case_names("module-"))
def test_in_a_module(name):
    """Three nn.Linear projections, dot_attention, a sum: out and the gradients that reach x and the three weights."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda q, k, v: pg.dot_attention(pattern, q, k, v)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x = c.x.float().to(DEV).requires_grad_(True)
    out = module(x)
    out.sum().backward()
    c.price(out.detach(), x.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    G = c.G.float().to(DEV)
    with torch.no_grad():
        pg.dot_attention(pattern, *[t.float().to(DEV) for t in (c.q, c.k, c.v)])
    assert seen == [FWD] and not pattern.has_transpose
    for needs, want in (((True, False, False), [FWD, ROWS]), ((True, True, True), [FWD, ROWS, SPMM, SPMM]),
                        ((False, True, False), [FWD, ROWS, SPMM]), ((False, False, True), [FWD, ROWS, SPMM])):
        del seen[:]
        leaves = [t.float().to(DEV).requires_grad_(n) for t, n in zip((c.q, c.k, c.v), needs)]
        out = pg.dot_attention(pattern, *leaves)
        grads = torch.autograd.grad(out, [t for t, n in zip(leaves, needs) if n], G)
        assert seen == want, (needs, seen)
        assert pattern.has_transpose == (needs != (True, False, False)), "dq alone never builds the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, [t for t, n in zip(leaves, needs) if n]))
    # edge_dot: the SDDMM forward, one SpMM per gradient asked for
    c = case.cases()["dot-hub-8x16-indices"]
    pattern = _pattern(c)
    Gd = c.G.float().to(DEV)
    for needs, want in (((True, False), [SDDMM, SPMM]), ((False, True), [SDDMM, SPMM]), ((True, True), [SDDMM, SPMM, SPMM])):
        del seen[:]
        leaves = [t.float().to(DEV).requires_grad_(n) for t, n in zip((c.q, c.k), needs)]
        u = pg.edge_dot(pattern, *leaves, c.fed_scale)
        torch.autograd.grad(u, [t for t, n in zip(leaves, needs) if n], Gd)
        assert seen == want, (needs, seen)
        assert pattern.has_transpose == needs[1], "dq alone never builds the transpose"
    # no entries: zeros of the right shape from the row pass alone, and empty scores with nothing launched
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    q0, k0, v0 = (torch.randn(n, 2, 8, device=DEV, requires_grad=True) for n in (5, 7, 7))
    out = pg.dot_attention(empty, q0, k0, v0)
    grads = torch.autograd.grad(out, [q0, k0, v0], torch.ones_like(out))
    assert out.shape == (5, 2, 8) and float(out.abs().max()) == 0.0
    assert all(g.shape == t.shape and float(g.abs().max()) == 0.0 for g, t in zip(grads, (q0, k0, v0)))
    del seen[:]
    assert pg.edge_dot(empty, q0, k0).shape == (0, 2) and seen == []


def test_refusals(monkeypatch):
    import copy
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    N = c.shape[0]

    def t(rows, *dims, **kw):
        return torch.rand(rows, *dims, device=DEV, **kw)
    q, k, v = t(N, 4, 16), t(N, 4, 16), t(N, 4, 16)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    for args, needle in (((object(), q, k, v), "EdgePattern"), ((pattern, q.cpu(), k, v), "q must be a tensor on the GPU"),
                         ((pattern, q, k, v.cpu()), "v must be a tensor on the GPU"), ((pattern, q.double(), k, v), "q must be float32"),
                         ((pattern, q, k.half(), v), "k must be float32"), ((elsewhere, q, k, v), "cuda:1"),
                         ((pattern, t(N, 4, 3), t(N, 4, 3), t(N, 4, 3)), "F = 3"),
                         ((pattern, t(N, 4, 12), t(N, 4, 12), t(N, 4, 12)), "F = 12"),
                         ((pattern, t(N, 1, 512), t(N, 1, 512), t(N, 1, 512)), "F = 512"),
                         ((pattern, t(N, 65, 4), t(N, 65, 4), t(N, 65, 4)), "H = 65"),
                         ((pattern, t(N, 8, 256), t(N, 8, 256), t(N, 8, 256)), "H * F = 8 * 256 = 2048"),
                         ((pattern, q, k, t(N, 4, 32)), "v (500, 4, 32) does not match q"),
                         ((pattern, q, k, t(N + 1, 4, 16)), f"v has {N + 1} rows but the pattern has {N} columns"),
                         ((pattern, t(N - 1, 4, 16), k, v), f"q has {N - 1} rows but the pattern has {N} rows"),
                         ((pattern, q, t(N + 2, 4, 16), t(N + 2, 4, 16)), f"k has {N + 2} rows but the pattern has {N} columns"),
                         ((pattern, q, t(N, 8, 16), t(N, 8, 16)), "the same number of heads"),
                         ((pattern, q[:, 0], k, v), "does not match q"), ((pattern, q.sum(), k, v), "expected")):
        with pytest.raises(ValueError, match="dot_attention") as err:
            pg.dot_attention(*args)
        assert needle in str(err.value), (needle, str(err.value))
    for F in (3, 12, 512):                                        # the way out is named: pad the columns with zeros
        with pytest.raises(ValueError, match="zero-padding the columns of q, k and v to the next allowed F"):
            pg.dot_attention(pattern, t(N, 1, F), t(N, 1, F), t(N, 1, F))
    for args, needle in (((object(), q, k), "EdgePattern"), ((pattern, q.cpu(), k), "GPU"), ((pattern, q, k.double()), "float32"),
                         ((pattern, t(N, 65, 4), t(N, 65, 4)), "H = 65"), ((pattern, t(N, 2, 1024), t(N, 2, 1024)), "H * F <= 1024"),
                         ((pattern, q, t(N, 8, 16)), "the same number of heads"), ((pattern, q, t(N + 1, 4, 16)), "columns")):
        with pytest.raises(ValueError, match="edge_dot") as err:
            pg.edge_dot(*args)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient
    mod = importlib.import_module("pygat_amd.dot_attention")
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    out = pg.dot_attention(pattern, *leaves)
    u = pg.edge_dot(pattern, leaves[0], leaves[1])
    del seen[:]
    with pytest.raises(ValueError, match="dot_attention.*float32"):
        mod._DotAttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    with pytest.raises(ValueError, match="edge_dot.*float32"):
        mod._EdgeDotFn.backward(u.grad_fn, torch.ones(u.shape, device=DEV, dtype=torch.float64))
    assert seen == []


def test_zero_padded_columns_change_nothing():
    """What the refusal of F = 12 advises: q, k, v padded with zero columns to F = 16, the scale of F = 12 passed explicitly."""
    import math
    import pygat_amd as pg
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    q, k, v = (t.float().to(DEV).clone() for t in (c.q, c.k, c.v))
    for t in (q, k, v):
        t[:, :, 12:] = 0.0
    out = pg.dot_attention(pattern, q, k, v, 1.0 / math.sqrt(12))
    qs, ks, vs = (t[:, :, :12].double().cpu() for t in (q, k, v))
    want = case.dot_attention_ref(c.row, c.col, c.shape[0], qs, ks, vs, 1.0 / math.sqrt(12))
    own = case.dot_attention_ref(c.row, c.col, c.shape[0], qs.float(), ks.float(), vs.float(), 1.0 / math.sqrt(12))
    assert float(out[:, :, 12:].abs().max()) == 0.0
    parity.close_fwd(out[:, :, :12], want, "the first 12 columns", own)


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_new_kernels_have_no_scratch():
    assert len(K19) == 40
    no_scratch(K19, (b"k19_fwd_row_l3v1", b"k19_fwd_row_l32v2", b"k19_fwd_row_l64v5", b"k19_mid_row_l8v1", b"k19_fwd_row_l8v1x", b"k19_"))
