"""pygat_amd.dot_attention with a per-entry bias on the score (the BIAS instantiations of csrc/k19_dot_attention.hip): out, dq, dk, dv
and db, the gradient of the bias.

Ground truth, inputs and the seeded cases live in dot_attention_bias_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>,
pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad).  Every case is rehearsed on the CPU, the
fp32 ground-truth run standing in for the device, by tests/test_dot_attention_bias_abi.py and passes there; no case is built here."""
import itertools

import pytest
import torch

import dot_attention_bias_case as case
from pattern_device import BFWD, BROWS, DEV, FWD, ROWS, SPMM, _pattern, degree, device_run, no_scratch, spied, two_runs_bit_equal

pytestmark = pytest.mark.gpu

K19B = [f"k19b_{d}_{kind}_l{l}v{v}" for d in ("fwd", "bwd") for kind in ("long", "row")
        for l, v in ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))]


def _fused(pattern, c):
    import pygat_amd as pg
    if c.fed_scale is None:
        return lambda q, k, v, b: pg.dot_attention(pattern, q, k, v, bias=b)
    return lambda q, k, v, b: pg.dot_attention(pattern, q, k, v, c.fed_scale, b)


def _from_parts(pattern, c):
    import pygat_amd as pg
    return lambda q, k, v, b: pg.spmm(pattern, pg.edge_softmax(pattern, pg.edge_dot(pattern, q, k, c.scale) + b), v)


def _unbiased(pattern, c):
    """The op without a bias, on a case of dot_attention_case."""
    import pygat_amd as pg
    return lambda q, k, v: pg.dot_attention(pattern, q, k, v) if c.fed_scale is None else pg.dot_attention(pattern, q, k, v, c.fed_scale)


def _device_run(pattern, c, fn=None):
    """-> (out, dq, dk, dv, db) on the device."""
    return device_run(pattern, c, fn or _fused)


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price(*res)
    return (c,) + res


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-") + case.case_names("shared-"))
def test_lane_shapes(name):
    """Every lane shape with a [E, H] bias ~ N(0, 1), with and without a permutation; tensors without a head axis with a [E] bias;
    a [E] bias shared by H > 1 heads (a head stride of 0), whose gradient is the sum over the heads."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks under a bias of std 3 on scores of std 1 / sqrt(F) ... 1: the bias decides which
    entries dominate a hub row, so a bias read at the wrong entry in the long-row launch, or a wrong merge of the records, moves out
    far beyond 1e-5."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("rect-") + case.case_names("repeats-"))
def test_unsorted_entries_take_their_own_bias(name):
    """Unsorted entries (only the permutation puts a bias on its entry), a rectangular pattern with empty rows and columns, repeated
    (row, col) pairs whose two entries carry different biases."""
    c, out, dq, dk, dv, db = _run_case(name)
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    if name.startswith("rect-"):
        assert int(no_row.sum()) == 100
        assert float(out[no_row].abs().max()) == 0.0 and float(dq[no_row].abs().max()) == 0.0


@pytest.mark.parametrize("name", case.case_names("masked-"))
def test_a_masked_entry_is_exactly_out(name):
    """bias = -9e15 on a third of the entries, every row keeping its first: priced as usual, and db at the masked entries is 0.0."""
    c, out, dq, dk, dv, db = _run_case(name)
    c.check_masked(db)
    assert float(db.abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    c, out, dq, dk, dv, db = _run_case(name)
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    assert torch.equal(out[rows], c.v.float().to(DEV)[cols]), "out_i == v_j bit for bit"
    assert float(dq[rows].abs().max()) == 0.0
    assert float(db[single.to(DEV)].abs().max()) == 0.0, "the one coefficient of a row is 1 whatever its bias"
    assert bool((dq[(deg > 1).to(DEV)].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("zero-"))
def test_a_bias_of_zeros_changes_no_bit(name):
    """out, dq, dk and dv under a bias of zeros are bit-equal to the op without a bias on the same inputs: the biased kernels take the
    difference score - (m - bias) where the unbiased ones take score - m, and form ds as the unbiased ones do."""
    c, out, dq, dk, dv, db = _run_case(name)
    want = device_run(_pattern(c), c.inner, _unbiased)
    for got, ref, what in zip((out, dq, dk, dv), want, ("out", "dq", "dk", "dv")):
        assert torch.equal(got, ref), (name, what)


def test_a_shift_per_row_leaves_the_row_sums_of_db_at_zero():
    """bias b against b + c[row, head]: both price against their own ground truth, and db sums to 0 over every row within
    max(1e-5, 4 x the largest such sum of the fp32 ground-truth run) -- the rule of test_gpu_dot_attention.py::test_long_rows."""
    for name in case.case_names("shift-"):
        c, out, dq, dk, dv, db = _run_case(name)
        own = float(c.db_row_sums(c.stand_in()[4]).abs().max())
        e = float(c.db_row_sums(db).abs().max())
        print(name, f"row sums of db off by {e:.2e} (fp32 ground truth {own:.2e})")
        assert e <= max(1e-5, 4.0 * own), (name, e, own)


@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    assert len(two_runs_bit_equal(case.cases()[name], _device_run)) == 5


@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax(edge_dot(q, k, scale) + bias), v) on the device and the fused op: both pass against the same fp64 run."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("module-"))
def test_in_a_module(name):
    """Three nn.Linear projections, bias = nn.Embedding(edge_type), dot_attention, a sum: out and the gradients that reach x, the three
    weights and the embedding table."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda q, k, v, b: pg.dot_attention(pattern, q, k, v, bias=b)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x = c.x.float().to(DEV).requires_grad_(True)
    out = module(x)
    out.sum().backward()
    c.price(out.detach(), x.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in (c.q, c.k, c.v, c.bias)]
    pattern = _pattern(c)
    with torch.no_grad():
        pg.dot_attention(pattern, *tensors[:3], bias=tensors[3])
    assert seen == [BFWD] and not pattern.has_transpose
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.dot_attention(pattern, *leaves[:3], bias=leaves[3])
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        assert seen == [BFWD, BROWS] + [SPMM] * (needs[1] + needs[2]), (needs, seen)
        assert pattern.has_transpose == (needs[1] or needs[2]), "neither dq nor db builds the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
    # without a bias: the entry points of the op as it was
    del seen[:]
    leaves = [t.clone().requires_grad_(True) for t in tensors[:3]]
    torch.autograd.grad(pg.dot_attention(pattern, *leaves), leaves, G)
    assert seen == [FWD, ROWS, SPMM, SPMM]
    del seen[:]
    torch.autograd.grad(pg.dot_attention(pattern, *leaves, None, None), leaves, G)
    assert seen == [FWD, ROWS, SPMM, SPMM]
    # no entries: zeros of the right shape and an empty db, from the row passes alone
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    q0, k0, v0 = (torch.randn(n, 2, 8, device=DEV, requires_grad=True) for n in (5, 7, 7))
    for shape in ((0, 2), (0,)):
        b0 = torch.zeros(shape, device=DEV, requires_grad=True)
        del seen[:]
        out = pg.dot_attention(empty, q0, k0, v0, bias=b0)
        grads = torch.autograd.grad(out, [q0, k0, v0, b0], torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, (q0, k0, v0, b0))) and grads[3].numel() == 0
        assert all(float(g.abs().max()) == 0.0 for g in grads[:3])
        assert seen == [BFWD, BROWS, SPMM, SPMM], seen            # (the two SpMMs write the zeros of dk and dv, as without a bias)


def test_refusals(monkeypatch):
    import copy
    import importlib
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    q, k, v = t(N, 4, 16), t(N, 4, 16), t(N, 4, 16)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    for args, bias, needle in (((pattern, q, k, v), [0.0] * E, "bias must be a tensor on the GPU"),
                               ((pattern, q, k, v), torch.zeros(E, 4), "bias must be a tensor on the GPU"),
                               ((pattern, q, k, v), t(E, 4).double(), "bias must be float32, not torch.float64"),
                               ((pattern, q, k, v), t(E, 4).half(), "bias must be float32"),
                               ((elsewhere, q, k, v), t(E, 4), "bias lives on cuda:0, the pattern on cuda:1"),
                               ((pattern, q, k, v), t(E, 8), f"[E, H] = [{E}, 4] or [E] = [{E}] expected"),
                               ((pattern, q, k, v), t(E, 8), f"got ({E}, 8)"),
                               ((pattern, q, k, v), t(E + 1, 4), f"got ({E + 1}, 4)"),
                               ((pattern, q, k, v), t(E - 1), f"got ({E - 1},)"),
                               ((pattern, q, k, v), t(E, 4, 1), f"got ({E}, 4, 1)"),
                               ((pattern, q, k, v), t(4, E), f"got (4, {E})"),
                               ((pattern, q, k, v), t(E, 1), f"got ({E}, 1)"),
                               ((pattern, q[:, 0], k[:, 0], v[:, 0]), t(E, 1), f"bias [E] = [{E}] expected")):
        with pytest.raises(ValueError, match="dot_attention.*bias") as err:
            pg.dot_attention(*args, bias=bias)
        assert needle in str(err.value), (needle, str(err.value))
    for args, needle in (((pattern, q.cpu(), k, v), "q must be a tensor on the GPU"), ((pattern, q, k, t(N, 4, 12)), "does not match q")):
        with pytest.raises(ValueError, match="dot_attention") as err:         # what the op refuses without a bias, it refuses with one
            pg.dot_attention(*args, bias=t(E, 4))
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient is refused as it is without a bias
    mod = importlib.import_module("pygat_amd.dot_attention")
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, t(E, 4))]
    out = pg.dot_attention(pattern, *leaves[:3], bias=leaves[3])
    del seen[:]
    with pytest.raises(ValueError, match="dot_attention.*float32"):
        mod._DotAttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_biased_kernels_have_no_scratch():
    assert len(K19B) == 40
    no_scratch(K19B, (b"k19b_fwd_row_l3v1", b"k19b_fwd_row_l32v2", b"k19b_fwd_row_l64v5", b"k19b_mid_row_l8v1", b"k19b_fwd_row_l8v1x",
                      b"k19b_", b"k19b", b"k19bfwd_row_l8v1", b"k19c_fwd_row_l8v1"))
