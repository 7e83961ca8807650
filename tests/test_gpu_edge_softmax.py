"""pygat_amd.edge_softmax (csrc/k18_edge_softmax.hip): the softmax of per-entry logits over the rows (columns) of a pattern, per head,
and its gradient.

Ground truth, inputs and the seeded cases live in edge_softmax_case.py: torch autograd in fp64 on the CPU, loss L = <alpha, G>, pricing
by parity.check_autograd unchanged (alpha by close_fwd, dlogits by close_grad).  Every seeded case is rehearsed on the CPU, the fp32
ground-truth run standing in for the device, by tests/test_edge_softmax_abi.py and passes there; no case is built here."""
import ctypes as C
import importlib

import pytest
import torch

import edge_softmax_case as case
import parity
from edge_softmax_case import edge_softmax_ref
from pattern_device import DEV, _graph
from pattern_graphs import SLOPE

pytestmark = pytest.mark.gpu

K18 = ["k18_rows_long_c1", "k18_rows_long_c4", "k18_rows_c1", "k18_rows_c4", "k18_grad_rows_long_c1", "k18_grad_rows_long_c4",
       "k18_grad_rows_c1", "k18_grad_rows_c4", "k18_apply", "k18_grad_apply"]


def _indices_pattern(row, col, shape):
    import pygat_amd as pg
    return pg.EdgePattern.from_indices(torch.stack([row, col]).to(DEV), shape)


def _pattern(c):
    if c.kind == "indices":
        return _indices_pattern(c.row, c.col, c.shape)
    pattern = _graph(*c.csr).edge_pattern()
    assert pattern.perm is None and torch.equal(pattern.edge_rc.cpu().long(), torch.stack([c.row, c.col], 1))
    return pattern


def _device_run(pattern, l, G, by="row"):
    """-> (alpha, dlogits) on the device."""
    import pygat_amd as pg
    ld = l.float().to(DEV).requires_grad_(True)
    alpha = pg.edge_softmax(pattern, ld, by)
    assert alpha.dtype == torch.float32 and alpha.shape == ld.shape and alpha.requires_grad
    (dl,) = torch.autograd.grad(alpha, [ld], G.float().to(DEV))
    return alpha.detach(), dl


def _run_case(name):
    c = case.cases()[name]
    alpha, dl = _device_run(_pattern(c), c.fed, c.G, c.by)
    rep, a64 = c.price(alpha, dl)
    return c, alpha, dl, a64


def _group_sums(c, alpha):
    a = alpha.detach().double().cpu().reshape(c.group.numel(), -1)
    return torch.zeros(c.n_groups, a.shape[1], dtype=torch.float64).index_add(0, c.group, a)


def _names(prefix):
    return [n for n in case.case_names() if n.startswith(prefix)]


# ------------------------------------------------------------------------------------------------------------------------ heads
@pytest.mark.parametrize("name", _names("heads-"))
def test_heads(name):
    """H in {1, 2, 3, 6, 8, 64} and logits without a head axis, on the hub pattern (a row of 699 entries: the long-row launches) and
    the asymmetric one; "indices" patterns carry a permutation, "graph" patterns none; 16-byte loads at H = 8 and 64, single floats
    at the other H."""
    _run_case(name)


# -------------------------------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("name", _names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks, logits N(0, 3^2): a few entries dominate a hub row, so a wrong merge of the
    (m, Z) records moves alpha far beyond 1e-5.  Every row's coefficients add up to 1."""
    c, alpha, _, _ = _run_case(name)
    own = float((_group_sums(c, edge_softmax_ref(c.group, c.n_groups, c.logits.float())) - 1.0).abs().max())
    e = float((_group_sums(c, alpha) - 1.0).abs().max())
    print(name, f"row sums off by {e:.2e} (fp32 ground truth {own:.2e})")
    assert e <= max(1e-5, 4.0 * own), (name, e, own)


# ---------------------------------------------------------------------------------------------------------------------- by="col"
@pytest.mark.parametrize("name", _names("col-"))
def test_by_col(name):
    """Grouped by column against the fp64 ground truth grouped by column; a graph's pattern brings its own transpose."""
    c, alpha, dl, _ = _run_case(name)
    if c.kind == "indices":        # the same walk as by="row" on the swapped index rows: both take a group's entries in the caller's order
        swapped = _indices_pattern(c.col, c.row, (c.shape[1], c.shape[0]))
        a2, d2 = _device_run(swapped, c.logits, c.G, "row")
        assert torch.equal(alpha, a2) and torch.equal(dl, d2)
        assert not swapped.has_transpose


# ------------------------------------------------------------------------------------------------- rectangular, unsorted, repeats
@pytest.mark.parametrize("name", _names("rect-"))
def test_rectangular_with_empty_rows_and_columns(name):
    c, alpha, dl, _ = _run_case(name)
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    sums = _group_sums(c, alpha)
    empty = torch.bincount(c.group, minlength=c.n_groups) == 0
    assert int(empty.sum()) in (100, 125)
    assert float((sums[~empty] - 1.0).abs().max()) <= 1e-5 and float(sums[empty].abs().max()) == 0.0


@pytest.mark.parametrize("name", _names("repeats-"))
def test_unsorted_entries_with_repeats(name):
    """A repeated (row, col) pair is two entries of the softmax, each with its own logit."""
    c, alpha, dl, a64 = _run_case(name)
    pairs = c.pairs
    assert pairs.shape[0] > 100 and bool((c.row[1:] < c.row[:-1]).any())
    assert torch.equal(c.row[pairs[:, 0]], c.row[pairs[:, 1]]) and torch.equal(c.col[pairs[:, 0]], c.col[pairs[:, 1]])
    assert not torch.equal(a64[pairs[:, 0]], a64[pairs[:, 1]])
    assert float((_group_sums(c, alpha)[torch.bincount(c.group, minlength=c.n_groups) > 0] - 1.0).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------------------------ exact cases
@pytest.mark.parametrize("name", _names("lonely-"))
def test_a_group_of_one_entry_is_exact(name):
    c, alpha, dl, _ = _run_case(name)
    single = (torch.bincount(c.row, minlength=c.shape[0]) == 1)[c.row].to(DEV)
    assert int(single.sum()) >= 12
    assert bool((alpha[single] == 1.0).all()) and bool((dl[single] == 0.0).all())
    assert bool((alpha[~single] < 1.0).all())


@pytest.mark.parametrize("name", _names("masked-"))
def test_masked_entries_are_exact_zeros(name):
    """The reference's mask value -9e15 (layers.py:40) among N(0, 1) logits: exactly 0 there, the rest of the row unharmed; in short
    rows and in the hub row of 699 entries (which goes through the (m, Z) records)."""
    c, alpha, dl, _ = _run_case(name)
    masked = c.masked.to(DEV)
    assert float(alpha[masked].abs().max()) == 0.0 and float(dl[masked].abs().max()) == 0.0
    assert float((_group_sums(c, alpha) - 1.0).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", _names("huge-"))
def test_rows_of_equal_huge_logits_are_uniform(name):
    """All logits of a row at 9e15: 1 / d, to within the rounding of one division."""
    c, alpha, dl, _ = _run_case(name)
    want = (1.0 / c.deg[c.row].double())[c.huge]
    got = alpha.double().cpu()[c.huge]
    assert float(((got - want[:, None]).abs() / want[:, None]).max()) <= 2.0 ** -23


@pytest.mark.parametrize("kind", ["indices", "graph"])
def test_a_constant_per_group_changes_nothing(kind):
    """Whole-number shifts per row of logits on a 2^-10 grid (edge_softmax_case._exact_cases): the exact softmax is the same, and
    the device's two results each lie within the parity tolerance of the one ground truth."""
    _, _, _, a64 = _run_case(f"grid-{kind}")
    c, alpha, _, _ = _run_case(f"shifted-{kind}")
    assert not torch.equal(c.fed, c.logits)
    parity.close_fwd(alpha, a64, "alpha of the shifted logits")


# ---------------------------------------------------------------------------------------------------------------- reproducible
@pytest.mark.parametrize("name", _names("twice-"))
def test_two_runs_are_bit_equal(name):
    c = case.cases()[name]
    pattern = _pattern(c)
    runs = [_device_run(pattern, c.fed, c.G, c.by) for _ in range(2)]
    for p, q in zip(*runs):
        assert torch.equal(p, q)
    c.price(*runs[0])


# ------------------------------------------------------------------------------------------------------------------ composition
def test_composition_is_the_reference_layer():
    """alpha = edge_softmax(pattern, logits), y = spmm(pattern, alpha, Wh): alpha is the level's own, y and the gradients through
    both ops agree with the fp64 torch spelling."""
    import pygat_amd as pg
    from alpha_grad_case import kink_count
    rowptr, col, x, W, a, logits, Wh, G = case.composition_inputs()
    assert kink_count(x, rowptr, col, W, a, SLOPE) == 0, "an input with a logit inside the kink band -- choose another seed"
    H = W.shape[0]
    graph = _graph(rowptr, col)
    pattern = graph.edge_pattern()
    ld, whd = logits.float().to(DEV).requires_grad_(True), Wh.float().to(DEV).requires_grad_(True)
    alpha = pg.edge_softmax(pattern, ld)
    y = pg.spmm(pattern, alpha, whd)
    grads = torch.autograd.grad(y, [ld, whd], G.float().to(DEV))
    _, level_alpha = pg.gat_level(x.to(DEV), graph, [W[h].to(DEV) for h in range(H)], [a[h].to(DEV) for h in range(H)], None, SLOPE,
                                  True, return_attention=True)
    e = float((alpha.detach() - level_alpha).abs().max())
    print(f"alpha against the level's: {e:.2e}")
    assert alpha.shape == level_alpha.shape and e <= 1e-5
    case.price_composition(y.detach(), grads, rowptr, col, logits, Wh, G)


# ---------------------------------------------------------------------------------------------------------- launches and refusals
class _Spy:
    def __init__(self, real, seen):
        self._real, self._seen = real, seen

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("pygat_") or name == "pygat_last_error":
            return fn

        def wrapped(*args):
            self._seen.append(name)
            return fn(*args)
        return wrapped


def _spied(monkeypatch):
    mod = importlib.import_module("pygat_amd.edge_softmax")       # (the package attribute of that name is the function)
    seen = []
    monkeypatch.setattr(mod, "lib", _Spy(mod.lib, seen))
    return seen


FWD = ["pygat_edge_softmax_rows", "pygat_edge_softmax_apply"]
BWD = ["pygat_edge_softmax_grad_rows", "pygat_edge_softmax_grad_apply"]


def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["col-asym-H8-indices"]
    pattern = _pattern(c)
    ld = c.logits.float().to(DEV)
    with torch.no_grad():
        pg.edge_softmax(pattern, ld)
    assert seen == FWD and not pattern.has_transpose
    del seen[:]
    _device_run(pattern, c.logits, c.G, "row")
    assert seen == FWD + BWD and not pattern.has_transpose, "by=\"row\" never builds the transpose"
    del seen[:]
    _device_run(pattern, c.logits, c.G, "col")
    assert seen == FWD + BWD and pattern.has_transpose
    # no entries: an empty tensor, nothing launched, forward or backward
    del seen[:]
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    for shape in ((0,), (0, 3)):
        for by in ("row", "col"):
            l0 = torch.zeros(shape, device=DEV, requires_grad=True)
            out = pg.edge_softmax(empty, l0, by)
            (d0,) = torch.autograd.grad(out, [l0], torch.zeros(shape, device=DEV))
            assert out.shape == shape and d0.shape == shape and out.dtype == torch.float32
    assert seen == [] and not empty.has_transpose


def test_refusals(monkeypatch):
    import copy
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["col-asym-H8-indices"]
    pattern = _pattern(c)
    E = c.row.numel()
    l = torch.rand(E, 4, device=DEV)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    for args, needle in (((object(), l), "EdgePattern"), ((pattern, l.cpu()), "GPU"), ((pattern, l.double()), "float32"),
                         ((pattern, l.half()), "float32"), ((elsewhere, l), "cuda:1"), ((pattern, l[:-1]), f"{E - 1} rows"),
                         ((pattern, l[:, :, None]), "expected"), ((pattern, l.sum()), "expected"),
                         ((pattern, torch.rand(E, 65, device=DEV)), "H = 65"), ((pattern, torch.rand(E, 0, device=DEV)), "H = 0"),
                         ((pattern, l, "rows"), "by must be"), ((pattern, l, None), "by must be")):
        with pytest.raises(ValueError, match="edge_softmax") as err:
            pg.edge_softmax(*args)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    ld = l.clone().requires_grad_(True)
    out = pg.edge_softmax(pattern, ld)
    del seen[:]
    with pytest.raises(ValueError, match="edge_softmax.*float32"):
        importlib.import_module("pygat_amd.edge_softmax")._EdgeSoftmaxFn.backward(out.grad_fn, torch.ones(E, 4, device=DEV, dtype=torch.float64))
    assert seen == []


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_new_kernels_have_no_scratch():
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    for name in K18:
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and 0 < regs.value <= 128, (name, regs.value, scratch.value)
    for bad in (b"k18_rows_c2", b"k18_apply_c4", b"k18_rows_c4x", b"k18_"):
        assert lib.pygat_kernel_footprint(bad, C.byref(regs), C.byref(scratch)) == -1, bad
