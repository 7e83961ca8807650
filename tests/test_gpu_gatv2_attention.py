"""pygat_amd.gatv2_attention (csrc/k21_gatv2_attention.hip, pygat_amd/gatv2_attention.py): softmax(a . LeakyReLU(x_dst_i + x_src_j))-
weighted sums of v_j over the entries of every row of a pattern, per head, fused; its gradients in x_dst, x_src, a and v.

Ground truth, inputs and the seeded cases live in gatv2_attention_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>, pricing
by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad); the level case by parity.check_level_v2.  Every
seeded case is rehearsed on the CPU, the fp32 ground-truth run standing in for the device, by tests/test_gatv2_attention_abi.py and
passes there; no case is built here."""
import copy
import importlib
import itertools

import pytest
import torch

import gatv2_attention_case as case
from pattern_device import DEV, _graph, _pattern, degree, device_run, no_scratch, spied, two_runs_bit_equal
from pattern_device import leaves as _leaves

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K21 = ([f"{prefix}_{d}_{kind}_l{l}v{v}" for prefix in ("k21", "k21s") for d in ("fwd", "bwd") for kind in ("long", "row") for l, v in SHAPES]
       + [f"k21_col_{kind}_l{l}v{v}" for kind in ("long", "row") for l, v in SHAPES] + ["k21_da_stage", "k21_da_final"])
FWD, ROWS, COLS, SPMM = "pygat_v2_attn_forward", "pygat_v2_attn_backward_rows", "pygat_v2_attn_backward_cols", "pygat_spmm_forward"


def _fused(pattern, c):
    import pygat_amd as pg
    return lambda x_dst, x_src, a, v=None: pg.gatv2_attention(pattern, x_dst, x_src, a, v, c.slope)


def _from_parts(pattern, c):
    import pygat_amd as pg
    row, col = c.row.to(DEV), c.col.to(DEV)

    def run(x_dst, x_src, a, v=None):
        e = (a * torch.nn.functional.leaky_relu(x_dst[row] + x_src[col], c.slope)).sum(-1)
        return pg.spmm(pattern, pg.edge_softmax(pattern, e), x_src if v is None else v)
    return run


def _device_run(pattern, c, fn=None, leaves=None):
    """-> (out, dx_dst, dx_src, da[, dv]) on the device."""
    return device_run(pattern, c, fn or _fused, leaves)


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price_all(*res)
    return (c,) + res


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-"))
def test_lane_shapes(name):
    """Every lane shape -- 1 to 256 chunks of 4 floats per row: LPR 1..64 with idle lanes at 6, 24 and 48 chunks, VEC 2, 3 and 4, one
    head on the whole wave -- and tensors without a head axis, on the hub pattern (a row and a column of 699 entries: the long
    launches of all three passes) and the asymmetric one (rows of one entry); "indices" patterns carry a permutation, "graph"
    patterns none; v shared (v=None) and separate."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("long"))
def test_long_rows_and_long_columns(name):
    """Every slot of a chunk and a row of three chunks, and the same patterns with rows and columns swapped: scores of std 3, so a few
    entries dominate a hub row and a wrong merge of the (m, Z, acc) records or of the dx records moves the result far beyond 1e-5."""
    _run_case(name)


# ------------------------------------------------------------------------------------------------- rectangular, unsorted, repeats
@pytest.mark.parametrize("name", case.case_names("rect-"))
def test_rectangular_with_empty_rows_and_columns(name):
    """A row without entries gives exact zeros in out and dx_dst; a column without entries in dx_src (and dv)."""
    res = _run_case(name)
    c, out, dd, ds = res[:4]
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    no_col = (torch.bincount(c.col, minlength=c.shape[1]) == 0).to(DEV)
    assert int(no_row.sum()) == 100 and int(no_col.sum()) == 125
    for t in (out[no_row], dd[no_row], ds[no_col]) + ((res[5][no_col],) if not c.shared else ()):
        assert float(t.abs().max()) == 0.0
    assert bool((out[~no_row].abs().amax(dim=(1, 2)) > 0.0).all())


def test_rows_and_columns_without_entries_at_the_end():
    """The column kernel's last work-group takes the columns behind the last entry; they and the rows behind it get exact zeros."""
    c, out, dd, ds, da = _run_case("tail-rect-3x8-shared")
    assert float(out[300:].abs().max()) == 0.0 and float(dd[300:].abs().max()) == 0.0 and float(ds[500:].abs().max()) == 0.0
    assert float(ds[:500].abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("repeats-"))
def test_repeated_pairs_are_separate_entries(name):
    """Unsorted entries, 5 % of them repeated: each repeat is an entry of its own."""
    c = _run_case(name)[0]
    assert c.pairs.shape[0] > 100 and torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]])
    assert torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])


# ----------------------------------------------------------------------------------------------------------------- exact results
@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    c, out, dd = _run_case(name)[:3]
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    v = (c.x_src if c.shared else c.v).float().to(DEV)
    assert torch.equal(out[rows], v[cols]), "out_i == v_j bit for bit"
    assert float(dd[rows].abs().max()) == 0.0, "the one S of the row is an exact zero, and dx_dst_i with it"
    assert bool((dd[(deg > 1).to(DEV)].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("slope-"))
def test_slopes(name):
    """Slopes 0.2, 0 and 1; at slope 1 the result is priced against the linear score's ground truth as well (price_all)."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("same-"))
def test_shared_against_a_copy_of_x_src(name):
    """v=None and v=x_src.clone(): out, dx_dst and da are the same bits; dx_src of the first is dx_src + dv of the second, priced by
    the parity rule against the fp64 run (in the shared run autograd adds the two parts, so the sum is what it returns)."""
    import pygat_amd as pg
    c, out, dd, ds, da = _run_case(name)
    assert c.shared
    pattern = _pattern(c)
    x_dst, x_src, a = _leaves(c)
    v = x_src.detach().clone().requires_grad_(True)
    out2 = pg.gatv2_attention(pattern, x_dst, x_src, a, v, c.slope)
    dd2, ds2, da2, dv2 = torch.autograd.grad(out2, [x_dst, x_src, a, v], c.G.float().to(DEV))
    for got, ref, what in ((out, out2.detach(), "out"), (dd, dd2, "dx_dst"), (da, da2, "da")):
        assert torch.equal(got, ref), (name, what)
    c.price(out2.detach(), dd2, ds2 + dv2, da2, what=name + " separate, dx_src + dv")


@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    """out and every gradient, da -- the staged reduce of per-wave records -- included; a hub case and long-column cases."""
    c = case.cases()[name]
    assert len(two_runs_bit_equal(c, _device_run)) == 1 + len(c.names)


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax((a * leaky_relu(x_dst[row] + x_src[col])).sum(-1)), v) on the device and the fused op: both pass against the
    same fp64 run."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("level-"))
def test_the_references_layer_from_the_op(name):
    """SpGraphAttentionLayerV2 (layers.py:270-300) on a square graph: Whi and Whj by torch matmul of x with W[:Fin] and W[Fin:] on the
    device, zero-padded from F = 6 to 8 columns (a too), elu(gatv2_attention(pattern, Whi, Whj, a, v=Whi)), loss <out, G>: out, dW, da
    and dX by parity.check_level_v2, unchanged; the same inputs through gatv2_level by the same rule."""
    import pygat_amd as pg
    c = case.cases()[name]
    graph = _graph(*c.csr)
    pattern = graph.edge_pattern()
    G = c.G.float().to(DEV)
    pad = lambda t: torch.nn.functional.pad(t, (0, c.FP - c.F))  # noqa: E731
    x, W, a = (t.float().to(DEV).requires_grad_(True) for t in (c.X, c.W, c.a))
    Whi, Whj = (torch.einsum("nk,hkf->nhf", x, part) for part in (W[:, :c.F_IN], W[:, c.F_IN:]))
    fused = pg.gatv2_attention(pattern, pad(Whi), pad(Whj), pad(a), v=pad(Whi), negative_slope=c.slope)
    assert fused.shape == (c.shape[0], c.H, c.FP) and float(fused.detach()[:, :, c.F:].abs().max()) == 0.0
    out = torch.nn.functional.elu(fused[:, :, :c.F]).reshape(c.shape[0], c.H * c.F)
    dX, dW, da = torch.autograd.grad(out, [x, W, a], G)
    c.price(out.detach(), dX, dW, da, name + " gatv2_attention")
    x2, W2, a2 = (t.float().to(DEV).requires_grad_(True) for t in (c.X, c.W, c.a))
    level = pg.GATv2LevelFn.apply(x2, W2, a2, None, graph, c.slope, True)
    dX2, dW2, da2 = torch.autograd.grad(level, [x2, W2, a2], G)
    c.price(level.detach(), dX2, dW2, da2, name + " gatv2_level")


@pytest.mark.parametrize("name", case.case_names("module-"))
def test_a_bipartite_gatv2_layer(name):
    """x_src [M, f_in] through W_l and x_dst [N, f_in] through W_r, one a, gatv2_attention with v=None over a rectangular pattern,
    ELU, a sum: out and the gradients that reach x_src, x_dst, W_l, W_r and a."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda h_dst, h_src, a: pg.gatv2_attention(pattern, h_dst, h_src, a, None, c.slope)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x_src, x_dst = (t.float().to(DEV).requires_grad_(True) for t in (c.x_src, c.x_dst))
    out = module(x_src, x_dst)
    out.sum().backward()
    c.price(out.detach(), x_src.grad, x_dst.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.gatv2_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def test_only_the_needed_launches(monkeypatch):
    """x_dst alone: the row pass, and the transposed pattern is never built; x_src or a: the column pass besides; v: K17 besides."""
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-separate"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]
    pattern = _pattern(c)
    with torch.no_grad():
        pg.gatv2_attention(pattern, *tensors[:3])
        pg.gatv2_attention(pattern, *tensors)
    assert seen == [FWD, FWD] and not pattern.has_transpose
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.gatv2_attention(pattern, *leaves, c.slope)
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        cols = needs[1] or needs[2]
        assert seen == [FWD, ROWS] + [COLS] * cols + [SPMM] * needs[3], (needs, seen)
        assert pattern.has_transpose == (cols or needs[3]), "dx_dst alone does not build the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
    # v=None: x_src is the value table too, so its gradient takes the column pass and K17; a alone takes the column pass only
    for needs, want in (((True, False, False), [FWD, ROWS]), ((False, True, False), [FWD, ROWS, COLS, SPMM]),
                        ((False, False, True), [FWD, ROWS, COLS])):
        pattern = _pattern(c)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors[:3], needs)]
        out = pg.gatv2_attention(pattern, *leaves, None, c.slope)
        torch.autograd.grad(out, [t for t, n in zip(leaves, needs) if n], G)
        assert seen == want and pattern.has_transpose == (len(want) > 2), (needs, seen)
    # no entries: zeros of the right shape, and nothing is launched
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    xd, xs, a0, v0 = (torch.randn(*dims, device=DEV, requires_grad=True) for dims in ((5, 2, 8), (7, 2, 8), (2, 8), (7, 2, 8)))
    for leaves in ([xd, xs, a0], [xd, xs, a0, v0]):
        del seen[:]
        out = pg.gatv2_attention(empty, *leaves)
        grads = torch.autograd.grad(out, leaves, torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, leaves)) and all(float(g.abs().max()) == 0.0 for g in grads)
        assert seen == [] and not empty.has_transpose, seen


def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-shared"]
    pattern = _pattern(c)
    N = c.shape[0]

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    xd, xs, a, v = t(N, 4, 16), t(N, 4, 16), t(4, 16), t(N, 4, 16)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    ok = (pattern, xd, xs, a)
    for args, kw, needle in (
            ((object(), xd, xs, a), {}, "an EdgePattern expected"),
            (ok, dict(negative_slope=float("nan")), "negative_slope = nan: a finite float expected"),
            (ok, dict(negative_slope=float("inf")), "negative_slope = inf"),
            (ok, dict(negative_slope="0.2"), "a finite float expected"),
            ((pattern, xd.cpu(), xs, a), {}, "x_dst must be a tensor on the GPU"),
            ((pattern, xd, [0.0] * N, a), {}, "x_src must be a tensor on the GPU"),
            ((pattern, xd, xs, a.cpu()), {}, "a must be a tensor on the GPU"),
            (ok, dict(v=v.double()), "v must be float32, not torch.float64"),
            ((pattern, xd, xs.half(), a), {}, "x_src must be float32"),
            ((pattern, xd, xs, a.bfloat16()), {}, "a must be float32, not torch.bfloat16"),
            ((elsewhere, xd, xs, a), {}, "x_dst lives on cuda:0, the pattern on cuda:1"),
            ((pattern, t(N), xs, a), {}, "x_dst [n_rows, F] or [n_rows, H, F] expected"),
            ((pattern, xd, t(N, 3, 16), a), {}, "x_src (%d, 3, 16) does not match x_dst" % N),
            ((pattern, xd, t(N, 16), a), {}, "does not match x_dst"),
            ((pattern, xd, xs, t(4, 8)), {}, "a (4, 8) does not match x_dst"),
            ((pattern, xd, xs, t(16)), {}, "a (16,) does not match x_dst"),
            (ok, dict(v=t(N, 4, 8)), "v (%d, 4, 8) does not match x_dst" % N),
            ((pattern, t(N + 1, 4, 16), xs, a), {}, f"x_dst has {N + 1} rows but the pattern has {N} rows"),
            ((pattern, xd, t(N - 1, 4, 16), a), {}, f"x_src has {N - 1} rows but the pattern has {N} columns"),
            (ok, dict(v=t(N + 2, 4, 16)), f"v has {N + 2} rows but the pattern has {N} columns"),
            ((pattern, t(N, 65, 4), t(N, 65, 4), t(65, 4)), {}, "H = 65 heads: the limits are 1 <= H <= 64"),
            ((pattern, t(N, 4, 12), t(N, 4, 12), t(4, 12)), {}, "F = 12: a head's width must be a power of two in 4..256; zero-pad the "
                                                                "columns of all four tensors"),
            ((pattern, t(N, 4, 12), t(N, 4, 12), t(4, 12)), {}, "zero columns of a add nothing to a score"),
            ((pattern, t(N, 4, 2), t(N, 4, 2), t(4, 2)), {}, "F = 2"),
            ((pattern, t(N, 512), t(N, 512), t(512)), {}, "F = 512"),
            ((pattern, t(N, 8, 256), t(N, 8, 256), t(8, 256)), {}, "H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024")):
        with pytest.raises(ValueError, match="gatv2_attention") as err:
            pg.gatv2_attention(*args, **kw)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient
    mod = importlib.import_module("pygat_amd.gatv2_attention")
    leaves = [x.clone().requires_grad_(True) for x in (xd, xs, a)]
    out = pg.gatv2_attention(pattern, *leaves)
    del seen[:]
    with pytest.raises(ValueError, match="gatv2_attention: the gradient of the output must be float32, not torch.float64"):
        mod._Gatv2AttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_no_kernel_uses_scratch():
    assert len(K21) == 102
    no_scratch(K21, (b"k21_fwd_row_l3v1", b"k21_fwd_row_l32v2", b"k21_fwd_row_l64v5", b"k21_mid_row_l8v1", b"k21_fwd_row_l8v1x", b"k21_",
                     b"k21", b"k21fwd_row_l8v1", b"k21b_fwd_row_l8v1", b"k21s_col_row_l8v1", b"k21s_bwd_row_l0v1", b"k21_da_stage_",
                     b"k21s_da_final", b"k21_col_mid_l8v1"))
