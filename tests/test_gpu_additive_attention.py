"""pygat_amd.additive_attention (csrc/k20_additive_attention.hip, pygat_amd/additive_attention.py): softmax(LeakyReLU(s_dst_i + s_src_j
(+ u_e)))-weighted sums of v_j over the entries of every row of a pattern, per head, fused; its gradients.

Ground truth, inputs and the seeded cases live in additive_attention_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>,
pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad).  Every seeded case is rehearsed on the CPU,
the fp32 ground-truth run standing in for the device, by tests/test_additive_attention_abi.py and passes there; no case is built here."""
import copy
import importlib
import itertools

import pytest
import torch

import additive_attention_case as case
from pattern_device import DEV, _graph, _pattern, degree, device_run, no_scratch, spied, two_runs_bit_equal
from pattern_device import leaves as _leaves

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K20 = [f"{prefix}_{d}_{kind}_l{l}v{v}" for prefix in ("k20", "k20u") for d in ("fwd", "bwd") for kind in ("long", "row") for l, v in SHAPES]
FWD, ROWS, SPMM = "pygat_add_attn_forward", "pygat_add_attn_backward_rows", "pygat_spmm_forward"


def _fused(pattern, c):
    import pygat_amd as pg
    return lambda s_dst, s_src, v, u=None: pg.additive_attention(pattern, s_dst, s_src, v, c.slope, u)


def _from_parts(pattern, c):
    import pygat_amd as pg
    row, col = c.row.to(DEV), c.col.to(DEV)

    def run(s_dst, s_src, v, u=None):
        z = s_dst[row] + s_src[col]
        if u is not None:
            z = z + (u[:, None] if u.dim() < z.dim() else u)
        return pg.spmm(pattern, pg.edge_softmax(pattern, torch.nn.functional.leaky_relu(z, c.slope)), v)
    return run


def _device_run(pattern, c, fn=None, leaves=None):
    """-> (out, ds_dst, ds_src, dv[, du]) on the device."""
    return device_run(pattern, c, fn or _fused, leaves)


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price(*res)
    return (c,) + res


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-"))
def test_lane_shapes(name):
    """Every lane shape -- 1 to 256 chunks of 4 floats per row: LPR 1..64 with idle lanes at 6, 24 and 48 chunks, VEC 2, 3 and 4, one
    head on the whole wave -- and tensors without a head axis, on the hub pattern (a row of 699 entries: the long-row launches) and
    the asymmetric one (rows of one entry); "indices" patterns carry a permutation, "graph" patterns none; without a logit, with a
    [E, H] one and with a [E] one shared by the heads, whose gradient is the sum over the heads."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks, s (and u) of std 3: a few entries dominate a hub row, so a wrong merge of the
    (m, Z, acc) records or of the dz records moves out and ds_dst far beyond 1e-5."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("exact-"))
def test_whole_number_scores(name):
    """s_dst, s_src and u on an integer grid (s_dst shifted by 1/4: no z is 0), slope 1/2: every l is exact, so the online rescale
    and the record merge are priced without score rounding in the way."""
    _run_case(name)


# ------------------------------------------------------------------------------------------------- rectangular, unsorted, repeats
@pytest.mark.parametrize("name", case.case_names("rect-"))
def test_rectangular_with_empty_rows_and_columns(name):
    c, out, dd, ds, dv = _run_case(name)[:5]
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    no_col = (torch.bincount(c.col, minlength=c.shape[1]) == 0).to(DEV)
    assert int(no_row.sum()) == 100 and int(no_col.sum()) == 125
    for t in (out[no_row], dd[no_row], ds[no_col], dv[no_col]):
        assert float(t.abs().max()) == 0.0
    assert bool((out[~no_row].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("repeats-"))
def test_repeated_pairs_are_separate_entries(name):
    """Unsorted entries, 5 % of them repeated: each repeat is an entry of its own (with a logit: under its own u)."""
    c = _run_case(name)[0]
    assert c.pairs.shape[0] > 100 and torch.equal(c.row[c.pairs[:, 0]], c.row[c.pairs[:, 1]])
    assert torch.equal(c.col[c.pairs[:, 0]], c.col[c.pairs[:, 1]])


# ----------------------------------------------------------------------------------------------------------------- exact results
@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    res = _run_case(name)
    c, out, dd = res[:3]
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    assert torch.equal(out[rows], c.v.float().to(DEV)[cols]), "out_i == v_j bit for bit"
    assert float(dd[rows].abs().max()) == 0.0, "the one dz of the row is an exact zero"
    if c.u is not None:
        assert float(res[5][single.to(DEV)].abs().max()) == 0.0, "S (the gradient of u) at the row's one entry is an exact zero"
    assert bool((dd[(deg > 1).to(DEV)].abs().amax(dim=1) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("zero-"))
def test_a_logit_of_zeros_changes_no_bit(name):
    """out, ds_dst, ds_src and dv under a logit of zeros are bit-equal to the op without a logit on the same inputs."""
    c, out, dd, ds, dv, du = _run_case(name)
    assert float(c.u.abs().max()) == 0.0
    want = _device_run(_pattern(c), c, leaves=_leaves(c)[:3])
    for got, ref, what in zip((out, dd, ds, dv), want, ("out", "ds_dst", "ds_src", "dv")):
        assert torch.equal(got, ref), (name, what)


@pytest.mark.parametrize("name", case.case_names("masked-"))
def test_a_masked_entry_is_exactly_out(name):
    """u = -9e15 on a third of the entries, every row keeping its first: priced as usual, and du at the masked entries is 0.0."""
    c, out, dd, ds, dv, du = _run_case(name)
    c.check_masked(du)
    assert float(du.abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    two_runs_bit_equal(case.cases()[name], _device_run)


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax(leaky_relu(s_dst[row] + s_src[col] (+ u))), v) on the device and the fused op: both pass against the same
    fp64 run."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("level-"))
def test_against_gat_level(name):
    """On a square graph additive_attention(graph.edge_pattern(), Wh . a_src, Wh . a_dst, Wh, 0.2) is gat_level(..., concat=False)
    without skip, head by head; Wh is formed in torch on the device and zero-padded to the next allowed F.  Both are priced against
    the fp64 level, per head, on the unpadded columns."""
    import pygat_amd as pg
    c = case.cases()[name]
    graph = _graph(*c.csr)
    x, W, a = (t.float().to(DEV) for t in (c.x, c.W, c.a))
    Wh = torch.einsum("nk,hkf->nhf", x, W)
    s_dst, s_src = (Wh * a[:, :c.F]).sum(-1), (Wh * a[:, c.F:]).sum(-1)
    padded = torch.nn.functional.pad(Wh, (0, c.FP - c.F))
    with torch.no_grad():
        fused = pg.additive_attention(graph.edge_pattern(), s_dst, s_src, padded, c.slope)
        level = torch.stack([pg.gat_level(x, graph, [W[h]], [a[h].reshape(-1, 1)], None, c.slope, False) for h in range(c.H)], 1)
    assert fused.shape == (c.shape[0], c.H, c.FP) and float(fused[:, :, c.F:].abs().max()) == 0.0
    c.price(fused[:, :, :c.F], name + " additive_attention")
    c.price(level, name + " gat_level")


@pytest.mark.parametrize("name", case.case_names("module-"))
def test_a_bipartite_gat_layer(name):
    """x_src [M, f_in] and x_dst [N, f_in] through one W and one a, additive_attention over a rectangular pattern, ELU, a sum: out and
    the gradients that reach x_src, x_dst, W and a."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda s_dst, s_src, v: pg.additive_attention(pattern, s_dst, s_src, v, c.slope)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x_src, x_dst = (t.float().to(DEV).requires_grad_(True) for t in (c.x_src, c.x_dst))
    out = module(x_src, x_dst)
    out.sum().backward()
    c.price(out.detach(), x_src.grad, x_dst.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.additive_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-logit"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]
    pattern = _pattern(c)
    with torch.no_grad():
        pg.additive_attention(pattern, *tensors[:3])
        pg.additive_attention(pattern, *tensors[:3], c.slope, tensors[3])
    assert seen == [FWD, FWD] and not pattern.has_transpose
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.additive_attention(pattern, *leaves[:3], c.slope, leaves[3])
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        assert seen == [FWD, ROWS] + [SPMM] * (needs[1] + needs[2]), (needs, seen)
        assert pattern.has_transpose == (needs[1] or needs[2]), "neither ds_dst nor du builds the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
    # no entries: zeros of the right shape, and nothing is launched
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    sd, ss, v0 = (torch.randn(*dims, device=DEV, requires_grad=True) for dims in ((5, 2), (7, 2), (7, 2, 8)))
    for shape in (None, (0, 2), (0,)):
        u0 = None if shape is None else torch.zeros(shape, device=DEV, requires_grad=True)
        leaves = [sd, ss, v0] + ([] if u0 is None else [u0])
        del seen[:]
        out = pg.additive_attention(empty, sd, ss, v0, 0.2, u0)
        grads = torch.autograd.grad(out, leaves, torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, leaves)) and all(float(g.abs().max()) == 0.0 for g in grads[:3])
        assert seen == [] and not empty.has_transpose, seen


def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    sd, ss, v = t(N, 4), t(N, 4), t(N, 4, 16)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    ok = (pattern, sd, ss, v)
    for args, kw, needle in (
            ((object(), sd, ss, v), {}, "an EdgePattern expected"),
            (ok, dict(negative_slope=float("nan")), "negative_slope = nan: a finite float expected"),
            (ok, dict(negative_slope=float("inf")), "negative_slope = inf"),
            (ok, dict(negative_slope="0.2"), "a finite float expected"),
            ((pattern, sd.cpu(), ss, v), {}, "s_dst must be a tensor on the GPU"),
            ((pattern, sd, [0.0] * N, v), {}, "s_src must be a tensor on the GPU"),
            ((pattern, sd, ss, v.double()), {}, "v must be float32, not torch.float64"),
            ((pattern, sd, ss.half(), v), {}, "s_src must be float32"),
            ((pattern, sd, ss, v.bfloat16()), {}, "v must be float32, not torch.bfloat16"),
            ((elsewhere, sd, ss, v), {}, "s_dst lives on cuda:0, the pattern on cuda:1"),
            ((pattern, t(N, 4, 1), ss, v), {}, "s_dst [n_rows] or [n_rows, H] expected"),
            ((pattern, sd, t(N, 3), v), {}, "s_src (%d, 3) does not match s_dst" % N),
            ((pattern, sd, t(N), v), {}, "does not match s_dst"),
            ((pattern, sd, ss, t(N, 16)), {}, "v (%d, 16) does not match s_dst" % N),
            ((pattern, sd, ss, t(N, 3, 16)), {}, "the same number of heads"),
            ((pattern, t(N + 1, 4), ss, v), {}, f"s_dst has {N + 1} rows but the pattern has {N} rows"),
            ((pattern, sd, t(N - 1, 4), v), {}, f"s_src has {N - 1} rows but the pattern has {N} columns"),
            ((pattern, sd, ss, t(N + 2, 4, 16)), {}, f"v has {N + 2} rows but the pattern has {N} columns"),
            ((pattern, t(N, 65), t(N, 65), t(N, 65, 4)), {}, "H = 65 heads: the limits are 1 <= H <= 64"),
            ((pattern, sd, ss, t(N, 4, 12)), {}, "F = 12: a head's width must be a power of two in 4..256; zero-padding the columns of v"),
            ((pattern, sd, ss, t(N, 4, 2)), {}, "F = 2"),
            ((pattern, t(N), t(N), t(N, 512)), {}, "F = 512"),
            ((pattern, t(N, 8), t(N, 8), t(N, 8, 256)), {}, "H * F = 8 * 256 = 2048 floats per row: the limit is H * F <= 1024"),
            (ok, dict(edge_logit=[0.0] * E), "edge_logit must be a tensor on the GPU"),
            (ok, dict(edge_logit=torch.zeros(E, 4)), "edge_logit must be a tensor on the GPU"),
            (ok, dict(edge_logit=t(E, 4).double()), "edge_logit must be float32, not torch.float64"),
            ((elsewhere, sd, ss, v), dict(edge_logit=t(E, 4)), "edge_logit lives on cuda:0, the pattern on cuda:1"),
            (ok, dict(edge_logit=t(E, 8)), f"edge_logit [E, H] = [{E}, 4] or [E] = [{E}] expected"),
            (ok, dict(edge_logit=t(E + 1, 4)), f"got ({E + 1}, 4)"),
            (ok, dict(edge_logit=t(E, 1)), f"got ({E}, 1)"),
            ((pattern, sd[:, 0], ss[:, 0], v[:, 0]), dict(edge_logit=t(E, 1)), f"edge_logit [E] = [{E}] expected")):
        with pytest.raises(ValueError, match="additive_attention") as err:
            pg.additive_attention(*args, **kw)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient
    mod = importlib.import_module("pygat_amd.additive_attention")
    leaves = [x.clone().requires_grad_(True) for x in (sd, ss, v)]
    out = pg.additive_attention(pattern, *leaves)
    del seen[:]
    with pytest.raises(ValueError, match="additive_attention: the gradient of the output must be float32, not torch.float64"):
        mod._AdditiveAttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# ---------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("name", ["twice-nine_hubs-8x16-indices-logit", "twice-hub-3x8-graph"])
def test_capture_and_replay(name):
    """Forward and backward captured once under torch.cuda.graph (nothing is read back to the host); the replay gives the eager
    result bit for bit."""
    c = case.cases()[name]
    pattern = _pattern(c)
    static = _leaves(c)
    G = c.G.float().to(DEV)
    fn = _fused(pattern, c)

    def step():
        out = fn(*static)
        return (out,) + torch.autograd.grad(out, static, G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # (warm-up off the default stream: the transpose is built here)
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in captured]
    eager = _device_run(pattern, c)
    for a, b, what in zip(got, eager, ["out"] + c.names):
        assert torch.equal(a, b), what
    c.price(*got)


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_no_kernel_uses_scratch():
    assert len(K20) == 80
    no_scratch(K20, (b"k20_fwd_row_l3v1", b"k20_fwd_row_l32v2", b"k20_fwd_row_l64v5", b"k20_mid_row_l8v1", b"k20_fwd_row_l8v1x", b"k20_",
                     b"k20", b"k20fwd_row_l8v1", b"k20b_fwd_row_l8v1", b"k20u_fwd_col_l8v1", b"k20u_bwd_row_l0v1"))
