"""pygat_amd.gatv2_attention_dropout (the DROP instantiations of the two row passes of csrc/k21_gatv2_attention.hip): gatv2_attention
with seeded dropout on the softmax coefficients, the decision for (entry, head) drawn in the kernels of both row passes -- out, dx_dst,
dx_src, da, dv.

Ground truth, the mask and the seeded cases live in gatv2_attention_dropout_case.py: torch autograd in fp64 on the CPU with the mask of
tests/philox_ref.py, loss L = <out, G>, pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad).
Every case is rehearsed on the CPU, the fp32 ground-truth run standing in for the device, by tests/test_gatv2_attention_dropout_abi.py
and passes there; no case is built here."""
import copy
import importlib
import itertools

import pytest
import torch

import gatv2_attention_dropout_case as case
from pattern_device import DEV, _pattern, _seed, device_run, no_scratch, spied
from pattern_device import leaves as _leaves

pytestmark = pytest.mark.gpu

FWD, ROWS, COLS, SPMM = "pygat_v2_attn_forward", "pygat_v2_attn_backward_rows", "pygat_v2_attn_backward_cols", "pygat_spmm_forward"
DFWD, DROWS = "pygat_v2_attn_dropout_forward", "pygat_v2_attn_dropout_backward_rows"
SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K21D = [f"{fam}_{d}_{kind}_l{l}v{v}" for fam in ("k21d", "k21ds") for d in ("fwd", "bwd") for kind in ("long", "row") for l, v in SHAPES]


def _fused(pattern, c, seed=None):
    import pygat_amd as pg
    seed = _seed(c.seed) if seed is None else seed
    return lambda x_dst, x_src, a, v=None: pg.gatv2_attention_dropout(pattern, x_dst, x_src, a, c.p, v, c.slope, seed=seed)


def _from_parts(pattern, c, seed=None):
    import pygat_amd as pg
    seed = _seed(c.seed) if seed is None else seed
    row, col = c.row.to(DEV), c.col.to(DEV)

    def run(x_dst, x_src, a, v=None):
        e = (a * torch.nn.functional.leaky_relu(x_dst[row] + x_src[col], c.slope)).sum(-1)
        alpha = pg.edge_softmax(pattern, e)
        return pg.spmm(pattern, alpha * pg.attention_dropout_mask(pattern, c.H, c.p, seed).view(alpha.shape), x_src if v is None else v)
    return run


def _device_run(pattern, c, fn=None, seed=None, leaves=None):
    """-> (out, dx_dst, dx_src, da[, dv]) on the device."""
    return device_run(pattern, c, fn or _fused, leaves, seed=seed)


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price(*res)
    c.check_all_dropped(res[0])
    return (c,) + res


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.gatv2_attention", "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-"))
def test_lane_shapes(name):
    """Every lane shape -- LPR 1..64, VEC 2, 3 and 4, tensors without a head axis -- at p = 0.5, with and without a permutation, v shared
    (v=None) and separate: the four DROP kernels with and without SHARED, and the column pass as it is."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks, scores of std 3, at p = 0.5 and 0.9: a mask drawn at the wrong entry index in
    the long-row launch, or Z taken over the kept entries alone, moves out far beyond 1e-5."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("rect-") + case.case_names("repeats-") + case.case_names("gone-"))
def test_unsorted_entries_and_rows_that_lose_every_entry(name):
    """Unsorted entries (only the permutation finds an entry's decision), a rectangular pattern with empty rows, repeated (row, col)
    pairs with a decision each; at p = 0.9, rows of two and more entries that lose all of them in a head are exact zeros there."""
    c, out = _run_case(name)[:2]
    if name.startswith("gone-"):
        gone = c.all_dropped().to(DEV)
        assert int(gone.sum()) >= 5 and float(out[gone].abs().max()) == 0.0
        some_kept = ~c.all_dropped(min_entries=0).to(DEV)                       # (a row and head that keep at least one entry)
        assert bool((out[some_kept].abs().amax(-1) > 0.0).all())


# -------------------------------------------------------------------------------------------------------------- the mask, bit for bit
@pytest.mark.parametrize("name", case.case_names("single-"))
def test_the_mask_bit_for_bit(name):
    """Exactly one entry per row, unsorted: every coefficient is 1, so out[i, h, :] == mask[e, h] * v[col_e, h, :] exactly, with the mask
    of tests/philox_ref.py at the CALLER's entry index; attention_dropout_mask writes the same table on the device; dx_dst is exact
    zeros (at p = 0.5 the factor 2 is exact in <G_i, out_i> as well)."""
    import pygat_amd as pg
    c, out, dd = _run_case(name)[:3]
    mask = c.mask.to(DEV)
    assert torch.equal(pg.attention_dropout_mask(_pattern(c), c.H, c.p, _seed(c.seed)), mask)
    v = c.x_src if c.shared else c.v
    want = torch.zeros_like(out)
    want[c.row.to(DEV)] = mask[:, :, None] * v.float().to(DEV)[c.col.to(DEV)]
    assert torch.equal(out, want), "out_i == mask_e * v_j bit for bit"
    assert bool((out == 0).any()) and bool((out != 0).any())
    assert float(dd.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax(score) * attention_dropout_mask, v) on the device and the fused op: both pass against the same fp64 run, out
    and every gradient.  The mask's bits through P, where v is a table of its own: with G = 1, dv[j, h, :] = sum over the entries of
    column j of P[e, h], a sum of terms >= 0 (p > 0: no score of these cases underflows), so it is an exact zero where, and only where,
    the mask drops every entry of the column in that head."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")
    if not c.shared:
        leaves = _leaves(c)
        out = _fused(pattern, c)(*leaves)
        dv = torch.autograd.grad(out, leaves[3], torch.ones_like(out))[0]
        kept = torch.zeros(c.shape[1], c.H).index_add(0, c.col, (c.mask != 0).float())
        assert torch.equal(dv[:, :, 0] == 0, (kept == 0).to(DEV)), "the exact zeros of P are the mask's"
        filled = torch.bincount(c.col, minlength=c.shape[1]) > 0
        assert bool((kept[filled] == 0).any()) and bool((kept[filled] != 0).any())


# ---------------------------------------------------------------------------------------------------------------- trivial paths
def test_trivial_paths(monkeypatch):
    """training=False and p = 0 are gatv2_attention itself, bit for bit, without a dropout launch; p = 1 gives zeros in out, dx_dst and
    dv (and in x_src's and a's gradients where v is a table of its own: S is zero); p next to 0 goes through the DROP kernels, keeps
    every entry with a factor of 1.0f, and is gatv2_attention bit for bit as well."""
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    for name in ("near0-hub-8x16-indices-shared", "near0-hub-12x64-graph-separate"):
        c = case.cases()[name]
        pattern = _pattern(c)
        G = c.G.float().to(DEV)

        def run(fn):
            del seen[:]
            leaves = _leaves(c)
            out = fn(*leaves)
            return (out.detach(),) + torch.autograd.grad(out, leaves, G), list(seen)
        want, launched = run(lambda *lv: pg.gatv2_attention(pattern, *lv[:3], *lv[3:], negative_slope=c.slope))
        assert launched[:3] == [FWD, ROWS, COLS]
        for kw in (dict(p=0.5, training=False), dict(p=0.0), dict(p=0.0, seed=_seed(5)), dict(p=0, training=False)):
            got, seen_now = run(lambda *lv: pg.gatv2_attention_dropout(pattern, *lv[:3], kw["p"], *lv[3:], negative_slope=c.slope,
                                                                      **{k: v for k, v in kw.items() if k != "p"}))
            assert seen_now == launched and DFWD not in seen_now, (kw, seen_now)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), kw
        got, seen_now = run(lambda *lv: pg.gatv2_attention_dropout(pattern, *lv[:3], 1.0, *lv[3:], negative_slope=c.slope,
                                                                  seed=_seed(c.seed)))
        assert seen_now[:3] == [DFWD, DROWS, COLS]
        assert all(float(t.abs().max()) == 0.0 for t in got), "p = 1: nothing is kept"
        got, seen_now = run(lambda *lv: pg.gatv2_attention_dropout(pattern, *lv[:3], c.p, *lv[3:], negative_slope=c.slope,
                                                                  seed=_seed(c.seed)))
        assert seen_now[:3] == [DFWD, DROWS, COLS]
        c.price(*got)
        assert all(torch.equal(a, b) for a, b in zip(got, want)), (name, "every entry kept with a factor of 1")


# ---------------------------------------------------------------------------------------------------------------- reproducible
@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_same_seed_same_bits_new_seed_new_mask(name):
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    runs = [_device_run(pattern, c) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    c.price(*runs[0])
    other = _device_run(pattern, c, seed=_seed(c.seed + 1))
    assert not torch.equal(other[0], runs[0][0]) and not torch.equal(other[1], runs[0][1])
    # without a seed: one is drawn from the generator -- the same generator state, the same bits
    leaves = [t.detach() for t in _leaves(c)]
    gen = torch.Generator(device=DEV)
    outs = []
    for s in (3, 3, 4):
        gen.manual_seed(s)
        outs.append(pg.gatv2_attention_dropout(pattern, *leaves[:3], c.p, *leaves[3:], negative_slope=c.slope, generator=gen))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def test_only_the_needed_launches(monkeypatch):
    """x_dst alone: the row pass, and the transposed pattern is never built; x_src or a: the column pass, unchanged, besides; v: K17
    besides."""
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-separate"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]
    seed = _seed(c.seed)
    pattern = _pattern(c)
    with torch.no_grad():
        pg.gatv2_attention_dropout(pattern, *tensors[:3], 0.5, seed=seed)
        pg.gatv2_attention_dropout(pattern, *tensors[:3], 0.5, tensors[3], seed=seed)
    assert seen == [DFWD, DFWD] and not pattern.has_transpose
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.gatv2_attention_dropout(pattern, *leaves[:3], 0.5, leaves[3], c.slope, seed=seed)
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        cols = needs[1] or needs[2]
        assert seen == [DFWD, DROWS] + [COLS] * cols + [SPMM] * needs[3], (needs, seen)
        assert pattern.has_transpose == (cols or needs[3]), "dx_dst alone does not build the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
    # v=None: x_src is the value table too, so its gradient takes the column pass and K17; a alone takes the column pass only
    for needs, want in (((True, False, False), [DFWD, DROWS]), ((False, True, False), [DFWD, DROWS, COLS, SPMM]),
                        ((False, False, True), [DFWD, DROWS, COLS])):
        pattern = _pattern(c)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors[:3], needs)]
        out = pg.gatv2_attention_dropout(pattern, *leaves, 0.5, None, c.slope, seed=seed)
        torch.autograd.grad(out, [t for t, n in zip(leaves, needs) if n], G)
        assert seen == want and pattern.has_transpose == (len(want) > 2), (needs, seen)
    # no entries: zeros of the right shape, differentiable, and nothing launched at all
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    xd, xs, a0, v0 = (torch.randn(*dims, device=DEV, requires_grad=True) for dims in ((5, 2, 8), (7, 2, 8), (2, 8), (7, 2, 8)))
    for leaves in ([xd, xs, a0], [xd, xs, a0, v0]):
        del seen[:]
        out = pg.gatv2_attention_dropout(empty, *leaves[:3], 0.5, *leaves[3:], seed=seed)
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
    xd, xs, a = t(N, 4, 16), t(N, 4, 16), t(4, 16)
    seed = _seed(1)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    ok = (pattern, xd, xs, a, 0.5)
    for args, kw, needle in (((pattern, xd, xs.bfloat16(), a, 0.5), {}, "no training path on bfloat16"),
                             (ok, dict(v=xs.bfloat16()), "no training path on bfloat16"),
                             ((pattern, xd, xs, a, 1.5), {}, "p = 1.5"), ((pattern, xd, xs, a, -0.5), {}, "p = -0.5"),
                             ((pattern, xd, xs, a, float("nan")), {}, "p = nan"), ((pattern, xd, xs, a, 2.0), dict(training=False), "p = 2.0"),
                             (ok, dict(seed=7), "seed must be an int64 tensor of shape [1]"),
                             (ok, dict(seed=seed.int()), "got torch.int32 (1,)"),
                             (ok, dict(seed=torch.zeros(2, dtype=torch.int64, device=DEV)), "got torch.int64 (2,)"),
                             (ok, dict(seed=seed.cpu()), "on cpu"),
                             ((pattern, xd, xs, a, 0.0), dict(seed=seed.cpu()), "on cpu"),
                             ((elsewhere, xd, xs, a, 0.5), dict(seed=seed), "cuda:1"),
                             (ok, dict(negative_slope=float("inf")), "negative_slope = inf"),
                             ((object(), xd, xs, a, 0.5), {}, "EdgePattern"),
                             ((pattern, xd.cpu(), xs, a, 0.5), {}, "x_dst must be a tensor on the GPU"),
                             ((pattern, xd, xs.double(), a, 0.5), {}, "x_src must be float32"),
                             ((pattern, xd, xs, a.half(), 0.5), {}, "a must be float32"),
                             ((pattern, t(N, 4, 12), t(N, 4, 12), t(4, 12), 0.5), {}, "F = 12"),
                             ((pattern, t(N, 65, 4), t(N, 65, 4), t(65, 4), 0.5), {}, "H = 65"),
                             ((pattern, t(N, 8, 256), t(N, 8, 256), t(8, 256), 0.5), {}, "H * F = 8 * 256 = 2048"),
                             (ok, dict(v=t(N + 1, 4, 16)), f"v has {N + 1} rows but the pattern has {N} columns"),
                             ((pattern, xd, xs, t(4, 8), 0.5), {}, "does not match x_dst"),
                             (ok, dict(v=t(N, 4, 16).cpu(), training=False), "v must be a tensor on the GPU")):
        with pytest.raises(ValueError, match="gatv2_attention_dropout: ") as err:
            pg.gatv2_attention_dropout(*args, **kw)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient is refused under this op's name
    mod = importlib.import_module("pygat_amd.gatv2_attention")
    leaves = [x.clone().requires_grad_(True) for x in (xd, xs, a)]
    out = pg.gatv2_attention_dropout(pattern, *leaves, 0.5, seed=seed)
    del seen[:]
    with pytest.raises(ValueError, match="gatv2_attention_dropout: the gradient of the output must be float32"):
        mod._Gatv2AttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# ---------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("name", case.case_names("capture-"))
def test_capture_and_replay_with_a_refilled_seed(name):
    """Forward and backward captured once under torch.cuda.graph, on one stream; the seed tensor is refilled in place between replays,
    and every replay gives the eager result of its seed, bit for bit."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    seed = _seed(c.seed)
    static = _leaves(c)
    G = c.G.float().to(DEV)

    def step():
        out = pg.gatv2_attention_dropout(pattern, *static[:3], c.p, *static[3:], negative_slope=c.slope, seed=seed)
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
    for value in (c.seed, c.seed + 1, c.seed):
        seed.fill_(value)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in captured]
        eager = _device_run(pattern, c, seed=_seed(value))
        for a, b, what in zip(got, eager, ["out"] + c.names):
            assert torch.equal(a, b), (value, what)
        if value == c.seed:
            c.price(got[0], *got[1:])


# ------------------------------------------------------------------------------------------------------------------ in a module
@pytest.mark.parametrize("name", case.case_names("module-"))
def test_a_bipartite_gatv2_layer_under_dropout(name):
    """gatv2_attention_case's BipartiteGATv2 with gatv2_attention_dropout as `attend`: out and the gradients that reach x_src, x_dst,
    W_l, W_r and a."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    seed = _seed(c.mask_seed)
    module = c.module(lambda h_dst, h_src, a: pg.gatv2_attention_dropout(pattern, h_dst, h_src, a, c.p, None, c.slope, seed=seed)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x_src, x_dst = (t.float().to(DEV).requires_grad_(True) for t in (c.x_src, c.x_dst))
    out = module(x_src, x_dst)
    out.sum().backward()
    c.price(out.detach(), x_src.grad, x_dst.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_dropout_kernels_have_no_scratch():
    assert len(K21D) == 80
    no_scratch(K21D, (b"k21d_fwd_row_l3v1", b"k21d_fwd_row_l32v2", b"k21ds_fwd_row_l64v5", b"k21d_mid_row_l8v1", b"k21ds_fwd_row_l8v1x", b"k21d_",
                      b"k21d", b"k21dfwd_row_l8v1", b"k21b_fwd_row_l8v1", b"k21sd_fwd_row_l8v1", b"k21d_col_row_l8v1", b"k21ds_col_long_l8v1"))
