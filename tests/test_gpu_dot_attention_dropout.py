"""pygat_amd.dot_attention_dropout (the DROP instantiations of csrc/k19_dot_attention.hip): dot_attention with seeded dropout on the
softmax coefficients, the decision for (entry, head) drawn in the kernels of both passes -- out, dq, dk, dv and db.

Ground truth, the mask and the seeded cases live in dot_attention_dropout_case.py: torch autograd in fp64 on the CPU with the mask of
tests/philox_ref.py, loss L = <out, G>, pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad).
Every case is rehearsed on the CPU, the fp32 ground-truth run standing in for the device, by tests/test_dot_attention_dropout_abi.py
and passes there; no case is built here."""
import itertools

import pytest
import torch

import dot_attention_dropout_case as case
from pattern_device import BFWD, BROWS, DEV, FWD, ROWS, SPMM, _pattern, _seed, device_run, no_scratch, spied  # noqa: F401
from pattern_device import leaves as _leaves

pytestmark = pytest.mark.gpu

DFWD, DROWS, MASK = "pygat_dot_attn_dropout_forward", "pygat_dot_attn_dropout_backward_rows", "pygat_dropout_mask"
SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K19D = [f"{fam}_{d}_{kind}_l{l}v{v}" for fam in ("k19d", "k19db") for d in ("fwd", "bwd") for kind in ("long", "row") for l, v in SHAPES]


def _fused(pattern, c, seed=None):
    import pygat_amd as pg
    seed = _seed(c.seed) if seed is None else seed
    return lambda q, k, v, b=None: pg.dot_attention_dropout(pattern, q, k, v, c.p, c.fed_scale, b, seed=seed)


def _from_parts(pattern, c, seed=None):
    import pygat_amd as pg
    seed = _seed(c.seed) if seed is None else seed

    def run(q, k, v, b=None):
        s = pg.edge_dot(pattern, q, k, c.scale)
        alpha = pg.edge_softmax(pattern, s if b is None else s + b)
        return pg.spmm(pattern, alpha * pg.attention_dropout_mask(pattern, c.H, c.p, seed), v)
    return run


def _device_run(pattern, c, fn=None, seed=None):
    """-> (out, dq, dk, dv[, db]) on the device."""
    return device_run(pattern, c, fn or _fused, seed=seed)


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price(*res)
    c.check_all_dropped(res[0])
    return (c,) + res


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-"))
def test_lane_shapes(name):
    """Every lane shape -- LPR 1..64, VEC 2, 3 and 4, tensors without a head axis -- at p = 0.5, with and without a permutation, without
    a bias and with one ([E, H], and [E] shared by the heads): the four DROP kernels of both families."""
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
    of tests/philox_ref.py at the CALLER's entry index; attention_dropout_mask writes the same table on the device; dq is exact zeros
    (at p = 0.5 the factor 2 is exact in <G_i, out_i> as well)."""
    import pygat_amd as pg
    c, out, dq = _run_case(name)[:3]
    mask = c.mask.to(DEV)
    assert torch.equal(pg.attention_dropout_mask(_pattern(c), c.H, c.p, _seed(c.seed)), mask)
    want = torch.zeros_like(out)
    want[c.row.to(DEV)] = mask[:, :, None] * c.v.float().to(DEV)[c.col.to(DEV)]
    assert torch.equal(out, want), "out_i == mask_e * v_j bit for bit"
    assert bool((out == 0).any()) and bool((out != 0).any())
    assert float(dq.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax(edge_dot(q, k, scale) + bias) * attention_dropout_mask, v) on the device and the fused op: both pass against the
    same fp64 run, out and every gradient."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("masked-"))
def test_masked_entries_under_dropout(name):
    """bias = -9e15 on a third of the entries and dropout on top: priced as usual; db at the masked entries is 0.0 whether or not the
    dropout keeps them."""
    c, out, dq, dk, dv, db = _run_case(name)
    c.check_masked(db)
    assert float(db.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------- trivial paths
def test_trivial_paths(monkeypatch):
    """training=False and p = 0 are dot_attention itself, bit for bit, without a dropout launch; p = 1 gives zeros everywhere; p next to
    0 goes through the DROP kernels, keeps every entry with a factor of 1.0f, and is dot_attention bit for bit as well."""
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    for name in ("near0-hub-8x16-indices-plain", "near0-hub-12x64-graph-bias"):
        c = case.cases()[name]
        pattern = _pattern(c)
        G = c.G.float().to(DEV)

        def run(fn):
            del seen[:]
            leaves = _leaves(c)
            out = fn(*leaves)
            return (out.detach(),) + torch.autograd.grad(out, leaves, G), list(seen)
        bias_kw = (lambda lv: {} if c.bias is None else {"bias": lv[3]})
        want, launched = run(lambda *lv: pg.dot_attention(pattern, *lv[:3], c.fed_scale, **bias_kw(lv)))
        assert launched[:2] == ([FWD, ROWS] if c.bias is None else [BFWD, BROWS])
        for kw in (dict(p=0.5, training=False), dict(p=0.0), dict(p=0.0, seed=_seed(5)), dict(p=0, training=False)):
            got, seen_now = run(lambda *lv: pg.dot_attention_dropout(pattern, *lv[:3], kw["p"], c.fed_scale, **bias_kw(lv),
                                                                    **{k: v for k, v in kw.items() if k != "p"}))
            assert seen_now == launched and DFWD not in seen_now, (kw, seen_now)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), kw
        got, seen_now = run(lambda *lv: pg.dot_attention_dropout(pattern, *lv[:3], 1.0, c.fed_scale, **bias_kw(lv), seed=_seed(c.seed)))
        assert seen_now[:2] == [DFWD, DROWS]
        assert all(float(t.abs().max()) == 0.0 for t in got), "p = 1: nothing is kept"
        got, seen_now = run(lambda *lv: pg.dot_attention_dropout(pattern, *lv[:3], c.p, c.fed_scale, **bias_kw(lv), seed=_seed(c.seed)))
        assert seen_now[:2] == [DFWD, DROWS]
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
        outs.append(pg.dot_attention_dropout(pattern, *leaves[:3], c.p, c.fed_scale, *leaves[3:], generator=gen))
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-hub-8x16-indices-bias"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]
    seed = _seed(c.seed)
    pattern = _pattern(c)
    with torch.no_grad():
        pg.dot_attention_dropout(pattern, *tensors[:3], 0.5, bias=tensors[3], seed=seed)
        pg.dot_attention_dropout(pattern, *tensors[:3], 0.5, seed=seed)
    assert seen == [DFWD, DFWD] and not pattern.has_transpose
    for needs in itertools.product((False, True), repeat=4):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.dot_attention_dropout(pattern, *leaves[:3], 0.5, bias=leaves[3], seed=seed)
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        assert seen == [DFWD, DROWS] + [SPMM] * (needs[1] + needs[2]), (needs, seen)
        assert pattern.has_transpose == (needs[1] or needs[2]), "neither dq nor db builds the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
    # the mask as a tensor: one launch
    del seen[:]
    dropout_mod = __import__("importlib").import_module("pygat_amd.dot_attention")
    assert pg.attention_dropout_mask(pattern, 8, 0.5, seed).shape == (c.row.numel(), 8) and seen == [MASK]
    assert dropout_mod.STREAM_ATT == case.STREAM_ATT
    # no entries: zeros of the right shape, differentiable, and nothing launched at all
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    q0, k0, v0 = (torch.randn(n, 2, 8, device=DEV, requires_grad=True) for n in (5, 7, 7))
    for shape in ((0, 2), (0,), None):
        b0 = None if shape is None else torch.zeros(shape, device=DEV, requires_grad=True)
        leaves = [q0, k0, v0] + ([] if b0 is None else [b0])
        del seen[:]
        out = pg.dot_attention_dropout(empty, q0, k0, v0, 0.5, bias=b0, seed=seed)
        grads = torch.autograd.grad(out, leaves, torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, leaves)) and all(float(g.abs().sum()) == 0.0 for g in grads)
        assert seen == [], seen
    assert pg.attention_dropout_mask(empty, 2, 0.5, seed).shape == (0, 2) and seen == []


def test_refusals(monkeypatch):
    import copy
    import importlib
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-plain"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    q, k, v = t(N, 4, 16), t(N, 4, 16), t(N, 4, 16)
    seed = _seed(1)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    for args, kw, needle in (((pattern, q, k.bfloat16(), v.bfloat16(), 0.5), {}, "no training path on bfloat16 tables"),
                             ((pattern, q, k, v.bfloat16(), 0.5), {}, "no training path on bfloat16 tables"),
                             ((pattern, q, k, v, 1.5), {}, "p = 1.5"), ((pattern, q, k, v, -0.5), {}, "p = -0.5"),
                             ((pattern, q, k, v, float("nan")), {}, "p = nan"), ((pattern, q, k, v, 2.0), dict(training=False), "p = 2.0"),
                             ((pattern, q, k, v, 0.5), dict(seed=7), "seed must be an int64 tensor of shape [1]"),
                             ((pattern, q, k, v, 0.5), dict(seed=seed.int()), "got torch.int32 (1,)"),
                             ((pattern, q, k, v, 0.5), dict(seed=torch.zeros(2, dtype=torch.int64, device=DEV)), "got torch.int64 (2,)"),
                             ((pattern, q, k, v, 0.5), dict(seed=seed.cpu()), "on cpu"),
                             ((pattern, q, k, v, 0.0), dict(seed=seed.cpu()), "on cpu"),
                             ((elsewhere, q, k, v, 0.5), dict(seed=seed), "cuda:1"),
                             ((object(), q, k, v, 0.5), {}, "EdgePattern"), ((pattern, q.cpu(), k, v, 0.5), {}, "q must be a tensor on the GPU"),
                             ((pattern, q.double(), k, v, 0.5), {}, "q must be float32"), ((pattern, q, k.half(), v, 0.5), {}, "k must be float32"),
                             ((pattern, t(N, 4, 12), t(N, 4, 12), t(N, 4, 12), 0.5), {}, "F = 12"),
                             ((pattern, t(N, 65, 4), t(N, 65, 4), t(N, 65, 4), 0.5), {}, "H = 65"),
                             ((pattern, t(N, 8, 256), t(N, 8, 256), t(N, 8, 256), 0.5), {}, "H * F = 8 * 256 = 2048"),
                             ((pattern, q, k, t(N + 1, 4, 16), 0.5), {}, f"v has {N + 1} rows but the pattern has {N} columns"),
                             ((pattern, q, k, v, 0.5), dict(bias=t(E, 8)), f"got ({E}, 8)"),
                             ((pattern, q, k, v, 0.5), dict(bias=t(E, 4).double()), "bias must be float32"),
                             ((pattern, q, k, v, 0.0), dict(bias=t(E + 1)), f"got ({E + 1},)"),
                             ((pattern, q, k, v, 0.5), dict(bias=t(E, 4).cpu(), training=False), "bias must be a tensor on the GPU")):
        with pytest.raises(ValueError, match="dot_attention_dropout: ") as err:
            pg.dot_attention_dropout(*args, **kw)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient is refused under this op's name
    mod = importlib.import_module("pygat_amd.dot_attention")
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v)]
    out = pg.dot_attention_dropout(pattern, *leaves, 0.5, seed=seed)
    del seen[:]
    with pytest.raises(ValueError, match="dot_attention_dropout: the gradient of the output must be float32"):
        mod._DotAttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# ---------------------------------------------------------------------------------------------------------------- graph capture
@pytest.mark.parametrize("name", case.case_names("capture-"))
def test_capture_and_replay_with_a_refilled_seed(name):
    """Forward and backward captured once under torch.cuda.graph; the seed tensor is refilled in place between replays, and every
    replay gives the eager result of its seed, bit for bit."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    seed = _seed(c.seed)
    static = _leaves(c)
    G = c.G.float().to(DEV)

    def step():
        out = pg.dot_attention_dropout(pattern, *static[:3], c.p, c.fed_scale, *static[3:], seed=seed)
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
def test_in_a_module(name):
    """Three nn.Linear projections, bias = nn.Embedding(edge_type), dot_attention_dropout, a sum: out and the gradients that reach x, the
    three weights and the embedding table."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    seed = _seed(c.mask_seed)
    module = c.module(lambda q, k, v, b: pg.dot_attention_dropout(pattern, q, k, v, c.p, bias=b, seed=seed)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x = c.x.float().to(DEV).requires_grad_(True)
    out = module(x)
    out.sum().backward()
    grads = [module.get_parameter(n).grad for n in c.NAMES]
    assert all(g is not None and float(g.abs().max()) > 0.0 for g in [x.grad] + grads)
    c.price(out.detach(), x.grad, *grads)


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_dropout_kernels_have_no_scratch():
    assert len(K19D) == 80
    no_scratch(K19D, (b"k19d_fwd_row_l3v1", b"k19d_fwd_row_l32v2", b"k19db_fwd_row_l64v5", b"k19d_mid_row_l8v1", b"k19db_fwd_row_l8v1x", b"k19d_",
                      b"k19d", b"k19dfwd_row_l8v1", b"k19dh_fwd_row_l8v1", b"k19dbb_fwd_row_l8v1"))
