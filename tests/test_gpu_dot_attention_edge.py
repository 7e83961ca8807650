"""pygat_amd.dot_attention_edge (the EDGE instantiations of csrc/k19_dot_attention.hip): dot_attention with a feature row e per entry
on the key and the value side -- out, dq, dk, dv, de and, with a bias, db.

Ground truth, inputs and the seeded cases live in dot_attention_edge_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>,
pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad).  Every case is rehearsed on the CPU, the
fp32 ground-truth run standing in for the device, by tests/test_dot_attention_edge_abi.py and passes there; no case is built here."""
import importlib
import itertools

import pytest
import torch

import dot_attention_edge_case as case
from pattern_device import DEV, FWD, ROWS, SPMM, _pattern, degree, device_run, no_scratch, spied, to_leaves, two_runs_bit_equal  # noqa: F401

pytestmark = pytest.mark.gpu

EFWD, EROWS = "pygat_dot_attn_edge_forward", "pygat_dot_attn_edge_backward_rows"
K19E = [f"k19{p}_{d}_{kind}_l{l}v{v}" for p in ("e", "eb") for d in ("fwd", "bwd") for kind in ("long", "row")
        for l, v in ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))]


def _fused(pattern, c):
    import pygat_amd as pg
    return lambda q, k, v, e, b=None: pg.dot_attention_edge(pattern, q, k, v, e, c.fed_scale, b)


def _from_parts(pattern, c):
    """The chain a user writes without the fused op: two score terms, edge_softmax, spmm and a scatter of alpha e."""
    import pygat_amd as pg
    row = c.row.to(DEV)

    def run(q, k, v, e, b=None):
        s = pg.edge_dot(pattern, q, k, c.scale) + c.scale * (q[row] * e).sum(-1)
        alpha = pg.edge_softmax(pattern, s if b is None else s + b)
        return pg.spmm(pattern, alpha, v) + torch.zeros_like(q).index_add(0, row, alpha[..., None] * e)
    return run


def _device_run(pattern, c, fn=None):
    """-> (out, dq, dk, dv, de[, db]) on the device."""
    return device_run(pattern, c, fn or _fused)


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def _run_case(name):
    c = case.cases()[name]
    res = _device_run(_pattern(c), c)
    c.price(*res)
    return (c,) + res


# ------------------------------------------------------------------------------------------------------------------ lane shapes
@pytest.mark.parametrize("name", case.case_names("lanes-"))
def test_lane_shapes(name):
    """Every lane shape with e ~ N(0, 1), with and without a permutation, on the hub pattern (a row of 699 entries: the long-row
    launches); three shapes on the asymmetric one (rows of one entry); tensors without a head axis with e [E, F]."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("bias-") + case.case_names("masked-"))
def test_with_a_bias(name):
    """e beside a [E, H] bias and a [E] one shared by the heads: db and de both priced; under a mask (-9e15 on a third of the entries,
    every row keeping its first) de and db at a masked entry are 0.0 in every element."""
    res = _run_case(name)
    res[0].check_masked(res[1:])
    assert float(res[6].abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("long-"))
def test_long_rows(name):
    """Every slot of a chunk and a row of three chunks under e of std 3: the key-side term decides which entries dominate a hub row,
    so a row of e read at the wrong entry in the long-row launch, or a wrong merge of the records, moves out far beyond the
    tolerance."""
    _run_case(name)


@pytest.mark.parametrize("name", case.case_names("rect-") + case.case_names("repeats-"))
def test_unsorted_entries_take_their_own_row_of_e(name):
    """Unsorted entries (only the permutation places a row of e and of de), a rectangular pattern with empty rows and columns,
    repeated (row, col) pairs whose two entries carry different rows of e and get different rows of de."""
    c, out, dq, dk, dv, de = _run_case(name)
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    if name.startswith("rect-"):
        assert int(no_row.sum()) == 100
        assert float(out[no_row].abs().max()) == 0.0 and float(dq[no_row].abs().max()) == 0.0
    else:
        a, b = c.pairs[:, 0].to(DEV), c.pairs[:, 1].to(DEV)
        assert bool((de[a] != de[b]).flatten(1).any(1).all())


@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    c, out, dq, dk, dv, de = _run_case(name)
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    e_c = c.e.float().to(DEV)[single.to(DEV)]
    assert torch.equal(out[rows], c.v.float().to(DEV)[cols] + e_c), "out_i == v_j + e_c bit for bit"
    assert float(dq[rows].abs().max()) == 0.0
    assert torch.equal(de[single.to(DEV)], c.G.float().to(DEV)[rows]), "de_c == G_i bit for bit"
    assert bool((dq[(deg > 1).to(DEV)].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("zero-"))
def test_e_of_zeros_gives_the_values_of_dot_attention(name):
    """out, dq, dk, dv and db under e = 0 are torch.equal to dot_attention's on the same inputs: k_j + 0 and v_j + 0 are k_j and v_j
    in value and everything after the add is the same arithmetic.  de is priced against the ground truth as ever: it is not zero."""
    import pygat_amd as pg
    c, out, *grads = _run_case(name)
    pattern = _pattern(c)
    leaves = to_leaves([c.q, c.k, c.v] + ([] if c.bias is None else [c.bias]))
    want = pg.dot_attention(pattern, *leaves[:3], c.fed_scale, leaves[3] if c.bias is not None else None)
    wgrads = torch.autograd.grad(want, leaves, c.G.float().to(DEV))
    got = [out] + grads[:3] + grads[4:]
    names = ["out", "dq", "dk", "dv", "db"]
    assert len(got) == 1 + len(wgrads)
    for g, w, what in zip(got, [want.detach()] + list(wgrads), names):
        assert torch.equal(g, w), (name, what, float((g - w).abs().max()))
    assert float(grads[3].abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    c = case.cases()[name]
    assert len(two_runs_bit_equal(c, _device_run)) == 1 + len(c.names)


@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """The chain of parts on the device and the fused op: both pass against the same fp64 run."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("module-"))
def test_in_a_module(name):
    """Three nn.Linear projections, e = lin_edge(edge_attr).view(E, H, F), dot_attention_edge, a sum: out and the gradients that reach
    x, the three weights and lin_edge.weight."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda q, k, v, e: pg.dot_attention_edge(pattern, q, k, v, e)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x = c.x.float().to(DEV).requires_grad_(True)
    out = module(x)
    out.sum().backward()
    c.price(out.detach(), x.grad, *[module.get_parameter(n).grad for n in c.NAMES])


def test_a_strided_e_gives_the_result_of_its_copy():
    """e as a slice of a wider tensor (non-contiguous) and the gradient that flows back into the wider tensor."""
    import pygat_amd as pg
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    q, k, v, e = to_leaves(c.leaves)
    G = c.G.float().to(DEV)
    want = pg.dot_attention_edge(pattern, q, k, v, e)
    wgrads = torch.autograd.grad(want, [q, k, v, e], G)
    wide = torch.randn(e.shape[0], c.H, 2 * c.F + 4, device=DEV)
    wide[:, :, 4:4 + c.F] = e.detach()
    wide.requires_grad_(True)
    sl = wide[:, :, 4:4 + c.F]
    assert not sl.is_contiguous()
    got = pg.dot_attention_edge(pattern, q, k, v, sl)
    ggrads = torch.autograd.grad(got, [q, k, v, wide], G)
    assert torch.equal(got, want)
    for g, w in zip(ggrads[:3], wgrads[:3]):
        assert torch.equal(g, w)
    assert torch.equal(ggrads[3][:, :, 4:4 + c.F], wgrads[3])
    assert float(ggrads[3][:, :, :4].abs().max()) == 0.0 and float(ggrads[3][:, :, 4 + c.F:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------- launches and refusals
def test_only_the_needed_launches(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    mod = importlib.import_module("pygat_amd.dot_attention")
    c = case.cases()["bias-hub-8x16-indices"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]                # q, k, v, e, bias
    pattern = _pattern(c)
    with torch.no_grad():
        pg.dot_attention_edge(pattern, *tensors[:4], bias=tensors[4])
        pg.dot_attention_edge(pattern, *tensors[:4])
    assert seen == [EFWD, EFWD] and not pattern.has_transpose

    # what backward_rows is handed as de, and every [E, H, F]-sized tensor backward makes
    handed, made = [], []
    real_rows, real_empty = mod.lib.pygat_dot_attn_edge_backward_rows, torch.empty
    E, HF = c.row.numel(), c.H * c.F

    def rows(*args):
        assert len(args) == 33 and args[15] == HF and args[29] == HF        # (lde and ldde, each behind its table)
        handed.append(args[28])                                     # (de)
        return real_rows(*args)

    def empty(*size, **kw):
        t = real_empty(*size, **kw)
        if t.numel() >= E * HF:
            made.append(tuple(t.shape))
        return t
    monkeypatch.setattr(mod.lib, "pygat_dot_attn_edge_backward_rows", rows, raising=False)
    monkeypatch.setattr(mod.torch, "empty", empty)
    for needs in itertools.product((False, True), repeat=5):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.dot_attention_edge(pattern, *leaves[:4], bias=leaves[4])
        wanted = [t for t, n in zip(leaves, needs) if n]
        del seen[:], handed[:], made[:]
        grads = torch.autograd.grad(out, wanted, G)
        assert seen == [EROWS] + [SPMM] * (needs[1] + needs[2]), (needs, seen)
        assert pattern.has_transpose == (needs[1] or needs[2]), "neither dq, de nor db builds the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
        assert len(handed) == 1 and (handed[0] is not None) == needs[3], (needs, handed)
        assert made == ([(E, HF)] if needs[3] else []), (needs, made)
    # no entries: zeros of the right shapes, nothing launched in either pass
    empty_pattern = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    q0, k0, v0 = (torch.randn(n, 2, 8, device=DEV, requires_grad=True) for n in (5, 7, 7))
    e0 = torch.zeros(0, 2, 8, device=DEV, requires_grad=True)
    for shape in ((0, 2), (0,), None):
        b0 = None if shape is None else torch.zeros(shape, device=DEV, requires_grad=True)
        del seen[:]
        out = pg.dot_attention_edge(empty_pattern, q0, k0, v0, e0, bias=b0)
        leaves = [q0, k0, v0, e0] + ([] if b0 is None else [b0])
        grads = torch.autograd.grad(out, leaves, torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, leaves)) and grads[3].numel() == 0
        assert all(float(g.abs().max()) == 0.0 for g in grads[:3])
        assert seen == [], seen


def test_refusals(monkeypatch):
    import copy
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
    for args, e, needle in (((pattern, q, k, v), [0.0] * E, "e must be a tensor on the GPU"),
                            ((pattern, q, k, v), torch.zeros(E, 4, 16), "e must be a tensor on the GPU"),
                            ((pattern, q, k, v), t(E, 4, 16).double(), "e must be float32, not torch.float64"),
                            ((pattern, q, k, v), t(E, 4, 16).half(), "e must be float32"),
                            ((pattern, q, k, v), t(E, 4, 16).bfloat16(), "k, v and e must be float32"),
                            ((pattern, q, k.bfloat16(), v.bfloat16()), t(E, 4, 16), "k, v and e must be float32"),
                            ((elsewhere, q, k, v), t(E, 4, 16), "e lives on cuda:0, the pattern on cuda:1"),
                            ((pattern, q, k, v), t(E, 4, 8), f"e [{E}, 4, 16] expected"),
                            ((pattern, q, k, v), t(E, 4, 8), f"got ({E}, 4, 8)"),
                            ((pattern, q, k, v), t(E + 1, 4, 16), f"got ({E + 1}, 4, 16)"),
                            ((pattern, q, k, v), t(N, 4, 16), f"got ({N}, 4, 16)"),
                            ((pattern, q, k, v), t(E, 64), f"got ({E}, 64)"),
                            ((pattern, q, k, v), t(E, 4), f"got ({E}, 4)"),
                            ((pattern, q[:, 0], k[:, 0], v[:, 0]), t(E, 1, 16), f"e [{E}, 16] expected"),
                            ((pattern, q, k, v.cpu()), t(E, 4, 16), "v must be a tensor on the GPU"),
                            ((pattern, q, k, t(N, 4, 12)), t(E, 4, 16), "does not match q"),
                            ((pattern, t(N, 4, 12), t(N, 4, 12), t(N, 4, 12)), t(E, 4, 12), "F = 12"),
                            ((pattern, t(N, 8, 256), t(N, 8, 256), t(N, 8, 256)), t(4, 8, 256), "H * F = 8 * 256 = 2048")):
        with pytest.raises(ValueError, match="dot_attention_edge") as err:
            pg.dot_attention_edge(*args, e)
        assert needle in str(err.value), (needle, str(err.value))
    with pytest.raises(ValueError, match="dot_attention_edge: bias"):
        pg.dot_attention_edge(pattern, q, k, v, t(E, 4, 16), bias=t(E, 8))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient is refused as in dot_attention
    mod = importlib.import_module("pygat_amd.dot_attention")
    leaves = [x.clone().requires_grad_(True) for x in (q, k, v, t(E, 4, 16))]
    out = pg.dot_attention_edge(pattern, *leaves)
    del seen[:]
    with pytest.raises(ValueError, match="dot_attention_edge.*float32"):
        mod._DotAttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_edge_kernels_have_no_scratch():
    assert len(K19E) == 80 and len(set(K19E)) == 80
    no_scratch(K19E, (b"k19e_fwd_row_l3v1", b"k19e_fwd_row_l32v2", b"k19e_fwd_row_l64v5", b"k19e_mid_row_l8v1", b"k19e_fwd_row_l8v1x", b"k19e_",
                      b"k19e", b"k19eb_", b"k19efwd_row_l8v1", b"k19ee_fwd_row_l8v1", b"k19eh_fwd_row_l8v1", b"k19ed_fwd_row_l8v1",
                      b"k19be_fwd_row_l8v1"))
