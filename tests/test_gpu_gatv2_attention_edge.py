"""pygat_amd.gatv2_attention_edge (the EDGE instantiations of csrc/k21_gatv2_attention.hip, pygat_amd/gatv2_attention.py):
softmax(a . LeakyReLU(x_dst_i + x_src_j + e_c))-weighted sums of v_j over the entries of every row of a pattern, per head, fused; its
gradients in x_dst, x_src, a, v and e.

Ground truth, inputs and the seeded cases live in gatv2_attention_edge_case.py: torch autograd in fp64 on the CPU, loss L = <out, G>,
pricing by parity.check_autograd unchanged (out by close_fwd, every gradient by close_grad, de among them).  Every seeded case is
rehearsed on the CPU, the fp32 ground-truth run standing in for the device, by tests/test_gatv2_attention_edge_abi.py and passes there;
no case is built here."""
import copy
import ctypes as C
import importlib
import itertools

import pytest
import torch

import gatv2_attention_edge_case as case
from pattern_device import DEV, _Spy, _pattern, degree, device_run, two_runs_bit_equal
from pattern_device import leaves as _leaves

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K21E = ([f"k21e_{d}_{kind}_l{l}v{v}" for d in ("fwd", "bwd", "col") for kind in ("long", "row") for l, v in SHAPES]
        + [f"k21es_{d}_{kind}_l{l}v{v}" for d in ("fwd", "bwd") for kind in ("long", "row") for l, v in SHAPES])
FWD, ROWS, COLS = "pygat_v2_attn_edge_forward", "pygat_v2_attn_edge_backward_rows", "pygat_v2_attn_edge_backward_cols"
SPMM = "pygat_spmm_forward"


def _fused(pattern, c):
    """leaves = (x_dst, x_src, a, [v,] e), the case's order."""
    import pygat_amd as pg
    return lambda x_dst, x_src, a, *rest: pg.gatv2_attention_edge(pattern, x_dst, x_src, a, rest[-1], rest[0] if len(rest) == 2 else None,
                                                                  c.slope)


def _from_parts(pattern, c):
    import pygat_amd as pg
    row, col = c.row.to(DEV), c.col.to(DEV)

    def run(x_dst, x_src, a, *rest):
        s = (a * torch.nn.functional.leaky_relu(x_dst[row] + x_src[col] + rest[-1], c.slope)).sum(-1)
        return pg.spmm(pattern, pg.edge_softmax(pattern, s), rest[0] if len(rest) == 2 else x_src)
    return run


def _device_run(pattern, c, fn=None, leaves=None):
    """-> (out, dx_dst, dx_src, da, [dv,] de) on the device."""
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
    """Every slot of a chunk and a row of three chunks, and the same patterns with rows and columns swapped: scores of std 3.  de of an
    entry of a long row is written by the piece kernel: every row of it is priced."""
    c, res = (lambda r: (r[0], r[1:]))(_run_case(name))
    de = res[-1]
    long_rows = (degree(c) > 512)[c.row].to(DEV)
    assert int(long_rows.sum()) > 512 and bool((de[long_rows].abs().amax(dim=(1, 2)) > 0.0).all()), "no row of de is left unwritten"


# ------------------------------------------------------------------------------------------------- rectangular, unsorted, repeats
@pytest.mark.parametrize("name", case.case_names("rect-"))
def test_rectangular_with_empty_rows_and_columns(name):
    """Unsorted entries: only the permutation places a row of e and a row of de.  A row without entries gives exact zeros in out and
    dx_dst; a column without entries in dx_src (and dv)."""
    res = _run_case(name)
    c, out, dd, ds = res[:4]
    assert bool((c.row[1:] < c.row[:-1]).any()), "the entries are unsorted"
    no_row = (degree(c) == 0).to(DEV)
    no_col = (torch.bincount(c.col, minlength=c.shape[1]) == 0).to(DEV)
    assert int(no_row.sum()) == 100 and int(no_col.sum()) == 125
    for t in (out[no_row], dd[no_row], ds[no_col]) + ((res[5][no_col],) if not c.shared else ()):
        assert float(t.abs().max()) == 0.0
    assert res[-1].shape == c.e.shape


def test_rows_and_columns_without_entries_at_the_end():
    """The column kernel's last work-group takes the columns behind the last entry; they and the rows behind it get exact zeros."""
    c, out, dd, ds, da, de = _run_case("tail-rect-3x8-shared")
    assert float(out[300:].abs().max()) == 0.0 and float(dd[300:].abs().max()) == 0.0 and float(ds[500:].abs().max()) == 0.0
    assert float(ds[:500].abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("repeats-"))
def test_repeated_pairs_are_separate_entries(name):
    """Unsorted entries, 5 % of them repeated: each repeat takes its own row of e and gets its own row of de."""
    res = _run_case(name)
    c, de = res[0], res[-1]
    pairs = c.pairs.to(DEV)
    assert pairs.shape[0] > 100
    assert bool((de[pairs[:, 0]] != de[pairs[:, 1]]).flatten(1).any(1).all())


# ----------------------------------------------------------------------------------------------------------------- exact results
@pytest.mark.parametrize("name", case.case_names("lonely-"))
def test_a_row_of_one_entry_is_exact(name):
    res = _run_case(name)
    c, out, dd, de = res[0], res[1], res[2], res[-1]
    deg = degree(c)
    single = deg[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= 12
    v = (c.x_src if c.shared else c.v).float().to(DEV)
    assert torch.equal(out[rows], v[cols]), "out_i == v_j bit for bit"
    assert float(dd[rows].abs().max()) == 0.0, "the one S of the row is an exact zero, and dx_dst_i with it"
    assert float(de[single.to(DEV)].abs().max()) == 0.0, "... and the entry's row of de"
    assert bool((de[(~single).to(DEV)].abs().amax(dim=(1, 2)) > 0.0).all())


@pytest.mark.parametrize("name", case.case_names("zero-"))
def test_e_of_zeros_gives_the_bits_of_gatv2_attention(name):
    """out, dx_dst, dx_src, da and dv of gatv2_attention_edge with e = 0 against gatv2_attention on the same inputs, bit for bit."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    res = _device_run(pattern, c)
    c.price(*res)
    leaves = [t.float().to(DEV).requires_grad_(True) for t in c.inner.leaves]
    out = pg.gatv2_attention(pattern, *leaves[:3], None if c.shared else leaves[3], c.slope)
    want = (out.detach(),) + torch.autograd.grad(out, leaves, c.G.float().to(DEV))
    assert len(want) == len(res) - 1
    for got, ref, what in zip(res, want, ["out"] + c.inner.names):
        assert torch.equal(got, ref), (name, what)


@pytest.mark.parametrize("name", case.case_names("slope-"))
def test_slopes(name):
    """Slopes 0.2, 0 and 1; at slope 1 the result is priced against the linear score's ground truth as well (price_all)."""
    _run_case(name)


def test_the_slope_at_the_kink():
    """The tables on the grid of 2^-10: t is exact, some t are exactly 0 (asserted on the CPU), and the slope is taken there in the
    value and in the derivative, as torch does: the fp64 ground truth prices de, dx_dst, dx_src and da."""
    c = _run_case("grid-hub-8x16-indices-separate")[0]
    assert int((c.t() == 0).sum()) >= 20


@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    """out and every gradient, de and da -- the staged reduce of per-wave records -- included; a hub case and long-column cases."""
    c = case.cases()[name]
    assert len(two_runs_bit_equal(c, _device_run)) == 1 + len(c.names)


@pytest.mark.parametrize("name", case.case_names("strided-"))
def test_a_row_strided_e_gives_the_bits_of_its_copy(name, monkeypatch):
    """e as a column slice of a wider tensor (row stride a multiple of 4 floats, a 16-byte offset) is read in place -- the launchers see
    its leading dimension -- and every output has the bits of the run on its contiguous copy; the gradient arrives in the wide tensor."""
    mod = importlib.import_module("pygat_amd.gatv2_attention")
    seen = []

    class Ld:
        def __init__(self, real):
            self._real = real

        def __getattr__(self, name):
            fn = getattr(self._real, name)
            if not name.startswith("pygat_v2_attn_edge"):
                return fn

            def wrapped(*args):
                seen.append((name, args[14] if name.endswith("cols") else args[16]))          # lde
                return fn(*args)
            return wrapped
    monkeypatch.setattr(mod, "lib", Ld(mod.lib))
    c = case.cases()[name]
    pattern = _pattern(c)
    plain = _device_run(pattern, c)
    HF, E = c.H * c.F, c.row.numel()
    assert [ld for _, ld in seen] == [HF] * 3
    del seen[:]
    leaves = _leaves(c)
    wide = torch.randn(E, HF + 12, device=DEV)
    wide[:, 4:4 + HF] = leaves[-1].detach().view(E, HF)
    wide.requires_grad_(True)
    e = wide[:, 4:4 + HF].view(c.e.shape)
    assert not e.is_contiguous()
    got = _device_run(pattern, c, leaves=leaves[:-1] + [wide], fn=lambda p, cc: (lambda *lv: _fused(p, cc)(*lv[:-1], e)))
    assert [ld for _, ld in seen] == [HF + 12] * 3, "no copy: the launchers were given the wide tensor's row stride"
    for p, q, what in zip(plain[:-1], got[:-1], ["out"] + c.names[:-1]):
        assert torch.equal(p, q), what
    assert torch.equal(got[-1][:, 4:4 + HF], plain[-1].view(E, HF))
    assert float(got[-1][:, :4].abs().max()) == 0.0 and float(got[-1][:, 4 + HF:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ composition
@pytest.mark.parametrize("name", case.case_names("composed-"))
def test_fused_against_the_composition(name):
    """spmm(edge_softmax((a * leaky_relu(x_dst[row] + x_src[col] + e)).sum(-1)), v) on the device and the fused op: both pass against
    the same fp64 run."""
    c = case.cases()[name]
    pattern = _pattern(c)
    c.price(*_device_run(pattern, c), what=name + " fused")
    c.price(*_device_run(pattern, c, _from_parts), what=name + " from parts")


@pytest.mark.parametrize("name", case.case_names("module-"))
def test_a_bipartite_gatv2_layer_with_edge_features(name):
    """x_src through W_l, x_dst through W_r, edge_attr through lin_edge to [E, H, F], gatv2_attention_edge with v=None over a
    rectangular pattern, ELU, a sum: out and the gradients that reach x_src, x_dst, edge_attr, W_l, W_r, a and lin_edge's weight."""
    import pygat_amd as pg
    c = case.cases()[name]
    pattern = _pattern(c)
    module = c.module(lambda h_dst, h_src, a, e: pg.gatv2_attention_edge(pattern, h_dst, h_src, a, e, None, c.slope)).to(DEV)
    for n, w in zip(c.NAMES, c.weights):
        assert torch.equal(module.get_parameter(n).detach().cpu().double(), w)
    x_src, x_dst, edge_attr = (t.float().to(DEV).requires_grad_(True) for t in (c.x_src, c.x_dst, c.edge_attr))
    out = module(x_src, x_dst, edge_attr)
    out.sum().backward()
    assert module.lin_edge.weight.grad is not None and float(module.lin_edge.weight.grad.abs().max()) > 0.0
    c.price(out.detach(), x_src.grad, x_dst.grad, edge_attr.grad, *[module.get_parameter(n).grad for n in c.NAMES])


# ---------------------------------------------------------------------------------------------------------- launches and refusals
class _ArgSpy(_Spy):
    """_Spy that also keeps the arguments of the row pass."""

    def __init__(self, real, seen, rows):
        super().__init__(real, seen)
        self._rows = rows

    def __getattr__(self, name):
        fn = super().__getattr__(name)
        if name != ROWS:
            return fn

        def wrapped(*args):
            self._rows.append(args)
            return fn(*args)
        return wrapped


def _spied(monkeypatch, rows=None):
    seen = []
    for mod in ("pygat_amd.gatv2_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax"):
        m = importlib.import_module(mod)
        monkeypatch.setattr(m, "lib", _Spy(m.lib, seen) if rows is None or not mod.endswith("gatv2_attention") else
                            _ArgSpy(m.lib, seen, rows))
    return seen


def test_only_the_needed_launches(monkeypatch):
    """x_dst or e alone: the row pass, and the transposed pattern is never built; x_src or a: the column pass besides; v: K17 besides.
    e not required: the row pass gets a null de and no [E, H, F] tensor is made."""
    import pygat_amd as pg
    rows = []
    seen = _spied(monkeypatch, rows)
    c = case.cases()["lanes-hub-8x16-indices-separate"]
    G = c.G.float().to(DEV)
    tensors = [t.float().to(DEV) for t in c.leaves]                 # x_dst, x_src, a, v, e
    E, HF = c.row.numel(), c.H * c.F
    pattern = _pattern(c)
    with torch.no_grad():
        pg.gatv2_attention_edge(pattern, *tensors[:3], tensors[4])
        pg.gatv2_attention_edge(pattern, *tensors[:3], tensors[4], tensors[3])
    assert seen == [FWD, FWD] and not pattern.has_transpose
    empties = []
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *size, **kw: empties.append(tuple(size)) or real_empty(*size, **kw))
    for needs in itertools.product((False, True), repeat=5):
        if not any(needs):
            continue
        pattern = _pattern(c)                                       # (a fresh one: has it built its transpose?)
        del seen[:], rows[:], empties[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors, needs)]
        out = pg.gatv2_attention_edge(pattern, *leaves[:3], leaves[4], leaves[3], c.slope)
        wanted = [t for t, n in zip(leaves, needs) if n]
        grads = torch.autograd.grad(out, wanted, G)
        cols = needs[1] or needs[2]
        assert seen == [FWD, ROWS] + [COLS] * cols + [SPMM] * needs[3], (needs, seen)
        assert pattern.has_transpose == (cols or needs[3]), "dx_dst and de alone do not build the transpose"
        assert all(g.shape == t.shape for g, t in zip(grads, wanted))
        de, ldde = rows[0][27], rows[0][28]
        assert (de is not None) == needs[4] and ldde == HF, (needs, de)
        assert ((E, HF) in empties) == needs[4], "no [E, H F] tensor is made where de is not asked for"
    monkeypatch.setattr(torch, "empty", real_empty)
    # v=None: x_src is the value table too, so its gradient takes the column pass and K17; a alone takes the column pass only
    for needs, want in (((True, False, False, False), [FWD, ROWS]), ((False, True, False, False), [FWD, ROWS, COLS, SPMM]),
                        ((False, False, True, False), [FWD, ROWS, COLS]), ((False, False, False, True), [FWD, ROWS])):
        pattern = _pattern(c)
        del seen[:]
        leaves = [t.clone().requires_grad_(n) for t, n in zip(tensors[:3] + tensors[4:], needs)]
        out = pg.gatv2_attention_edge(pattern, *leaves, None, c.slope)
        torch.autograd.grad(out, [t for t, n in zip(leaves, needs) if n], G)
        assert seen == want and pattern.has_transpose == (len(want) > 2), (needs, seen)
    # no entries: zeros of the right shape, and nothing is launched
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    xd, xs, a0, v0, e0 = (torch.randn(*dims, device=DEV, requires_grad=True) for dims in ((5, 2, 8), (7, 2, 8), (2, 8), (7, 2, 8), (0, 2, 8)))
    for leaves, v in (([xd, xs, a0, e0], None), ([xd, xs, a0, e0, v0], v0)):
        del seen[:]
        out = pg.gatv2_attention_edge(empty, xd, xs, a0, e0, v)
        grads = torch.autograd.grad(out, leaves, torch.ones_like(out))
        assert out.shape == (5, 2, 8) and float(out.detach().abs().max()) == 0.0
        assert all(g.shape == t.shape for g, t in zip(grads, leaves)) and all(g.numel() == 0 or float(g.abs().max()) == 0.0 for g in grads)
        assert seen == [] and not empty.has_transpose, seen


def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices-shared"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    xd, xs, a, v, e = t(N, 4, 16), t(N, 4, 16), t(4, 16), t(N, 4, 16), t(E, 4, 16)
    elsewhere = copy.copy(pattern)
    elsewhere.device = torch.device("cuda", 1)                    # (a pattern that says it lives on another device: no second GPU needed)
    ok = (pattern, xd, xs, a, e)
    for args, kw, needle in (
            ((object(), xd, xs, a, e), {}, "an EdgePattern expected"),
            (ok, dict(negative_slope=float("nan")), "negative_slope = nan: a finite float expected"),
            ((pattern, xd, xs, a, e.cpu()), {}, "e must be a tensor on the GPU (there is no CPU path); e [E, H, F]"),
            ((pattern, xd, xs, a, None), {}, "e must be a tensor on the GPU"),
            ((pattern, xd, xs, a, e.double()), {}, "e must be float32, not torch.float64"),
            ((pattern, xd, xs, a, e.bfloat16()), {}, "x_dst, x_src, a, v and e must be float32"),
            ((pattern, xd, xs.bfloat16(), a, e), {}, "x_dst, x_src, a, v and e must be float32"),
            ((elsewhere, xd, xs, a, e), {}, "e lives on cuda:0, the pattern on cuda:1"),
            ((pattern, xd.cpu(), xs, a, e), {}, "x_dst must be a tensor on the GPU"),
            (ok, dict(v=v.double()), "v must be float32, not torch.float64"),
            ((pattern, xd, xs, a, t(E + 1, 4, 16)), {}, f"e [{E}, 4, 16] expected for E = {E} entries"),
            ((pattern, xd, xs, a, t(E - 1, 4, 16)), {}, f"got ({E - 1}, 4, 16)"),
            ((pattern, xd, xs, a, t(E, 4, 8)), {}, f"got ({E}, 4, 8)"),
            ((pattern, xd, xs, a, t(E, 2, 16)), {}, f"got ({E}, 2, 16)"),
            ((pattern, xd, xs, a, t(E, 64)), {}, f"got ({E}, 64)"),
            ((pattern, xd, t(N, 3, 16), a, e), {}, "x_src (%d, 3, 16) does not match x_dst" % N),
            ((pattern, xd, xs, t(4, 8), e), {}, "a (4, 8) does not match x_dst"),
            ((pattern, t(N + 1, 4, 16), xs, a, e), {}, f"x_dst has {N + 1} rows but the pattern has {N} rows"),
            ((pattern, t(N, 65, 4), t(N, 65, 4), t(65, 4), t(E, 65, 4)), {}, "H = 65 heads: the limits are 1 <= H <= 64"),
            ((pattern, t(N, 4, 12), t(N, 4, 12), t(4, 12), t(E, 4, 12)), {}, "F = 12: a head's width must be a power of two in 4..256"),
            ((pattern, t(N, 8, 256), t(N, 8, 256), t(8, 256), t(8, 8, 256)), {}, "H * F = 8 * 256 = 2048 floats per row")):
        with pytest.raises(ValueError, match="gatv2_attention_edge") as err:
            pg.gatv2_attention_edge(*args, **kw)
        assert needle in str(err.value), (needle, str(err.value))
    assert seen == [] and not pattern.has_transpose
    # an fp64 incoming gradient
    mod = importlib.import_module("pygat_amd.gatv2_attention")
    leaves = [x.clone().requires_grad_(True) for x in (xd, xs, a, e)]
    out = pg.gatv2_attention_edge(pattern, *leaves)
    del seen[:]
    with pytest.raises(ValueError, match="gatv2_attention_edge: the gradient of the output must be float32, not torch.float64"):
        mod._Gatv2AttentionFn.backward(out.grad_fn, torch.ones(N, 4, 16, device=DEV, dtype=torch.float64))
    assert seen == []


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_no_kernel_uses_scratch():
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    assert len(K21E) == 100
    for name in K21E:
        assert lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)) == 0, (name, lib.pygat_last_error())
        assert scratch.value == 0 and regs.value > 0, (name, regs.value, scratch.value)
    for bad in (b"k21es_col_row_l8v1", b"k21e_fwd_row_l3v1", b"k21e_fwd_row_l64v5", b"k21e_mid_row_l8v1", b"k21e_", b"k21ed_fwd_row_l8v1",
                b"k21de_fwd_row_l8v1", b"k21se_fwd_row_l8v1", b"k21es_bwd_row_l0v1", b"k21e_col_mid_l8v1", b"k21e_fwd_row_l8v1x"):
        assert lib.pygat_kernel_footprint(bad, C.byref(regs), C.byref(scratch)) == -1, bad
        assert b"k21{,s,d,ds,e,es}_" in lib.pygat_last_error() and b"k21{,e}_col_" in lib.pygat_last_error()
