"""pygat_amd.dot_attention on bfloat16 k and v tables, the inference forward (the bf16-table instantiations of the two forward kernels of
csrc/k19_dot_attention.hip).

The contract is bit equality: dot_attention(p, q, k16, v16, s, b) is dot_attention(p, q, k16.float(), v16.float(), s, b), the float32
op on the widened tables -- a lane's chunk is the same 4 row elements, loaded as 8 bytes and widened in registers, and everything after
the load is the float32 kernels' -- so those tests carry no tolerance.  Beside it the op is priced against the fp64 ground truth on the
widened tables by the one rule of parity.py, so that this file does not lean on the float32 kernels alone.  The seeded cases live in
dot_attention_bf16_case.py and are rehearsed on the CPU by tests/test_dot_attention_bf16_abi.py; no case is built here."""

import pytest
import torch

import dot_attention_bf16_case as case
from pattern_device import DEV, FWD, _indices_pattern, _pattern, degree, no_scratch, spied  # noqa: F401

pytestmark = pytest.mark.gpu

HFWD = "pygat_dot_attn_bf16_forward"
SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K19H = [f"{prefix}_fwd_{kind}_l{l}v{v}" for prefix in ("k19h", "k19hb") for kind in ("long", "row") for l, v in SHAPES]


def _inputs(c):
    """-> (q, k16, v16, bias | None) on the device."""
    bias = None if c.bias is None else c.bias.float().to(DEV)
    return c.q.float().to(DEV), c.k16.to(DEV), c.v16.to(DEV), bias


def _attend(pattern, c, q, k, v, bias):
    import pygat_amd as pg
    with torch.no_grad():
        out = pg.dot_attention(pattern, q, k, v, c.fed_scale, bias)
    assert out.dtype == torch.float32 and out.shape == q.shape and not out.requires_grad
    return out


def _both(c, pattern=None):
    """-> (out on the bf16 tables, out of the float32 op on the widened tables)."""
    pattern = pattern or _pattern(c)
    q, k16, v16, bias = _inputs(c)
    return _attend(pattern, c, q, k16, v16, bias), _attend(pattern, c, q, k16.float(), v16.float(), bias)


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.dot_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("name", case.case_names())
def test_the_bits_of_the_float32_op_on_the_widened_tables(name):
    """Every lane shape on the hub pattern (a row of 699 entries: the long-row launch too), with and without a permutation; two
    chunks per lane at 8x64; the asymmetric pattern with its rows of one entry; no head axis; nine rows of 521 entries and a row over
    three chunks; and with a bias: unsorted and repeated entries, which only the permutation gives their own bias, a [E] bias shared
    by the heads, masked entries, a bias of zeros."""
    c = case.cases()[name]
    got, want = _both(c)
    assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert float(got.abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("bias-zero-"))
def test_a_bias_of_zeros_against_no_bias(name):
    c = case.cases()[name]
    plain = case.cases()["plain-" + name[len("bias-zero-"):]]
    assert plain.inner is c.inner.inner and c.bias is not None and plain.bias is None
    pattern = _pattern(c)
    assert torch.equal(_attend(pattern, c, *_inputs(c)), _attend(pattern, plain, *_inputs(plain))), name


# ------------------------------------------------------------------------------------------------------------ parity with fp64
PRICED = ([f"plain-lanes-hub-{H}x{F}-indices" for H, F in case.LANE_SHAPES + (case.WIDE_SHAPE,)]
          + ["plain-lanes-hub-noaxis-indices", "plain-lanes-hub-noaxis-graph", "plain-lanes-asym-12x64-indices"]
          + case.case_names("plain-long-") + case.case_names("bias-long-") + case.case_names("bias-masked-")
          + ["bias-rect-3x8", "bias-repeats-8x16", "bias-shared-hub-8x16-indices", "bias-lanes-hub-8x64-graph"])


@pytest.mark.parametrize("name", PRICED)
def test_against_fp64_on_the_widened_tables(name):
    """One case per lane shape, the long rows and the kinds of bias against the fp64 ground truth on k16.double(), v16.double(): out
    by parity.close_fwd with the fp32 ground-truth run's own error, the rule of every forward here."""
    c = case.cases()[name]
    c.price(_attend(_pattern(c), c, *_inputs(c)))


# ------------------------------------------------------------------------------------- the bf16 kernels ran, nothing was widened
def test_only_the_bf16_launcher_runs(monkeypatch):
    seen = _spied(monkeypatch)
    for name in ("plain-lanes-asym-8x16-indices", "bias-rect-3x8", "plain-long-nine_hubs-8x16-graph"):
        c = case.cases()[name]
        pattern = _pattern(c)
        tensors = _inputs(c)
        del seen[:]
        _attend(pattern, c, *tensors)
        assert seen == [HFWD], (name, seen)
        assert c.kind == "graph" or not pattern.has_transpose, "(a graph's pattern shares the graph's transpose from the start)"
    del seen[:]
    _attend(pattern, c, tensors[0], tensors[1].float(), tensors[2].float(), tensors[3])
    assert seen == [FWD], "float32 tables: the entry point of the op as it was"


def test_no_widened_copy_is_made():
    """At 12x64 on the hub pattern the call may allocate its result and the workspace of the long rows and nothing of a table's size.
    The pattern is square, so the result [n_rows, 768] fp32 is itself exactly as large as one widened table [n_cols, 768] fp32: the
    peak of the allocator over the call, less the result it returns, must stay below one widened table -- a single fp32 copy of k or
    of v, however short-lived, would break that."""
    c = case.cases()["plain-lanes-hub-12x64-indices"]
    pattern = _pattern(c)
    q, k16, v16, bias = _inputs(c)
    _attend(pattern, c, q, k16, v16, bias)                              # (anything made once per pattern or process is made here)
    widened = k16.numel() * 4
    assert widened == v16.numel() * 4 == 2 * k16.numel() * k16.element_size()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _attend(pattern, c, q, k16, v16, bias)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    result = out.numel() * out.element_size()
    print(f"peak over the call {delta} bytes, the result {result}, one widened table {widened}")
    assert result <= delta and delta - result < widened, (delta, result, widened)


# ------------------------------------------------------------------------------------------------- reproducible, exact cases
@pytest.mark.parametrize("name", ["plain-twice-nine_hubs-8x16-indices", "plain-twice-hub-3x8-graph", "bias-twice-nine_hubs-8x16-indices"])
def test_two_runs_are_bit_equal(name):
    c = case.cases()[name]
    pattern = _pattern(c)
    tensors = _inputs(c)
    assert torch.equal(_attend(pattern, c, *tensors), _attend(pattern, c, *tensors))


def test_an_empty_pattern_gives_zeros_without_a_launch(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    q0 = torch.randn(5, 2, 8, device=DEV)
    k0, v0 = (torch.randn(7, 2, 8, device=DEV).bfloat16() for _ in range(2))
    del seen[:]
    for bias in (None, torch.zeros(0, 2, device=DEV), torch.zeros(0, device=DEV)):
        with torch.no_grad():
            out = pg.dot_attention(empty, q0, k0, v0, bias=bias)
        assert out.shape == (5, 2, 8) and out.dtype == torch.float32 and float(out.abs().max()) == 0.0
    assert seen == []


@pytest.mark.parametrize("name", case.case_names("plain-lonely-") + ["bias-lonely-8x16-indices", "plain-lanes-asym-12x64-indices"])
def test_a_row_of_one_entry_is_its_v_row(name):
    c = case.cases()[name]
    out = _attend(_pattern(c), c, *_inputs(c))
    single = degree(c)[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= (12 if "lonely" in name else 1)
    assert torch.equal(out[rows], c.v16.to(DEV)[cols].float()), "out_i == v16[j].float() bit for bit"


@pytest.mark.parametrize("name", case.case_names("bias-masked-"))
def test_a_masked_entry_contributes_exact_zeros(name):
    """bias = -9e15 on a third of the entries, never on the first of a row.  A row up to the long-row threshold (512 entries) is
    folded entry by entry in its order, and a masked entry folds in p = 0 exactly -- Z, the weighted sum and the running maximum
    stay as they are -- so its out row has the bits of the same row of the pattern without the masked entries.  (A longer row is
    split among lane groups by position, so dropping entries reorders its sum: those rows are priced against fp64 above.)"""
    import pygat_amd as pg
    c = case.cases()[name]
    assert c.kind == "indices" or c.csr is not None
    pattern = _indices_pattern(c.row, c.col, c.shape)
    q, k16, v16, bias = _inputs(c)
    out = _attend(pattern, c, q, k16, v16, bias)
    keep = ~c.masked
    kept = _indices_pattern(c.row[keep], c.col[keep], c.shape)
    with torch.no_grad():
        want = pg.dot_attention(kept, q, k16, v16, c.fed_scale, bias[keep.to(DEV)].contiguous())
    short = (degree(c) <= 512).to(DEV)
    assert int(short.sum()) > 0.9 * c.shape[0]
    assert torch.equal(out[short], want[short]), name
    some = torch.bincount(c.row[c.masked], minlength=c.shape[0]).to(DEV) > 0
    assert int((some & short).sum()) >= 100, "rows with a masked entry are among them"


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["plain-lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    N = c.shape[0]

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    q, k, v = t(N, 4, 16), t(N, 4, 16), t(N, 4, 16)
    k16, v16 = k.bfloat16(), v.bfloat16()
    with torch.no_grad():
        for args, needle in (((pattern, q, k16, v), "k is torch.bfloat16 and v is torch.float32"),
                             ((pattern, q, k, v16), "k is torch.float32 and v is torch.bfloat16"),
                             ((pattern, q, k16, v.half()), "both k and v as bfloat16"),
                             ((pattern, q.bfloat16(), k16, v16), "q must be float32, not torch.bfloat16"),
                             ((pattern, q.bfloat16(), k, v), "q must be float32, not torch.bfloat16"),
                             ((pattern, q, k.half(), v), "k must be float32"),
                             ((pattern, q, k.half(), v.half()), "k must be float32"),
                             ((pattern, q, k16.cpu(), v16), "k must be a tensor on the GPU"),
                             ((pattern, q, k16, t(N, 4, 32).bfloat16()), "v (500, 4, 32) does not match q"),
                             ((pattern, q, t(N + 2, 4, 16).bfloat16(), t(N + 2, 4, 16).bfloat16()), f"k has {N + 2} rows"),
                             ((pattern, t(N, 4, 12), t(N, 4, 12).bfloat16(), t(N, 4, 12).bfloat16()), "F = 12"),
                             ((pattern, t(N, 8, 256), t(N, 8, 256).bfloat16(), t(N, 8, 256).bfloat16()), "H * F = 8 * 256 = 2048")):
            with pytest.raises(ValueError, match="dot_attention") as err:
                pg.dot_attention(*args)
            assert needle in str(err.value), (needle, str(err.value))
        with pytest.raises(ValueError, match="dot_attention: bias must be float32"):
            pg.dot_attention(pattern, q, k16, v16, bias=t(c.row.numel(), 4).bfloat16())
        for args in ((pattern, q, k16), (pattern, q.bfloat16(), k16)):
            with pytest.raises(ValueError, match="edge_dot.*must be float32"):
                pg.edge_dot(*args)
    # inference only: a tensor that requires grad under grad mode is refused; the same call under no_grad runs
    bias = t(c.row.numel(), 4)
    for which in range(4):
        args = [x.clone().requires_grad_(i == which) if x.is_floating_point() else x for i, x in enumerate((q, k16, v16, bias))]
        with pytest.raises(ValueError, match="dot_attention: bfloat16 k and v are for inference") as err:
            pg.dot_attention(pattern, *args[:3], bias=args[3])
        assert "torch.no_grad()" in str(err.value) and "float32 tables" in str(err.value)
        assert seen == []
        with torch.no_grad():
            out = pg.dot_attention(pattern, *args[:3], bias=args[3])
        assert seen == [HFWD] and not out.requires_grad and out.grad_fn is None
        del seen[:]
    out = pg.dot_attention(pattern, q, k16, v16)                       # grad mode on, nothing requires grad: it runs
    assert seen == [HFWD] and not out.requires_grad and not pattern.has_transpose


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_bf16_kernels_have_no_scratch():
    assert len(K19H) == 40
    no_scratch(K19H, (b"k19h_bwd_row_l8v1", b"k19hb_bwd_long_l8v1", b"k19h_fwd_row_l3v1", b"k19h_fwd_row_l32v2", b"k19hb_fwd_row_l64v5",
                      b"k19h_fwd_row_l8v1x", b"k19h_", b"k19h", b"k19hb_", b"k19hc_fwd_row_l8v1", b"k19hfwd_row_l8v1"))
