"""pygat_amd.additive_attention_bf16, the inference forward on a bfloat16 v table (the BF16 instantiations of the two forward kernels of
csrc/k20_additive_attention.hip).

The contract is bit equality: additive_attention_bf16(p, s_dst, s_src, v16, slope, u) is additive_attention(p, s_dst, s_src, v16.float(),
slope, u), the float32 op on the widened table -- a lane's chunk is the same 4 row elements, loaded as 8 bytes and widened in
registers, and everything after the load is the float32 kernels' -- so those tests carry no tolerance.  Beside it the op is priced
against the fp64 ground truth on the widened table by the one rule of parity.py, so that this file does not lean on the float32
kernels alone.  The seeded cases live in additive_attention_bf16_case.py and are rehearsed on the CPU by
tests/test_additive_attention_bf16_abi.py; no case is built here."""
import pytest
import torch

import additive_attention_bf16_case as case
from pattern_device import DEV, _graph, _indices_pattern, _pattern, degree, no_scratch, spied

pytestmark = pytest.mark.gpu

HFWD, FWD = "pygat_add_attn_bf16_forward", "pygat_add_attn_forward"
SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K20H = [f"{prefix}_fwd_{kind}_l{l}v{v}" for prefix in ("k20h", "k20hu") for kind in ("long", "row") for l, v in SHAPES]


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.additive_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def _inputs(c):
    """-> (s_dst, s_src, v16, u | None) on the device."""
    u = None if c.u is None else c.u.float().to(DEV)
    return c.s_dst.float().to(DEV), c.s_src.float().to(DEV), c.v16.to(DEV), u


def _attend(pattern, c, s_dst, s_src, v, u):
    """The bf16 op on a bfloat16 v, the float32 op on a float32 one."""
    import pygat_amd as pg
    op = pg.additive_attention_bf16 if v.dtype == torch.bfloat16 else pg.additive_attention
    with torch.no_grad():
        out = op(pattern, s_dst, s_src, v, c.slope, u)
    assert out.dtype == torch.float32 and out.shape == c.G.shape and not out.requires_grad
    return out


def _both(c, pattern=None):
    """-> (out on the bf16 table, out of the float32 op on the widened table)."""
    pattern = pattern or _pattern(c)
    s_dst, s_src, v16, u = _inputs(c)
    return _attend(pattern, c, s_dst, s_src, v16, u), _attend(pattern, c, s_dst, s_src, v16.float(), u)


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("name", case.case_names())
def test_the_bits_of_the_float32_op_on_the_widened_table(name):
    """Every lane shape on the hub pattern (a row of 699 entries: the long-row launch too), with and without a permutation, without a
    logit and with a [E, H] one; two chunks per lane at 8x64; the asymmetric pattern with its rows of one entry; no head axis; nine
    rows of 521 entries and a row over three chunks; unsorted and repeated entries, which only the permutation gives their own logit;
    a [E] logit shared by the heads, masked entries, a logit of zeros."""
    c = case.cases()[name]
    got, want = _both(c)
    assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert float(got.abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("zero-"))
def test_a_logit_of_zeros_against_no_logit(name):
    c = case.cases()[name]
    assert float(c.u.abs().max()) == 0.0
    pattern = _pattern(c)
    s_dst, s_src, v16, u = _inputs(c)
    assert torch.equal(_attend(pattern, c, s_dst, s_src, v16, u), _attend(pattern, c, s_dst, s_src, v16, None)), name


# ------------------------------------------------------------------------------------------------------------ parity with fp64
PRICED = ([f"lanes-hub-{H}x{F}-indices" for H, F in case.LANE_SHAPES + (case.WIDE_SHAPE,)]
          + ["lanes-hub-noaxis-indices", "lanes-hub-noaxis-graph-logit", "lanes-asym-12x64-indices-logit", "lanes-hub-8x64-graph-logit"]
          + case.case_names("long-") + case.case_names("masked-")
          + ["rect-3x8-logit", "repeats-8x16-logit", "lanes-hub-3x8-indices-shared", "lanes-hub-12x64-graph-logit"])


@pytest.mark.parametrize("name", PRICED)
def test_against_fp64_on_the_widened_table(name):
    """One case per lane shape, the long rows and the kinds of logit against the fp64 ground truth on v16.double(): out by
    parity.close_fwd with the fp32 ground-truth run's own error, the rule of every forward here."""
    c = case.cases()[name]
    c.price(_attend(_pattern(c), c, *_inputs(c)))


# ------------------------------------------------------------------------------------- the bf16 kernels ran, nothing was widened
def test_only_the_bf16_launcher_runs(monkeypatch):
    seen = _spied(monkeypatch)
    for name in ("lanes-asym-8x16-indices", "rect-3x8-logit", "long-nine_hubs-8x16-graph-shared"):
        c = case.cases()[name]
        pattern = _pattern(c)
        tensors = _inputs(c)
        del seen[:]
        _attend(pattern, c, *tensors)
        assert seen == [HFWD], (name, seen)
        assert c.kind == "graph" or not pattern.has_transpose, "(a graph's pattern shares the graph's transpose from the start)"
    del seen[:]
    _attend(pattern, c, tensors[0], tensors[1], tensors[2].float(), tensors[3])
    assert seen == [FWD], "a float32 table: the entry point of the op as it was"


def test_no_widened_copy_is_made():
    """At 12x64 on the hub pattern the call may allocate its result and the workspace of the long rows and nothing of the table's
    size.  The pattern is square, so the result [n_rows, 768] fp32 is itself exactly as large as the widened table [n_cols, 768] fp32:
    the peak of the allocator over the call, less the result it returns, must stay below one widened table -- a single fp32 copy of
    v, however short-lived, would break that."""
    c = case.cases()["lanes-hub-12x64-indices-logit"]
    pattern = _pattern(c)
    tensors = _inputs(c)
    _attend(pattern, c, *tensors)                                       # (anything made once per pattern or process is made here)
    v16 = tensors[2]
    widened = v16.numel() * 4
    assert widened == 2 * v16.numel() * v16.element_size() and c.shape[0] == c.shape[1]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = _attend(pattern, c, *tensors)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    result = out.numel() * out.element_size()
    print(f"peak over the call {delta} bytes, the result {result}, one widened table {widened}")
    assert result <= delta and delta - result < widened, (delta, result, widened)


# ------------------------------------------------------------------------------------------------- reproducible, exact cases
@pytest.mark.parametrize("name", case.case_names("twice-"))
def test_two_runs_are_bit_equal(name):
    c = case.cases()[name]
    pattern = _pattern(c)
    tensors = _inputs(c)
    assert torch.equal(_attend(pattern, c, *tensors), _attend(pattern, c, *tensors))


def test_an_empty_pattern_gives_zeros_without_a_launch(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    s_dst, s_src, v16 = torch.randn(5, 2, device=DEV), torch.randn(7, 2, device=DEV), torch.randn(7, 2, 8, device=DEV).bfloat16()
    del seen[:]
    for u in (None, torch.zeros(0, 2, device=DEV), torch.zeros(0, device=DEV)):
        with torch.no_grad():
            out = pg.additive_attention_bf16(empty, s_dst, s_src, v16, edge_logit=u)
        assert out.shape == (5, 2, 8) and out.dtype == torch.float32 and float(out.abs().max()) == 0.0
    out = pg.additive_attention_bf16(empty, s_dst[:, 0].contiguous(), s_src[:, 0].contiguous(), v16[:, 0].contiguous())
    assert out.shape == (5, 8) and float(out.abs().max()) == 0.0
    assert seen == []


@pytest.mark.parametrize("name", case.case_names("lonely-") + ["lanes-asym-12x64-indices", "lanes-asym-3x8-indices-logit"])
def test_a_row_of_one_entry_is_its_v_row(name):
    c = case.cases()[name]
    out = _attend(_pattern(c), c, *_inputs(c))
    single = degree(c)[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= (12 if "lonely" in name else 1)
    assert torch.equal(out[rows], c.v16.to(DEV)[cols].float()), "out_i == v16[j].float() bit for bit"


@pytest.mark.parametrize("name", case.case_names("masked-"))
def test_a_masked_entry_contributes_exact_zeros(name):
    """edge_logit = -9e15 on a third of the entries, never on the first of a row.  A row up to the long-row threshold (512 entries) is
    folded entry by entry in its order, and a masked entry folds in p = 0 exactly -- Z, the weighted sum and the running maximum
    stay as they are -- so its out row has the bits of the same row of the pattern without the masked entries.  (A longer row is
    split among lane groups by position, so dropping entries reorders its sum: those rows are priced against fp64 above.)"""
    c = case.cases()[name]
    pattern = _indices_pattern(c.row, c.col, c.shape)
    s_dst, s_src, v16, u = _inputs(c)
    out = _attend(pattern, c, s_dst, s_src, v16, u)
    keep = ~c.masked
    kept = _indices_pattern(c.row[keep], c.col[keep], c.shape)
    want = _attend(kept, c, s_dst, s_src, v16, u[keep.to(DEV)].contiguous())
    short = (degree(c) <= 512).to(DEV)
    assert int(short.sum()) > 0.9 * c.shape[0]
    assert torch.equal(out[short], want[short]), name
    some = torch.bincount(c.row[c.masked], minlength=c.shape[0]).to(DEV) > 0
    assert int((some & short).sum()) >= 100, "rows with a masked entry are among them"


# ------------------------------------------------------------------------------------------------------------- sampled blocks
def test_a_sampled_block_with_gathered_bf16_rows():
    """The workload the op is for: a two-hop sample of a graph, the bf16 table of all nodes gathered by blk.src_nodes and a per-edge
    logit of the whole graph by blk.edge_ids, bit-equal to the float32 op on the widened gathers."""
    import pygat_amd as pg
    import sample_case
    t = sample_case.TWO_HOP
    g = _graph(*sample_case.graphs()[t["graph"]])
    seed = torch.tensor([t["seed"]], dtype=torch.int64, device=DEV)
    blocks = pg.sample_blocks(g, torch.as_tensor(sample_case.two_hop_seeds()).to(DEV), list(t["fanouts"]), seed=seed)
    gen = torch.Generator(device=DEV).manual_seed(7)
    H, F = 4, 16
    x16 = torch.randn(g.n, H, F, device=DEV, generator=gen).bfloat16()
    s = torch.randn(g.n, 2, H, device=DEV, generator=gen)
    u_full = torch.randn(g.nnz, H, device=DEV, generator=gen)
    for blk in blocks:
        s_dst, s_src = s[blk.dst_nodes, 0].contiguous(), s[blk.src_nodes, 1].contiguous()
        v16, u = x16[blk.src_nodes], u_full[blk.edge_ids]
        assert v16.dtype == torch.bfloat16 and blk.nnz > 0
        for logit in (None, u):
            with torch.no_grad():
                got = pg.additive_attention_bf16(blk.pattern, s_dst, s_src, v16, 0.2, logit)
                want = pg.additive_attention(blk.pattern, s_dst, s_src, v16.float(), 0.2, logit)
            assert got.shape == (blk.n_dst, H, F) and torch.equal(got, want) and float(got.abs().max()) > 0.0


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["lanes-asym-8x16-indices"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    s_dst, s_src, v = t(N, 4), t(N, 4), t(N, 4, 16)
    v16 = v.bfloat16()
    with torch.no_grad():
        for args, kw, needle in (((pattern, s_dst, s_src, v), {}, "v16 must be torch.bfloat16, not torch.float32"),
                                 ((pattern, s_dst, s_src, v.half()), {}, "v16 must be torch.bfloat16, not torch.float16"),
                                 ((pattern, s_dst.bfloat16(), s_src, v16), {}, "s_dst must be torch.float32, not torch.bfloat16"),
                                 ((pattern, s_dst, s_src.bfloat16(), v16), {}, "s_src must be torch.float32, not torch.bfloat16"),
                                 ((pattern, s_dst, s_src, v16), dict(edge_logit=t(E, 4).bfloat16()),
                                  "edge_logit must be torch.float32, not torch.bfloat16"),
                                 ((pattern, s_dst, s_src, v16.cpu()), {}, "v16 must be a tensor on the GPU"),
                                 ((pattern, s_dst, s_src, t(N, 5, 16).bfloat16()), {}, f"v16 ({N}, 5, 16) does not match s_dst"),
                                 ((pattern, s_dst, s_src, t(N + 2, 4, 16).bfloat16()), {}, f"v16 has {N + 2} rows"),
                                 ((pattern, s_dst, s_src, t(N, 4, 12).bfloat16()), {}, "F = 12"),
                                 ((pattern, t(N, 8), t(N, 8), t(N, 8, 256).bfloat16()), {}, "H * F = 8 * 256 = 2048"),
                                 ((pattern, s_dst, s_src, v16), dict(edge_logit=t(E, 3)), "edge_logit [E, H] = "),
                                 ((pattern, s_dst, s_src, v16), dict(negative_slope=float("nan")), "negative_slope = nan")):
            with pytest.raises(ValueError, match="additive_attention_bf16") as err:
                pg.additive_attention_bf16(*args, **kw)
            assert needle in str(err.value), (needle, str(err.value))
        # the float32 ops keep their refusals of bfloat16 tensors
        with pytest.raises(ValueError, match="additive_attention: v must be float32, not torch.bfloat16"):
            pg.additive_attention(pattern, s_dst, s_src, v16)
    assert seen == []
    # inference only: a tensor that requires grad under grad mode is refused; the same call under no_grad runs
    u = t(E, 4)
    for which in range(4):
        args = [x.clone().requires_grad_(i == which) for i, x in enumerate((s_dst, s_src, v16, u))]
        with pytest.raises(ValueError, match="additive_attention_bf16: bfloat16 tables are for inference") as err:
            pg.additive_attention_bf16(pattern, *args[:3], edge_logit=args[3])
        assert "torch.no_grad()" in str(err.value) and "use additive_attention on float32 tables" in str(err.value)
        assert seen == []
        with torch.no_grad():
            out = pg.additive_attention_bf16(pattern, *args[:3], edge_logit=args[3])
        assert seen == [HFWD] and not out.requires_grad and out.grad_fn is None
        del seen[:]
    out = pg.additive_attention_bf16(pattern, s_dst, s_src, v16, edge_logit=u)      # grad mode on, nothing requires grad: it runs
    assert seen == [HFWD] and not out.requires_grad and not pattern.has_transpose


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_bf16_kernels_have_no_scratch():
    assert len(K20H) == 40
    no_scratch(K20H, (b"k20h_bwd_row_l8v1", b"k20hu_bwd_long_l8v1", b"k20h_col_row_l8v1", b"k20h_fwd_row_l3v1", b"k20h_fwd_row_l32v2",
                      b"k20hu_fwd_row_l64v5", b"k20h_fwd_row_l8v1x", b"k20h_", b"k20h", b"k20hu_", b"k20hd_fwd_row_l8v1", b"k20hfwd_row_l8v1",
                      b"k20b_fwd_row_l8v1", b"k20hb_fwd_row_l8v1", b"k20dh_fwd_row_l8v1"))
