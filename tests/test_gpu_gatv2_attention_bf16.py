"""pygat_amd.gatv2_attention_bf16 and pygat_amd.gatv2_attention_edge_bf16, the inference forwards on bfloat16 tables (the BF16
instantiations of the two forward kernels of csrc/k21_gatv2_attention.hip, without and with EDGE).

The contract is bit equality: gatv2_attention_bf16(p, x_dst, x_src16, a, v16, slope) is gatv2_attention(p, x_dst, x_src16.float(), a,
v16.float(), slope), and gatv2_attention_edge_bf16 is gatv2_attention_edge on the widened x_src16, v16 and e16 -- a lane's chunk is the
same 4 row elements, loaded as 8 bytes and widened in registers, and everything after the load is the float32 kernels' -- so those tests
carry no tolerance.  Beside it the ops are priced against the fp64 ground truth on the widened tables by the one rule of parity.py, so
that this file does not lean on the float32 kernels alone.  The seeded cases live in gatv2_attention_bf16_case.py ("plain-..." and
"edge-...") and are rehearsed on the CPU by tests/test_gatv2_attention_bf16_abi.py; no case is built here."""
import importlib

import pytest
import torch

import gatv2_attention_bf16_case as case
from pattern_device import DEV, _graph, _pattern, degree, no_scratch, spied

pytestmark = pytest.mark.gpu

HFWD, HEFWD = "pygat_v2_attn_bf16_forward", "pygat_v2_attn_edge_bf16_forward"
FWD, EFWD = "pygat_v2_attn_forward", "pygat_v2_attn_edge_forward"
SHAPES = ((1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
K21H = [f"{prefix}_fwd_{kind}_l{l}v{v}" for prefix in ("k21h", "k21hs", "k21he", "k21hes") for kind in ("long", "row") for l, v in SHAPES]


def _spied(monkeypatch):
    return spied(monkeypatch, "pygat_amd.gatv2_attention", "pygat_amd.spmm", "pygat_amd.edge_softmax")


def _inputs(c):
    """-> (x_dst, x_src16, a, v16 | None, e16 | None) on the device."""
    return (c.x_dst.float().to(DEV), c.x_src16.to(DEV), c.a.float().to(DEV), None if c.v16 is None else c.v16.to(DEV),
            None if c.e16 is None else c.e16.to(DEV))


def _widened(tensors):
    return tuple(t.float() if t is not None and t.dtype == torch.bfloat16 else t for t in tensors)


def _attend(pattern, c, x_dst, x_src, a, v, e):
    """The bf16 ops on a bfloat16 x_src, the float32 ops on a float32 one; with e the edge op, without it the plain one."""
    import pygat_amd as pg
    bf16 = x_src.dtype == torch.bfloat16
    with torch.no_grad():
        if e is None:
            out = (pg.gatv2_attention_bf16 if bf16 else pg.gatv2_attention)(pattern, x_dst, x_src, a, v, c.slope)
        else:
            out = (pg.gatv2_attention_edge_bf16 if bf16 else pg.gatv2_attention_edge)(pattern, x_dst, x_src, a, e, v, c.slope)
    assert out.dtype == torch.float32 and out.shape == c.G.shape and not out.requires_grad
    return out


def _both(c, pattern=None):
    """-> (out on the bf16 tables, out of the float32 op on the widened tables)."""
    pattern = pattern or _pattern(c)
    tensors = _inputs(c)
    return _attend(pattern, c, *tensors), _attend(pattern, c, *_widened(tensors))


# ---------------------------------------------------------------------------------------------------------------- bit equality
@pytest.mark.parametrize("name", case.case_names())
def test_the_bits_of_the_float32_op_on_the_widened_tables(name):
    """Both ops: every lane shape on the hub pattern (a row of 699 entries: the long-row launch too), with and without a permutation,
    v shared and separate; two chunks per lane at 8x64; the asymmetric pattern with its rows of one entry; no head axis; nine rows of
    521 entries and a row over three chunks; unsorted and repeated entries, which only the permutation gives their own e row; for the
    edge op an e of zeros and the tables on the grid of 2^-10, where some t are exactly 0."""
    c = case.cases()[name]
    got, want = _both(c)
    assert torch.equal(got, want), (name, float((got - want).abs().max()))
    assert float(got.abs().max()) > 0.0


@pytest.mark.parametrize("name", case.case_names("edge-zero-"))
def test_e_of_zeros_against_the_op_without_it(name):
    c = case.cases()[name]
    plain = case.cases()["plain-" + name[len("edge-zero-"):]]
    assert float(c.e16.float().abs().max()) == 0.0 and plain.inner is c.inner.inner and plain.e16 is None
    pattern = _pattern(c)
    assert torch.equal(_attend(pattern, c, *_inputs(c)), _attend(pattern, plain, *_inputs(plain))), name


@pytest.mark.parametrize("name", ["plain-lanes-hub-8x16-indices-shared", "plain-lanes-hub-12x64-graph-shared", "edge-lanes-hub-3x8-indices-shared",
                                  "edge-long-three_chunk_hub-8x16-indices-shared"])
def test_shared_against_a_separate_copy_of_x_src(name):
    """v16=None aggregates the widened x_src16 row of the one gather per entry: the bits of the kernels with a v table of their own
    fed a copy of x_src16."""
    c = case.cases()[name]
    assert c.shared
    pattern = _pattern(c)
    x_dst, x_src16, a, _, e16 = _inputs(c)
    assert torch.equal(_attend(pattern, c, x_dst, x_src16, a, None, e16), _attend(pattern, c, x_dst, x_src16, a, x_src16.clone(), e16))


def test_a_row_strided_e16_is_read_in_place(monkeypatch):
    """e16 as a column slice of a wider bfloat16 tensor goes to the launcher by its leading dimension: the same bits, no copy."""
    import pygat_amd as pg
    mod = importlib.import_module("pygat_amd.gatv2_attention")
    for name in ("edge-strided-rect-4x16-shared", "edge-strided-hub-3x8-graph-separate"):
        c = case.cases()[name]
        pattern = _pattern(c)
        x_dst, x_src16, a, v16, e16 = _inputs(c)
        HF, E = c.H * c.F, c.row.numel()
        wide = torch.zeros(E, HF + 12, dtype=torch.bfloat16, device=DEV)
        wide[:, 4:4 + HF] = e16.reshape(E, HF)
        strided = wide[:, 4:4 + HF].view(E, c.H, c.F)
        assert not strided.is_contiguous() and strided.data_ptr() % 8 == 0 and strided.data_ptr() % 16 == 8
        rows, lde = mod._edge_rows(strided, HF)
        assert rows.data_ptr() == strided.data_ptr() and lde == HF + 12, "read in place"
        assert torch.equal(_attend(pattern, c, x_dst, x_src16, a, v16, strided), _attend(pattern, c, x_dst, x_src16, a, v16, e16)), name
        odd = torch.zeros(E, HF + 2, dtype=torch.bfloat16, device=DEV)[:, 2:].view(E, c.H, c.F)       # 4 bytes off: a contiguous copy
        assert mod._edge_rows(odd, HF)[1] == HF
    assert pg.gatv2_attention_edge_bf16 is mod.gatv2_attention_edge_bf16


# ------------------------------------------------------------------------------------------------------------ parity with fp64
PRICED = ([f"{prefix}-lanes-hub-{H}x{F}-{tail}" for prefix, tail in (("plain", "indices-shared"), ("edge", "graph-separate"))
           for H, F in case.LANE_SHAPES]
          + ["plain-lanes-hub-8x64-graph-separate", "edge-lanes-hub-8x64-indices-separate", "edge-lanes-hub-8x64-graph-shared",
             "plain-lanes-hub-noaxis-indices-shared", "edge-lanes-asym-noaxis-graph-separate", "plain-lanes-asym-12x64-graph-separate",
             "edge-lanes-asym-12x64-indices-shared"]
          + case.case_names("plain-long-") + case.case_names("edge-long-")
          + ["plain-rect-3x8-separate", "edge-rect-4x16-shared", "edge-repeats-8x16-separate", "edge-grid-hub-8x16-indices-separate",
             "edge-zero-lanes-hub-4x256-indices-shared"])


@pytest.mark.parametrize("name", PRICED)
def test_against_fp64_on_the_widened_tables(name):
    """One case per lane shape and op, the long rows and the kinds of e against the fp64 ground truth on the widened tables: out by
    parity.close_fwd with the fp32 ground-truth run's own error, the rule of every forward here."""
    c = case.cases()[name]
    c.price(_attend(_pattern(c), c, *_inputs(c)))


# ------------------------------------------------------------------------------------- the bf16 kernels ran, nothing was widened
def test_only_the_bf16_launcher_runs(monkeypatch):
    seen = _spied(monkeypatch)
    for name in ("plain-lanes-asym-8x16-indices-shared", "plain-rect-3x8-separate", "edge-rect-4x16-shared",
                 "edge-long-nine_hubs-8x16-graph-separate"):
        c = case.cases()[name]
        pattern = _pattern(c)
        tensors = _inputs(c)
        del seen[:]
        _attend(pattern, c, *tensors)
        assert seen == [HEFWD if c.edge else HFWD], (name, seen)
        assert c.kind == "graph" or not pattern.has_transpose, "(a graph's pattern shares the graph's transpose from the start)"
        del seen[:]
        _attend(pattern, c, *_widened(tensors))
        assert seen == [EFWD if c.edge else FWD], "float32 tables: the entry point of the op as it was"


@pytest.mark.parametrize("name", ["plain-lanes-hub-12x64-indices-separate", "edge-lanes-hub-12x64-indices-separate"])
def test_no_widened_copy_is_made(name):
    """At 12x64 on the hub pattern the call may allocate its result and the workspace and nothing of a table's size.  The pattern is
    square, so the result [n_rows, 768] fp32 is itself exactly as large as one widened table [n_cols, 768] fp32: the peak of the
    allocator over the call, less the result it returns, must stay below one widened table -- a single fp32 copy of x_src16 or v16,
    however short-lived, would break that; e16 [E, 768], of more rows than a table, all the more."""
    c = case.cases()[name]
    pattern = _pattern(c)
    tensors = _inputs(c)
    _attend(pattern, c, *tensors)                                       # (anything made once per pattern or process is made here)
    x_src16, e16 = tensors[1], tensors[4]
    widened = x_src16.numel() * 4
    assert widened == tensors[3].numel() * 4 and c.shape[0] == c.shape[1] and (e16 is None or e16.numel() * 4 > widened)
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
@pytest.mark.parametrize("name", case.case_names("plain-twice-") + case.case_names("edge-twice-"))
def test_two_runs_are_bit_equal(name):
    c = case.cases()[name]
    pattern = _pattern(c)
    tensors = _inputs(c)
    assert torch.equal(_attend(pattern, c, *tensors), _attend(pattern, c, *tensors))


def test_an_empty_pattern_gives_zeros_without_a_launch(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    empty = pg.EdgePattern.from_indices(torch.zeros(2, 0, dtype=torch.int64, device=DEV), (5, 7))
    x_dst, a = torch.randn(5, 2, 8, device=DEV), torch.randn(2, 8, device=DEV)
    x_src16, v16 = (torch.randn(7, 2, 8, device=DEV).bfloat16() for _ in range(2))
    e16 = torch.zeros(0, 2, 8, device=DEV).bfloat16()
    del seen[:]
    for v in (None, v16):
        with torch.no_grad():
            outs = (pg.gatv2_attention_bf16(empty, x_dst, x_src16, a, v), pg.gatv2_attention_edge_bf16(empty, x_dst, x_src16, a, e16, v))
        for out in outs:
            assert out.shape == (5, 2, 8) and out.dtype == torch.float32 and float(out.abs().max()) == 0.0
    assert seen == []


@pytest.mark.parametrize("name", case.case_names("plain-lonely-") + case.case_names("edge-lonely-")
                         + ["plain-lanes-asym-12x64-indices-shared", "edge-lanes-asym-12x64-graph-separate"])
def test_a_row_of_one_entry_is_its_value_row(name):
    c = case.cases()[name]
    out = _attend(_pattern(c), c, *_inputs(c))
    single = degree(c)[c.row] == 1
    rows, cols = c.row[single].to(DEV), c.col[single].to(DEV)                      # the one entry (i, j) of every such row
    assert rows.numel() >= (12 if "lonely" in name else 1)
    value = (c.x_src16 if c.shared else c.v16).to(DEV)
    assert torch.equal(out[rows], value[cols].float()), "out_i == v16[j].float() (x_src16[j].float() when shared) bit for bit"


# ------------------------------------------------------------------------------------------------------------- sampled blocks
def test_a_sampled_block_with_gathered_bf16_rows():
    """The workload the ops are for: a two-hop sample of a graph, the bf16 table of all nodes gathered by blk.src_nodes and the bf16
    edge features of the whole graph by blk.edge_ids, bit-equal to the float32 ops on the widened gathers."""
    import pygat_amd as pg
    import sample_case
    t = sample_case.TWO_HOP
    g = _graph(*sample_case.graphs()[t["graph"]])
    seed = torch.tensor([t["seed"]], dtype=torch.int64, device=DEV)
    blocks = pg.sample_blocks(g, torch.as_tensor(sample_case.two_hop_seeds()).to(DEV), list(t["fanouts"]), seed=seed)
    gen = torch.Generator(device=DEV).manual_seed(11)
    H, F = 4, 16
    x = torch.randn(g.n, H, F, device=DEV, generator=gen)
    x16 = x.bfloat16()
    e16_full = torch.randn(g.nnz, H, F, device=DEV, generator=gen).bfloat16()
    a = torch.randn(H, F, device=DEV, generator=gen) / F ** 0.5
    for blk in blocks:
        x_dst, x_src16, e16 = x[blk.dst_nodes], x16[blk.src_nodes], e16_full[blk.edge_ids]
        assert x_src16.dtype == e16.dtype == torch.bfloat16 and blk.nnz > 0
        with torch.no_grad():
            got = pg.gatv2_attention_bf16(blk.pattern, x_dst, x_src16, a)
            want = pg.gatv2_attention(blk.pattern, x_dst, x_src16.float(), a)
            got_e = pg.gatv2_attention_edge_bf16(blk.pattern, x_dst, x_src16, a, e16)
            want_e = pg.gatv2_attention_edge(blk.pattern, x_dst, x_src16.float(), a, e16.float())
        assert got.shape == (blk.n_dst, H, F) and torch.equal(got, want) and float(got.abs().max()) > 0.0
        assert torch.equal(got_e, want_e) and not torch.equal(got_e, got)


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    import pygat_amd as pg
    seen = _spied(monkeypatch)
    c = case.cases()["edge-lanes-asym-8x16-indices-shared"]
    pattern = _pattern(c)
    N, E = c.shape[0], c.row.numel()

    def t(*dims, **kw):
        return torch.rand(*dims, device=DEV, **kw)
    x_dst, x_src, a, e = t(N, 4, 16), t(N, 4, 16), t(4, 16), t(E, 4, 16)
    x16, e16 = x_src.bfloat16(), e.bfloat16()
    plain_op = lambda x_dst, x_src16, a, v16=None, e16=None, **kw: pg.gatv2_attention_bf16(pattern, x_dst, x_src16, a, v16, **kw)   # noqa: E731
    edge_op = lambda x_dst, x_src16, a, v16=None, e16=e16, **kw: pg.gatv2_attention_edge_bf16(pattern, x_dst, x_src16, a, e16, v16, **kw)   # noqa: E731
    with torch.no_grad():
        for op, fn in (("gatv2_attention_bf16", plain_op), ("gatv2_attention_edge_bf16", edge_op)):
            for args, kw, needle in (((x_dst, x_src, a), {}, "x_src16 must be torch.bfloat16, not torch.float32"),
                                     ((x_dst, x_src.half(), a), {}, "x_src16 must be torch.bfloat16, not torch.float16"),
                                     ((x_dst.bfloat16(), x16, a), {}, "x_dst must be torch.float32, not torch.bfloat16"),
                                     ((x_dst, x16, a.bfloat16()), {}, "a must be torch.float32, not torch.bfloat16"),
                                     ((x_dst, x16, a, x_src), {}, "v16 must be torch.bfloat16, not torch.float32"),
                                     ((x_dst, x16.cpu(), a), {}, "x_src16 must be a tensor on the GPU"),
                                     ((x_dst, t(N, 4, 32).bfloat16(), a), {}, f"x_src16 ({N}, 4, 32) does not match x_dst"),
                                     ((x_dst, x16, a, t(N, 2, 16).bfloat16()), {}, f"v16 ({N}, 2, 16) does not match x_dst"),
                                     ((x_dst, t(N + 2, 4, 16).bfloat16(), a), {}, f"x_src16 has {N + 2} rows"),
                                     ((x_dst, x16, t(4, 8)), {}, "a (4, 8) does not match x_dst"),
                                     ((t(N, 4, 12), t(N, 4, 12).bfloat16(), t(4, 12)), dict(e16=t(E, 4, 12).bfloat16()), "F = 12"),
                                     ((t(N, 8, 256), t(N, 8, 256).bfloat16(), t(8, 256)), dict(e16=t(2, 8, 256).bfloat16()),
                                      "H * F = 8 * 256 = 2048"),
                                     ((x_dst, x16, a), dict(negative_slope=float("inf")), "negative_slope = inf")):
                with pytest.raises(ValueError, match=op + ":") as err:
                    fn(*args, **kw)
                assert needle in str(err.value), (op, needle, str(err.value))
        for bad, needle in ((e, "e16 must be torch.bfloat16, not torch.float32"), (e16.cpu(), "e16 must be a tensor on the GPU"),
                            (e16[:-1], f"e16 [{E}, 4, 16] expected"), (t(E, 4, 8).bfloat16(), f"e16 [{E}, 4, 16] expected"),
                            (None, "e16 must be a tensor on the GPU")):
            with pytest.raises(ValueError, match="gatv2_attention_edge_bf16:") as err:
                edge_op(x_dst, x16, a, None, bad)
            assert needle in str(err.value), (needle, str(err.value))
        # the float32 ops keep their refusals of bfloat16 tensors
        with pytest.raises(ValueError, match="gatv2_attention: x_src must be float32, not torch.bfloat16"):
            pg.gatv2_attention(pattern, x_dst, x16, a)
        with pytest.raises(ValueError, match="gatv2_attention_edge: x_dst, x_src, a, v and e must be float32"):
            pg.gatv2_attention_edge(pattern, x_dst, x16, a, e16)
    assert seen == []
    # inference only: a tensor that requires grad under grad mode is refused; the same call under no_grad runs
    for op, fn, launcher in (("gatv2_attention_bf16", plain_op, HFWD), ("gatv2_attention_edge_bf16", edge_op, HEFWD)):
        for which in range(5 if launcher == HEFWD else 4):              # (the plain op takes no e16)
            args = [x.clone().requires_grad_(i == which) for i, x in enumerate((x_dst, x16, a, x16, e16))]
            with pytest.raises(ValueError, match=f"{op}: bfloat16 tables are for inference") as err:
                fn(*args)
            assert "torch.no_grad()" in str(err.value) and f"use {op[:-5]} on float32 tables" in str(err.value)
            assert seen == []
            with torch.no_grad():
                out = fn(*args)
            assert seen == [launcher] and not out.requires_grad and out.grad_fn is None
            del seen[:]
        out = fn(x_dst, x16, a)                                         # grad mode on, nothing requires grad: it runs
        assert seen == [launcher] and not out.requires_grad and not pattern.has_transpose
        del seen[:]


# -------------------------------------------------------------------------------------------------------------------- footprint
def test_bf16_kernels_have_no_scratch():
    assert len(K21H) == 80
    no_scratch(K21H, (b"k21h_bwd_row_l8v1", b"k21hs_bwd_long_l8v1", b"k21h_col_row_l8v1", b"k21he_col_long_l8v1", b"k21hes_bwd_row_l8v1",
                      b"k21hd_fwd_row_l8v1", b"k21hds_fwd_row_l8v1", b"k21h_fwd_row_l3v1", b"k21h_fwd_row_l32v2", b"k21hs_fwd_row_l64v5",
                      b"k21h_fwd_row_l8v1x", b"k21h_", b"k21h", b"k21hes_", b"k21hse_fwd_row_l8v1", b"k21hfwd_row_l8v1", b"k21b_fwd_row_l8v1",
                      b"k21hb_fwd_row_l8v1", b"k20h_bwd_row_l8v1", b"k21h_da_stage"))
