"""Graph intake (csrc/k0_graph.hip) and the slot structures of pygat_amd/graph.py against the plain NumPy reference of
tests/graph_ref.py, bit for bit: the CSR of a dense adjacency in every dtype and layout, the exclusive scan, the edge pairs,
the mirror permutation and the transpose, from_edge_index / block_diag / as_graph, the row-snapped slot borders, the slot
records, the cut-row list with its `wide` split, the row chunks of the pipelined level, the degree order and the
self-loop-only tail.  All integer work: no tolerance anywhere.  tests/test_graph_ref.py shows on the CPU that the graphs have
what these comparisons need (wide chains, both branches of the snapping rule, a tail)."""
import numpy as np
import pytest
import torch

import graph_ref as R
from graph_cases import SLOT_EDGES, from_bool, graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def pg():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import pygat_amd
    return pygat_amd


_graphs = {}


def csr_graph(pg, name):
    """The CSRGraph of graph_cases.graph(name), built once."""
    if name not in _graphs:
        rowptr, col = graph(name)
        _graphs[name] = pg.CSRGraph(torch.tensor(rowptr, device=DEV), torch.tensor(col, device=DEV), slot_edges=4)
    return _graphs[name]


def host(t):
    return t.detach().cpu().numpy().astype(np.int64)


def same(got, want, what, fields=None):
    """Bit-exact comparison that names the first entry that differs: "slot 17: flags 1, expected 3"."""
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.int64)
    want = np.asarray(want, dtype=np.int64)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    bad = np.argwhere(got != want)
    if len(bad):
        idx = tuple(int(v) for v in bad[0])
        field = f" {fields[idx[1]]}" if fields and len(idx) > 1 else ""
        raise AssertionError(f"{what} {idx[0]}:{field} {got[idx]}, expected {want[idx]}  ({len(bad)} entries differ)")


def arange_like(t):
    return np.arange(t.numel())


# =================================================================== dense intake
NAN, INF = float("nan"), float("inf")
SPECIALS = np.array([1.0, -1.0, -0.0, NAN, INF, -INF, 1e-40, -1e-40], dtype=np.float32)     # 1e-40: an fp32 subnormal
NONZERO = SPECIALS[[0, 1, 3, 4, 5, 6, 7]]
DENSE_SIZES = [1, 3, 63, 64, 65, 127, 129, 301]


def dense_case(N):
    """fp32 [N, N]: a fifth of the entries drawn from SPECIALS, +0.0 elsewhere; row 0 full, row 1 empty (one -0.0), row 2 a
    single subnormal in column N - 1, row 3 only inside the last partial 64-column sweep."""
    rng = np.random.default_rng(100 + N)
    a = np.zeros((N, N), dtype=np.float32)
    mask = rng.random((N, N)) < 0.2
    a[mask] = SPECIALS[rng.integers(0, len(SPECIALS), (N, N))][mask]
    a[0, :] = NONZERO[np.arange(N) % len(NONZERO)]
    if N >= 2:
        a[1, :] = 0.0
        a[1, 0] = -0.0
    if N >= 3:
        a[2, :] = 0.0
        a[2, N - 1] = 1e-40
    if N >= 4:
        c0 = 64 * ((N - 1) // 64)
        a[3, :] = 0.0
        a[3, c0:] = NONZERO[np.arange(N - c0) % len(NONZERO)]
    return a


def strided(a, margin=7.0):
    """a as the [:N, :N] view of an (N + 3) x (N + 5) device buffer whose margin is non-zero (and positive)."""
    N = a.shape[0]
    big = torch.full((N + 3, N + 5), margin, dtype=a.dtype, device=DEV)
    big[:N, :N] = a.to(DEV)
    return big[:N, :N]


def abi_pattern(view, mode):
    """pygat_dense_row_counts -> scan -> pygat_dense_fill_cols, as from_dense calls them: (counts, rowptr, col + 8 guards)."""
    from pygat_amd._lib import lib, check
    n, ld, m = view.shape[0], view.stride(0), (1 if mode == "positive" else 0)
    s = torch.cuda.current_stream().cuda_stream
    counts = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    check(lib.pygat_dense_row_counts(view.data_ptr(), n, ld, m, counts.data_ptr(), s), "row_counts")
    rowptr = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(lib.pygat_scan_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    check(lib.pygat_exclusive_scan_i32(counts.data_ptr(), n, rowptr.data_ptr(), ws.data_ptr(), s), "scan")
    nnz = int(rowptr[-1].item())
    assert 0 < nnz <= n * n
    col = torch.full((nnz + 8,), -7, dtype=torch.int32, device=DEV)
    check(lib.pygat_dense_fill_cols(view.data_ptr(), n, ld, m, rowptr.data_ptr(), col.data_ptr(), s), "fill_cols")
    return counts, rowptr, col


@pytest.mark.parametrize("N", DENSE_SIZES)
def test_dense_intake_abi(pg, N):
    """The three intake calls on a strided view with empty rows: counts, rowptr and col equal the reference in both modes, and
    no column is written past nnz."""
    a = dense_case(N)
    t = torch.from_numpy(a)
    view = strided(t)
    assert view.stride(0) == N + 5 and view.stride(1) == 1
    for mode in ("nonzero", "positive"):
        rp, col = R.dense_pattern(a, mode)
        mask = (t > 0) if mode == "positive" else (t != 0)                 # torch on the CPU says the same
        same(from_bool(mask.numpy())[1], col, f"N={N} {mode}: torch CPU col")
        counts, rowptr, colg = abi_pattern(view, mode)
        same(counts, np.diff(rp), f"N={N} {mode}: count of row")
        same(rowptr, rp, f"N={N} {mode}: rowptr")
        same(colg[:len(col)], col, f"N={N} {mode}: col")
        same(colg[len(col):], np.full(8, -7), f"N={N} {mode}: guard behind col")
    if N >= 2:
        assert (np.diff(R.dense_pattern(a, "nonzero")[0]) == 0).any()      # the empty row reached the kernels
    nz, pos = R.dense_pattern(a, "nonzero")[1], R.dense_pattern(a, "positive")[1]
    assert N == 1 or len(pos) < len(nz)


@pytest.mark.parametrize("layout", ["strided", "contiguous"])
@pytest.mark.parametrize("N", DENSE_SIZES)
def test_from_dense_fp32(pg, N, layout):
    """CSRGraph.from_dense on the same matrices with a positive diagonal (no empty row in either mode)."""
    a = dense_case(N)
    np.fill_diagonal(a, 1.0)
    t = torch.from_numpy(a)
    adj = strided(t) if layout == "strided" else t.to(DEV)
    for mode in ("nonzero", "positive"):
        rp, col = R.dense_pattern(a, mode)
        g = pg.CSRGraph.from_dense(adj, mode)
        assert (g.n, g.nnz) == (N, len(col))
        same(g.fwd.rowptr, rp, f"N={N} {layout} {mode}: rowptr")
        same(g.fwd.col, col, f"N={N} {layout} {mode}: col")
        same(g.fwd.edge_rc, R.edge_pairs(rp, col), f"N={N} {layout} {mode}: edge", ("row", "col"))


def _dtype_case(kind):
    """[65, 65] CPU tensor of another dtype or layout, asymmetric, positive diagonal."""
    N = 65
    rng = np.random.default_rng(7)
    mask = torch.from_numpy(rng.random((N, N)) < 0.15)
    pick = torch.from_numpy(rng.integers(0, 8, (N, N)))
    if kind == "bool":
        adj = mask.clone()
    elif kind == "int64":
        adj = torch.tensor([1, -1, 0, 2 ** 40, -2 ** 40, 3, -(2 ** 62), 2 ** 62], dtype=torch.int64)[pick] * mask
    else:
        dtype = {"float64": torch.float64, "float16": torch.float16, "bfloat16": torch.bfloat16, "transposed": torch.float32}[kind]
        tiny = {"float64": 1e-60, "float16": 1e-7, "bfloat16": 1e-40, "transposed": 1e-40}[kind]     # float64: 0 in fp32; the
        vals = torch.tensor([1.0, -1.0, -0.0, NAN, INF, -INF, tiny, -tiny], dtype=torch.float64).to(dtype)   # others: subnormals
        assert (vals[6] != 0) and (vals[7] != 0) and (kind != "float64" or vals[6].float() == 0)
        adj = torch.where(mask, vals[pick], torch.zeros((), dtype=dtype))
    adj.fill_diagonal_(True if kind == "bool" else 1)
    return adj


@pytest.mark.parametrize("kind", ["float64", "float16", "bfloat16", "bool", "int64", "transposed"])
def test_from_dense_other_dtypes_and_layouts(pg, kind):
    """The pattern is `adj != 0` / `adj > 0` in the tensor's OWN dtype, as torch evaluates it on the CPU."""
    adj = _dtype_case(kind)
    dev = adj.to(DEV)
    if kind == "transposed":
        adj, dev = adj.t(), dev.t()
        assert dev.stride(1) != 1
    for mode in ("nonzero", "positive"):
        mask = ((adj > 0) if mode == "positive" else (adj != 0)).numpy()
        rp, col = from_bool(mask)
        assert not np.array_equal(mask, mask.T) and (np.diff(rp) > 0).all()
        if kind not in ("bfloat16", "bool"):      # NumPy has no bfloat16; the others straight through the reference as well
            rp2, col2 = R.dense_pattern(adj.contiguous().numpy(), mode)
            assert np.array_equal(rp2, rp) and np.array_equal(col2, col)
        g = pg.CSRGraph.from_dense(dev, mode)
        same(g.fwd.rowptr, rp, f"{kind} {mode}: rowptr")
        same(g.fwd.col, col, f"{kind} {mode}: col")
        assert not g.symmetric


# =================================================================== exclusive scan
T = 4096          # items per scan tile; a chunk of tile sums holds 256
SCAN_SIZES = [1, 15, 16, 17, T - 1, T, T + 1, 256 * T, 256 * T + 1, 513 * T + 5]


@pytest.mark.parametrize("n", SCAN_SIZES)
def test_exclusive_scan(pg, n):
    from pygat_amd._lib import lib, check
    gen = torch.Generator().manual_seed(n)
    inputs = {"random": torch.randint(0, 7, (n,), dtype=torch.int32, generator=gen), "zeros": torch.zeros(n, dtype=torch.int32),
              "ones": torch.ones(n, dtype=torch.int32)}
    for what, v in inputs.items():
        ref = np.concatenate([[0], np.cumsum(v.numpy().astype(np.int64))])
        assert ref[-1] < 2 ** 31
        vd = v.to(DEV)
        out = torch.full((n + 1,), -7, dtype=torch.int32, device=DEV)
        ws = torch.empty(lib.pygat_scan_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        check(lib.pygat_exclusive_scan_i32(vd.data_ptr(), n, out.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream),
              "scan")
        same(out, ref, f"scan of {n} {what}: out")


# =================================================================== pairs, mirror permutation, transpose
@pytest.mark.parametrize("name", ["hub", "ladder"])
def test_pairs_and_mirror_perm(pg, name):
    rowptr, col = graph(name)
    g = csr_graph(pg, name)
    perm, asym, empty = R.mirror_perm(rowptr, col)
    assert g.symmetric and not asym and not empty
    same(g.fwd.edge_rc, R.edge_pairs(rowptr, col), f"{name}: edge", ("row", "col"))
    same(g.perm_t, perm, f"{name}: perm_t")
    assert g.perm_f is g.perm_t and g.bwd is g.fwd
    same(g.perm_t[g.perm_t.long()], arange_like(g.perm_t), f"{name}: perm_t[perm_t]")


@pytest.mark.parametrize("name", ["hub_minus_edge", "asym65"])
def test_transpose(pg, name):
    rowptr, col = graph(name)
    g = csr_graph(pg, name)
    rp_t, col_t, perm_t, perm_f = R.transpose(rowptr, col)
    assert not g.symmetric and g.bwd is not g.fwd
    same(g.fwd.edge_rc, R.edge_pairs(rowptr, col), f"{name}: edge", ("row", "col"))
    same(g.bwd.rowptr, rp_t, f"{name}: transposed rowptr")
    same(g.bwd.col, col_t, f"{name}: transposed col")
    same(g.bwd.edge_rc, R.edge_pairs(rp_t, col_t), f"{name}: transposed edge", ("row", "col"))
    same(g.perm_t, perm_t, f"{name}: perm_t")
    same(g.perm_f, perm_f, f"{name}: perm_f")
    same(g.perm_f[g.perm_t.long()], arange_like(g.perm_t), f"{name}: perm_f[perm_t]")


# =================================================================== from_edge_index, block_diag, as_graph
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("symmetrize", [False, True])
def test_from_edge_index(pg, symmetrize, self_loops):
    """A COO list with duplicates, one orientation only for most edges, no self loop; every node has an out-edge."""
    n = 97
    rng = np.random.default_rng(3)
    r = np.concatenate([np.arange(n), rng.integers(0, n, 300)])
    c = np.concatenate([(np.arange(n) + 1) % n, rng.integers(0, n, 300)])
    keep = r != c
    r, c = r[keep], c[keep]
    r, c = np.concatenate([r, r[:50]]), np.concatenate([c, c[:50]])                 # duplicates
    order = rng.permutation(len(r))
    r, c = r[order], c[order]
    raw = set(zip(r.tolist(), c.tolist()))
    assert len(raw) < len(r) and any((j, i) not in raw for i, j in raw)
    rr, cc = r, c
    if symmetrize:
        rr, cc = np.concatenate([rr, cc]), np.concatenate([cc, rr])
    if self_loops:
        rr, cc = np.concatenate([rr, np.arange(n)]), np.concatenate([cc, np.arange(n)])
    key = np.unique(rr.astype(np.int64) * n + cc)
    rp = np.concatenate([[0], np.cumsum(np.bincount(key // n, minlength=n))])
    g = pg.CSRGraph.from_edge_index(torch.as_tensor(r, device=DEV), torch.as_tensor(c, device=DEV), n, symmetrize=symmetrize,
                                    self_loops=self_loops)
    same(g.fwd.rowptr, rp, "from_edge_index: rowptr")
    same(g.fwd.col, key % n, "from_edge_index: col")
    assert g.symmetric == symmetrize == (not R.mirror_perm(rp, key % n)[1])
    assert bool((g.fwd.edge_rc[:, 0] == g.fwd.edge_rc[:, 1]).any().item()) == self_loops


def test_block_diag(pg):
    names = ["hub", "asym65", "shared_slot"]           # node offsets 1001 and 1066, edge offsets 7387 and 7787
    parts = [graph(k) for k in names]
    rps, cols, noff, eoff = [np.zeros(1, dtype=np.int64)], [], 0, 0
    for rp, col in parts:
        rps.append(rp[1:] + eoff)
        cols.append(col + noff)
        noff, eoff = noff + len(rp) - 1, eoff + len(col)
    rowptr, col = np.concatenate(rps), np.concatenate(cols)
    assert (len(parts[0][0]) - 1) % 2 == 1 and len(parts[0][1]) % 2 == 1
    g = pg.CSRGraph.block_diag([csr_graph(pg, k) for k in names])
    assert (g.n, g.nnz) == (noff, eoff) and not g.symmetric
    same(g.fwd.rowptr, rowptr, "block_diag: rowptr")
    same(g.fwd.col, col, "block_diag: col")
    same(g.fwd.edge_rc, R.edge_pairs(rowptr, col), "block_diag: edge", ("row", "col"))
    rp_t, col_t, perm_t, perm_f = R.transpose(rowptr, col)
    same(g.bwd.rowptr, rp_t, "block_diag: transposed rowptr")
    same(g.bwd.col, col_t, "block_diag: transposed col")
    same(g.perm_t, perm_t, "block_diag: perm_t")
    same(g.perm_f, perm_f, "block_diag: perm_f")


def test_as_graph(pg):
    from pygat_amd.graph import as_graph
    rowptr, col = graph("tail")
    n = len(rowptr) - 1
    rp_d, col_d = torch.tensor(rowptr, device=DEV), torch.tensor(col, device=DEV)
    g_pair = as_graph((rp_d, col_d))
    g_csr = as_graph(torch.sparse_csr_tensor(rp_d, col_d, torch.ones(len(col), device=DEV), size=(n, n)))
    for g in (g_pair, g_csr):
        same(g.fwd.rowptr, rowptr, "as_graph: rowptr")
        same(g.fwd.col, col, "as_graph: col")
    assert as_graph(g_pair) is g_pair
    dense = np.zeros((n, n), dtype=np.float32)
    dense[R.edge_rows(rowptr), col] = 1.0
    adj = torch.from_numpy(dense).to(DEV)
    g1 = as_graph(adj)
    assert as_graph(adj) is g1                                      # the same tensor, unchanged: the cached graph
    same(g1.fwd.rowptr, rowptr, "as_graph(dense): rowptr")
    same(g1.fwd.col, col, "as_graph(dense): col")
    i, j = 10, 500
    assert dense[i, j] == 0 and dense[j, i] == 0
    adj[i, j] = adj[j, i] = 1
    g2 = as_graph(adj)
    assert g2 is not g1 and g2.nnz == g1.nnz + 2 and as_graph(adj) is g2
    dense[i, j] = dense[j, i] = 1.0
    rp2, col2 = R.dense_pattern(dense, "nonzero")
    same(g2.fwd.rowptr, rp2, "as_graph(modified dense): rowptr")
    same(g2.fwd.col, col2, "as_graph(modified dense): col")
    same(g1.fwd.col, col, "as_graph: the earlier graph's col")


# =================================================================== slot borders, records, cut list
META = ("first edge", "end edge", "first row", "flags")
CUT = ("owner slot", "row", "pieces")


def check_cut_list(st, cut, want, what):
    """The struct's list against the brute-force set `want`: content, order (pieces descending, owner ascending inside a
    piece count), n_cut and n_cut_wide."""
    assert cut is not None and st.cut_rows == cut.data_ptr() and st.cut_rows, f"{what}: cut list pointer"
    assert st.n_cut == len(want), f"{what}: n_cut {st.n_cut}, expected {len(want)}"
    wide = sum(1 for t in want if t[2] > 32)
    assert st.n_cut_wide == wide, f"{what}: n_cut_wide {st.n_cut_wide}, expected {wide}"
    if want:
        assert cut.shape == (len(want), 3) and cut.dtype == torch.int32 and cut.is_contiguous()
        got = [tuple(t) for t in host(cut).tolist()]
        assert len(set(got)) == len(got), f"{what}: a cut row is listed twice"
        assert set(got) == set(want), f"{what}: cut rows {sorted(set(got) ^ set(want))[:4]} differ"
        same(cut, R.cut_list_order(want), f"{what}: cut entry", CUT)


@pytest.mark.parametrize("ts", SLOT_EDGES)
@pytest.mark.parametrize("name", ["ladder", "hub", "tail", "cora", "pieces32"])
def test_slot_structures(pg, name, ts):
    rowptr, col = graph(name)
    pat = csr_graph(pg, name).fwd
    pat.ref(ts)
    st, sb, cut, meta, order = pat._alt[(ts, True)]
    nslots = R.n_slots(len(col), ts)
    sb_ref = R.slot_borders(rowptr, ts)
    same(sb, sb_ref, f"{name} ts={ts}: border")
    assert meta.shape == (nslots, 4) and order is None
    same(meta, R.slot_meta(rowptr, ts, sb_ref), f"{name} ts={ts}: slot", META)
    assert (st.n, st.nnz, st.slot_edges, st.slot_first, st.slot_count) == (len(rowptr) - 1, len(col), ts, 0, 0)
    assert (st.rowptr, st.edge_rc, st.slot_begin, st.slot_meta) == (pat.rowptr.data_ptr(), pat.edge_rc.data_ptr(), sb.data_ptr(),
                                                                   meta.data_ptr())
    check_cut_list(st, cut, R.cut_rows(rowptr, sb_ref), f"{name} ts={ts}")
    # uniform slots (K3b): records of the plain k * ts borders, no border table and no cut list
    pat.ref(ts, snapped=False)
    stu, sbu, cutu, metau, _ = pat._alt[(ts, False)]
    assert sbu is None and cutu is None and not stu.slot_begin and not stu.cut_rows and (stu.n_cut, stu.n_cut_wide) == (0, 0)
    same(metau, R.slot_meta(rowptr, ts, None), f"{name} ts={ts} uniform: slot", META)
    assert stu.slot_meta == metau.data_ptr() and stu.slot_edges == ts


def test_wide_split_at_32_pieces(pg):
    """32 pieces are not `wide`, 33 are."""
    pat = csr_graph(pg, "pieces32").fwd
    pat.ref(4)
    st, _, cut, _, _ = pat._alt[(4, True)]
    same(cut, [(32, 1, 33), (0, 0, 32)], "pieces32: cut entry", CUT)
    assert (st.n_cut, st.n_cut_wide) == (2, 1)


@pytest.mark.parametrize("ts", SLOT_EDGES)
def test_empty_cut_list(pg, ts):
    pat = csr_graph(pg, "identity64").fwd
    pat.ref(ts)
    st, sb, cut, meta, _ = pat._alt[(ts, True)]
    check_cut_list(st, cut, set(), f"identity ts={ts}")
    same(sb, R.uniform_borders(64, ts), f"identity ts={ts}: border")
    same(meta, R.slot_meta(graph("identity64")[0], ts, None), f"identity ts={ts}: slot", META)


# =================================================================== row chunks
NCHUNKS = (1, 2, 4, 7, 500)


def check_row_chunks(pat, rowptr, ts, nchunks, nslots, row_end, what):
    """-> (number of chunks, number of chunks without a cut row)."""
    sb = R.slot_borders(rowptr, ts)
    all_slots = len(sb) - 1
    prefix = nslots is not None
    out = pat.row_chunks(nchunks, ts, nslots, row_end) if prefix else pat.row_chunks(nchunks, ts)
    nslots, row_end = (nslots, row_end) if prefix else (all_slots, len(rowptr) - 1)
    structs, keep = pat._alt[("chunks", ts, nchunks, nslots if prefix else None)]
    assert 1 <= len(out) <= nchunks and len(out) == len(structs) == len(keep)
    full = [t for t in R.cut_list_order(R.cut_rows(rowptr, sb)) if t[0] < nslots]
    slot, row, seen, bare = 0, 0, [], 0
    for c, ((ref, r0, r1), (st, _, _), sub) in enumerate(zip(out, structs, keep)):
        w = f"{what} chunk {c} of {nchunks}"
        assert ref._obj is st
        assert st.slot_first == slot and st.slot_count > 0, f"{w}: slots [{st.slot_first}, +{st.slot_count}), expected to begin at {slot}"
        assert r0 == row and r1 > r0, f"{w}: rows [{r0}, {r1}), expected to begin at {row}"
        assert rowptr[r0] == sb[st.slot_first], f"{w}: row {r0} begins at edge {rowptr[r0]}, slot {st.slot_first} at {sb[st.slot_first]}"
        slot, row = slot + st.slot_count, r1
        mine = [t for t in full if st.slot_first <= t[0] < slot]          # full is in list order: so is every sub-list
        for owner, r, pieces in mine:
            assert owner + pieces - 1 < slot, f"{w}: the chain of row {r} leaves the chunk"
            assert r0 <= r < r1
        check_cut_list(st, sub, set(mine), w)
        if mine:
            same(sub, mine, f"{w}: cut entry", CUT)
        bare += not mine
        seen += mine
        assert (st.n, st.nnz, st.slot_edges) == (len(rowptr) - 1, int(rowptr[-1]), ts)
        assert (st.rowptr, st.edge_rc) == (pat.rowptr.data_ptr(), pat.edge_rc.data_ptr())
        assert st.slot_begin == pat._alt[(ts, True)][1].data_ptr() and st.slot_meta == pat._alt[(ts, True)][3].data_ptr()
    assert slot == nslots, f"{what}: the chunks end at slot {slot}, expected {nslots}"
    assert row == row_end, f"{what}: the chunks end at row {row}, expected {row_end}"
    assert len(seen) == len(set(seen)) and set(seen) == set(full), f"{what}: the sub-lists do not partition the cut list"
    return len(out), bare


@pytest.mark.parametrize("ts", [4, 64])
@pytest.mark.parametrize("name", ["ladder", "hub", "cora", "pieces32"])
def test_row_chunks(pg, name, ts):
    rowptr, _ = graph(name)
    pat = csr_graph(pg, name).fwd
    counts = {k: check_row_chunks(pat, rowptr, ts, k, None, None, f"{name} ts={ts}") for k in NCHUNKS}
    assert counts[1][0] == 1 and counts[7][0] > 1
    starts = int(np.isin(R.slot_borders(rowptr, ts)[:-1], rowptr[:-1]).sum())
    assert counts[500][0] <= min(500, starts)
    if ts == 64:
        assert counts[500][1] > 0          # some chunk had no cut row: the empty non-NULL list was checked


@pytest.mark.parametrize("ts", [4, 32])
def test_row_chunks_of_the_prefix(pg, ts):
    """The slots in front of the self-loop-only tail of the degree-ordered tail graph."""
    rowptr, col = graph("tail")
    _, _, rp2, c2 = R.degree_order(rowptr, col)
    row_first, first_slot = R.self_loop_tail(rp2, c2, ts)
    pat = csr_graph(pg, "tail").degree_ordered()[0].fwd
    same(pat.rowptr, rp2, "degree-ordered tail graph: rowptr")
    for k in NCHUNKS:
        check_row_chunks(pat, rp2, ts, k, first_slot, row_first, f"tail prefix ts={ts}")


# =================================================================== degree order and tail
@pytest.mark.parametrize("name", ["tail", "hub", "ladder"])
def test_degree_order(pg, name):
    rowptr, col = graph(name)
    to_user, to_int, rp2, c2 = R.degree_order(rowptr, col)
    g = csr_graph(pg, name)
    g2, urow, tint = g.degree_ordered()
    assert g.degree_ordered()[0] is g2 and g2.degree_sorted and not g.degree_sorted
    same(urow, to_user, f"{name}: to_user")
    same(tint, to_int, f"{name}: to_internal")
    same(tint[urow.long()], np.arange(len(to_user)), f"{name}: to_internal[to_user]")
    assert g2.user_row is urow and g2.fwd.user_row is urow and g2.fwd.struct.user_row == urow.data_ptr()
    same(g2.fwd.rowptr, rp2, f"{name} degree-ordered: rowptr")
    same(g2.fwd.col, c2, f"{name} degree-ordered: col")
    same(g2.fwd.edge_rc, R.edge_pairs(rp2, c2), f"{name} degree-ordered: edge", ("row", "col"))
    same(g2.perm_t, R.mirror_perm(rp2, c2)[0], f"{name} degree-ordered: perm_t")
    assert g2.symmetric


@pytest.mark.parametrize("ts", SLOT_EDGES)
@pytest.mark.parametrize("name", ["tail", "hub", "ladder", "identity64", "shared_slot"])
def test_self_loop_tail(pg, name, ts):
    rowptr, col = graph(name)
    _, _, rp2, c2 = R.degree_order(rowptr, col)
    want = R.self_loop_tail(rp2, c2, ts)
    pat = csr_graph(pg, name).degree_ordered()[0].fwd
    got = pat.self_loop_tail(ts)
    assert (want is None) == (name != "tail")
    if want is None:
        assert got is None, f"{name} ts={ts}: tail {got[:2]}, expected None"
        return
    assert got is not None and got[:2] == want, f"{name} ts={ts}: tail {got and got[:2]}, expected {want}"
    row_first, first_slot, ref = got
    n = len(rp2) - 1
    rp_g, col_g = host(pat.rowptr), host(pat.col)
    st, sb, _, meta, _ = pat._alt[(ts, True)]
    sb, meta = host(sb), host(meta)
    n1 = int((np.diff(rp_g) > 1).sum())
    assert (np.diff(rp_g)[row_first:] == 1).all() and np.array_equal(col_g[rp_g[row_first]:], np.arange(row_first, n))
    assert rp_g[row_first] == sb[first_slot]
    assert (meta[first_slot:, 2] >= n1).all() and (meta[:first_slot, 2] < n1).all()
    pre = ref._obj
    assert (pre.slot_first, pre.slot_count) == (0, first_slot)
    for f, _ in type(pre)._fields_:
        if f not in ("slot_first", "slot_count"):
            assert getattr(pre, f) == getattr(st, f), f
    assert (st.slot_first, st.slot_count) == (0, 0)          # the full pattern's struct is left as it was
