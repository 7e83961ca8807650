"""Sparse input features (pygat_amd/features.py, csrc/k9_sparse.hip): the first level's projection and weight gradient on
the non-zeros of a bag-of-words X.  Checked against fp64 products under tests/parity.py's rule, against the dense HIP
kernels under the SAME dropout decisions (the two paths may differ in summation order only), and end to end through the
model on the Cora topology.  The second half runs the case table of tests/sparse_features_case.py: SparseFeatures against
the plain-loop `sparse_ref` bit for bit, and both kernels at every columns-per-lane instantiation, every hq_shift and rows,
columns and segments one short of, at and one past every batch and segment border -- priced by close_grad, and in the
integer flavour required to equal the fp64 result."""
import numpy as np
import pytest
import torch

import sparse_features_case as case
from parity import close_grad

pytestmark = pytest.mark.gpu


def _features(n, fin, density, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, fin, generator=g) < density).float() * (torch.rand(n, fin, generator=g) + 0.1)
    x[3] = 0                                         # an empty row
    x[11] = torch.rand(fin, generator=g) + 0.1       # a full row: several 64-pair batches of the walk
    x[:, 5] = 0                                      # an empty column
    return x / x.sum(1, keepdim=True).clamp(min=1e-6)


@pytest.mark.parametrize("n,fin,H,Fo,skip,p", [(2708, 1433, 8, 8, False, 0.0), (2708, 1433, 8, 8, False, 0.6), (1000, 500, 8, 3, True, 0.5),
                                                (777, 300, 4, 32, True, 0.0), (500, 129, 1, 7, False, 0.3), (300, 50, 3, 121, False, 0.0)])
def test_sparse_projection_and_weight_gradient(n, fin, H, Fo, skip, p):
    import pygat_amd as pg
    from pygat_amd._lib import lib, check
    from pygat_amd.features import SparseFeatures
    dev = "cuda"
    Fp = pg.padded_width(Fo); R = H * Fp
    assert R * (2 if skip else 1) + H <= 512, "more output columns than the sparse kernels take"
    x = _features(n, fin, 0.02, n + fin)
    x[:, 7] = torch.rand(n) + 0.1                    # a column every row has: several segments
    x = x / x.sum(1, keepdim=True).clamp(min=1e-6)
    g = torch.Generator().manual_seed(H + Fo)
    W = torch.randn(H, fin, Fo, generator=g) * 0.3; a = torch.randn(H, 2 * Fo, generator=g) * 0.3
    Ws = torch.randn(H, fin, Fo, generator=g) * 0.3 if skip else None
    keep = 1.0 - p
    M = (torch.rand(H, n, fin, generator=g) < keep) if p > 0 and H <= 8 else None      # explicit decisions
    bits = None
    if M is not None:
        bits = sum((M[h].to(torch.int32) << h) for h in range(H)).to(torch.uint8).to(dev).contiguous()
    xd = x.to(dev); xs = SparseFeatures(xd)
    # (the full row and the full column come on top of the 2 %: a third of one percent at 1433 columns, 2.2 % at 50)
    assert xs.nnz == int((x != 0).sum()) and abs(xs.density - 0.02) < 0.02 + 1.0 / fin + 1.0 / n and xs.nseg > fin
    assert xs.density == xs.nnz / (n * fin)
    ldw = -(-(R * (2 if skip else 1) + 2 * H) // 4) * 4
    Wcat = torch.empty(fin, ldw, device=dev); a_pad = torch.empty(H, 2, Fp, device=dev)
    Wd, ad, Wsd = W.to(dev).contiguous(), a.to(dev).contiguous(), (Ws.to(dev).contiguous() if skip else None)   # (kept alive)
    check(lib.pygat_pack_params(H, fin, Fo, Wd.data_ptr(), ad.data_ptr(), Wsd.data_ptr() if skip else None, Wcat.data_ptr(), ldw,
                                a_pad.data_ptr(), None))
    Wh = torch.full((n, R), float("nan"), device=dev); Sk = torch.full((n, R), float("nan"), device=dev) if skip else None
    s = torch.full((n, H), float("nan"), device=dev) if p == 0 else None
    pe = p if M is not None else 0.0
    check(lib.pygat_project_sparse(n, fin, H, Fo, xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(), Wcat.data_ptr(), ldw,
                                   pe, None, 0, bits.data_ptr() if bits is not None else None, Wh.data_ptr(),
                                   Sk.data_ptr() if skip else None, s.data_ptr() if s is not None else None, None), "project_sparse")
    torch.cuda.synchronize()
    scale = 1.0 / keep if M is not None else 1.0
    for h in range(H):
        xm = (x * M[h] if M is not None else x) * scale
        close_grad(Wh.view(n, H, Fp)[:, h, :Fo], (xm.double() @ W[h].double()).numpy(), (xm @ W[h]).double().numpy(), f"Wh head {h}")
        assert Fp == Fo or float(Wh.view(n, H, Fp)[:, h, Fo:].abs().max()) == 0.0
        if skip:
            close_grad(Sk.view(n, H, Fp)[:, h, :Fo], (xm.double() @ Ws[h].double()).numpy(), (xm @ Ws[h]).double().numpy(), f"Sk head {h}")
        if s is not None:
            ref = x.double() @ (W[h].double() @ a[h, :Fo].double())
            close_grad(s[:, h], ref.numpy(), (x @ (W[h] @ a[h, :Fo])).double().numpy(), f"s head {h}")
    # weight gradient
    dWh = torch.zeros(n, H, Fp); dWh[:, :, :Fo] = torch.randn(n, H, Fo, generator=g)
    RW = R + 4 * H
    GR = torch.randn(n, RW, generator=g)
    dW = torch.full((H, fin, Fo), float("nan"), device=dev); dWs = torch.full((H, fin, Fo), float("nan"), device=dev) if skip else None
    dWh_d, GR_d = dWh.view(n, R).to(dev).contiguous(), GR.to(dev).contiguous()
    wss = torch.empty(lib.pygat_wgrad_sparse_workspace_bytes(xs.nseg, H, Fo, int(skip)) // 4 + 4, device=dev)
    check(lib.pygat_wgrad_sparse(n, fin, H, Fo, xs.nseg, xs.colseg.data_ptr(), xs.seg_col.data_ptr(), xs.seg_begin.data_ptr(),
                                 xs.seg_end.data_ptr(), xs.trow.data_ptr(), xs.tval.data_ptr(), pe, None, 0,
                                 bits.data_ptr() if bits is not None else None, dWh_d.data_ptr(),
                                 GR_d.data_ptr() if skip else None, RW, wss.data_ptr(), dW.data_ptr(),
                                 dWs.data_ptr() if skip else None, None), "wgrad_sparse")
    torch.cuda.synchronize()
    for h in range(H):
        xm = (x * M[h] if M is not None else x) * scale
        d = dWh[:, h, :Fo]
        close_grad(dW[h], (xm.double().t() @ d.double()).numpy(), (xm.t() @ d).double().numpy(), f"dW head {h}")
        if skip:
            gph = GR[:, h * Fp:h * Fp + Fo]
            close_grad(dWs[h], (xm.double().t() @ gph.double()).numpy(), (xm.t() @ gph).double().numpy(), f"dWskip head {h}")


@pytest.mark.parametrize("dropout", [0.0, 0.6])
def test_model_on_sparse_features_equals_the_dense_path(topologies, monkeypatch, dropout):
    """The Cora-shaped model, training step and eval forward, with the first level on the sparse kernels and on the dense
    ones: same in-kernel dropout decisions (same seed), so loss, logits and every gradient agree to rounding."""
    import pygat_amd as pg
    from pygat_amd import features
    rowptr, col = topologies["cora"]
    N = len(rowptr) - 1
    x = _features(N, 1433, 0.013, 1).cuda()
    y = torch.randint(0, 7, (N,), generator=torch.Generator().manual_seed(2)).cuda()
    it = torch.arange(140).cuda()
    graph = pg.CSRGraph(torch.as_tensor(rowptr).cuda(), torch.as_tensor(col).cuda())
    crit = pg.EluLogSoftmaxNLL(it, y, N)
    res = []
    for sparse in (True, False):
        monkeypatch.setattr(features, "ENABLED", sparse)
        features._cache.clear()
        torch.manual_seed(11)
        model = pg.GAT([1433, 8, 7], [8, 1], 2, dropout, 0.2, pg.SpGraphAttentionLayer).cuda().train()
        torch.manual_seed(12)                          # the levels draw their mask seeds from torch's generator
        loss = crit(model(x, graph))
        loss.backward()
        with torch.no_grad():
            logits = model.eval()(x, graph)
        res.append((float(loss), [p.grad.clone() for p in model.parameters()], logits))
        assert (features.as_sparse_features(x, 72) is not None) == sparse
    assert abs(res[0][0] - res[1][0]) <= 2e-6 * max(1.0, abs(res[1][0]))
    for gs, gd in zip(res[0][1], res[1][1]):
        assert float((gs - gd).abs().max()) <= 2e-6 * max(1.0, float(gd.abs().max()))
    assert float((res[0][2] - res[1][2]).abs().max()) <= 2e-6


# ---------------------------------------------------------------------------------------------------
# the case table of tests/sparse_features_case.py
# ---------------------------------------------------------------------------------------------------
DEV = "cuda"
NAN = float("nan")


def _same_structures(xs, ref, what):
    assert xs.nseg == ref["nseg"] and xs.nnz == len(ref["col"]), what
    for name in case.STRUCTURE_ARRAYS:
        got, want = getattr(xs, name), torch.as_tensor(ref[name])
        assert got.dtype == want.dtype and got.is_contiguous(), (what, name)
        assert torch.equal(got.cpu(), want), f"{what}: {name} differs from sparse_ref"


@pytest.mark.parametrize("kind", list(case.KINDS))
@pytest.mark.parametrize("flavour", case.FLAVOURS)
def test_sparse_features_hold_what_the_plain_loops_give(kind, flavour):
    from pygat_amd.features import SEGMENT, MAX_COLUMNS, SparseFeatures
    assert (SEGMENT, MAX_COLUMNS) == (case.SEGMENT, case.MAX_COLUMNS)
    x = case.matrix(kind, flavour)
    _same_structures(SparseFeatures(x.to(DEV)), case.sparse_ref(x), f"{kind} {flavour}")


@pytest.mark.parametrize("n,fin", [(1, 300), (300, 1), (1, 1), (129, 2)])
def test_sparse_features_of_a_single_row_and_a_single_column(n, fin):
    """One row (every column of at most one entry), one column (three segments, the last one short) and both at once."""
    from pygat_amd.features import SparseFeatures
    g = torch.Generator().manual_seed(n + fin)
    x = (torch.rand(n, fin, generator=g) < 0.9).float() * (torch.rand(n, fin, generator=g) + 0.1)
    x[0, 0] = 0.5
    _same_structures(SparseFeatures(x.to(DEV)), case.sparse_ref(x), f"{n} x {fin}")


_xs = {}


def _features_of(c):
    """The SparseFeatures of a case's matrix, built once per (kind, flavour) and left unchanged."""
    from pygat_amd.features import SparseFeatures
    key = (c.kind, c.flavour)
    if key not in _xs:
        _xs[key] = SparseFeatures(case.matrix(*key).to(DEV))
    return _xs[key]


def _run(c, xs, d, Wcat, ldw, seed_ptr, bits_ptr):
    """Both kernels of case `c` through the C ABI, every output and the workspace pre-filled with NaN.  -> {name: tensor}."""
    from pygat_amd._lib import lib, check
    n, fin, H, Fo, R = case.N, case.FIN, c.H, c.Fo, c.R
    out = {"Wh": torch.full((n, R), NAN, device=DEV), "dW": torch.full((H, fin, Fo), NAN, device=DEV)}
    if c.skip:
        out["Sk"] = torch.full((n, R), NAN, device=DEV); out["dWskip"] = torch.full((H, fin, Fo), NAN, device=DEV)
    if c.with_s:
        out["s"] = torch.full((n, H), NAN, device=DEV)
    ptr = lambda name: out[name].data_ptr() if name in out else None  # noqa: E731
    check(lib.pygat_project_sparse(n, fin, H, Fo, xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(), Wcat.data_ptr(), ldw,
                                   c.p, seed_ptr, case.STREAM, bits_ptr, ptr("Wh"), ptr("Sk"), ptr("s"), None), "project_sparse")
    words = lib.pygat_wgrad_sparse_workspace_bytes(xs.nseg, H, Fo, int(c.skip)) // 4
    assert words == xs.nseg * c.ncols_bwd
    ws = torch.full((words + 4,), NAN, device=DEV)
    check(lib.pygat_wgrad_sparse(n, fin, H, Fo, xs.nseg, xs.colseg.data_ptr(), xs.seg_col.data_ptr(), xs.seg_begin.data_ptr(),
                                 xs.seg_end.data_ptr(), xs.trow.data_ptr(), xs.tval.data_ptr(), c.p, seed_ptr, case.STREAM, bits_ptr,
                                 d["dWh"].data_ptr(), d["Gp"].data_ptr() if c.skip else None, d["ldg"], ws.data_ptr(), ptr("dW"),
                                 ptr("dWskip"), None), "wgrad_sparse")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[words:]).all()), f"{c.name}: the weight gradient wrote behind its workspace"
    return out


@pytest.mark.parametrize("name", case.case_names())
def test_sparse_kernels_on_the_case_table(name):
    """Wh, Sk, s, dW and dWskip of one case against the fp64 products under the case's masks (close_grad per head; the exact
    flavour bit for bit), padded columns exactly zero, ldw and ldg wider than the columns with NaN behind them, a second run
    equal to the first, and a seeded run of up to 8 heads equal to the same call on philox_ref.head_bits."""
    from pygat_amd._lib import lib, check
    c = case.cases()[name]
    H, Fo, R, fin = c.H, c.Fo, c.R, case.FIN
    inp = c.inputs()
    xs = _features_of(c)
    d = {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    assert d["ldg"] > R and c.ncols_fwd <= case.MAX_COLUMNS
    d["Gp"][:, R:] = NAN                                              # nothing behind the R columns of a Gp row is read
    ldw = -(-(c.ncols_bwd + 2 * H) // 4) * 4 + 4
    Wcat = torch.full((fin, ldw), NAN, device=DEV); a_pad = torch.empty(H, 2, c.Fp, device=DEV)
    check(lib.pygat_pack_params(H, fin, Fo, d["W"].data_ptr(), d["a"].data_ptr(), d["Ws"].data_ptr() if c.skip else None,
                                Wcat.data_ptr(), ldw, a_pad.data_ptr(), None))
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Wcat[:, :c.ncols_fwd]).any())
    Wcat[:, c.ncols_fwd:] = NAN                                       # nothing behind the columns in use is read
    seed = torch.tensor([case.SEED], dtype=torch.int64, device=DEV)
    bits = c.bits()
    bits_d = torch.as_tensor(bits).to(DEV).contiguous() if bits is not None else None
    seed_ptr = seed.data_ptr() if c.mask == "seed" else None
    bits_ptr = bits_d.data_ptr() if c.mask == "bytes" else None
    first = _run(c, xs, d, Wcat, ldw, seed_ptr, bits_ptr)
    worst = c.price(first)
    print(name, f"cpl {c.cpl_fwd}/{c.cpl_bwd} hq_shift {c.hq_shift}", {k: f"{e:.2e}" for k, e in worst.items()})
    again = _run(c, xs, d, Wcat, ldw, seed_ptr, bits_ptr)
    for k in first:
        assert torch.equal(first[k], again[k]), f"{name} {k}: two runs differ"
    if c.mask == "seed" and H <= 8:
        assert np.array_equal(bits, case.seeded_bits(H, c.p))
        given = _run(c, xs, d, Wcat, ldw, None, bits_d.data_ptr())
        for k in first:
            assert torch.equal(first[k], given[k]), f"{name} {k}: a seed and philox_ref's bytes for it give different bits"
