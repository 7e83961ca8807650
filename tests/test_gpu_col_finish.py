"""The column pass's cut-row fix-up and the tail's backward stream in one launch (pygat_gat_backward_col_finish, behind
pygat_gat_backward_col_phase(PYGAT_F_MAIN_ONLY)), and the weight gradient's reduce that writes dW [H, Fin, F'] itself: both must
leave exactly the bits of the launch sequences they replace, and ops must pick them where -- and only where -- they apply."""
import ctypes as C

import numpy as np
import pytest
import torch

from tail_case import _iso_csr

pytestmark = pytest.mark.gpu


def _hub_csr(N, iso, seed):
    """tail_case._iso_csr's layout with one hub of 3000 and one of 1200 neighbours: at 64-edge slots (HUB_SLOT_EDGES, the
    headline graph's; a graph this small would get 8-edge slots by itself and both hubs 150+ pieces) a row cut into more than
    32 pieces, merged by a whole work-group, and one cut into 17..32, merged by one wave in several rounds."""
    from oracle import gat_oracle as O
    n0 = int(N * (1 - iso))
    parts = [O.random_symmetric_csr(n0, 6, seed, hub=(2, 3000)), O.random_symmetric_csr(n0, 2, seed + 7, hub=(5, 1200))]
    rows = np.concatenate([np.repeat(np.arange(n0), np.diff(np.asarray(rp, dtype=np.int64))) for rp, _ in parts] + [np.arange(n0, N)])
    cols = np.concatenate([np.asarray(c, dtype=np.int64) for _, c in parts] + [np.arange(n0, N)])
    key = np.unique(rows * N + cols)
    rows, cols = key // N, key % N
    relabel = np.random.default_rng(seed + 1).permutation(N)
    r2, c2 = relabel[rows], relabel[cols]
    o = np.lexsort((c2, r2))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=N))]).astype(np.int32)
    return rowptr, c2[o].astype(np.int32)


HUB_SLOT_EDGES = 64


def _bits(t):
    return t.contiguous().view(torch.int32)


CASES = [dict(graph="iso", N=20000, iso=0.5, seed=40, H=8, Fo=16, urow=False),
         dict(graph="iso", N=12345, iso=0.55, seed=41, H=8, Fo=16, urow=True),
         dict(graph="iso", N=9001, iso=0.37, seed=42, H=4, Fo=16, urow=False),
         dict(graph="iso", N=9001, iso=0.37, seed=42, H=3, Fo=7, urow=True),
         dict(graph="hub", N=16000, iso=0.5, seed=43, H=8, Fo=16, urow=True),
         dict(graph="hub", N=16000, iso=0.5, seed=43, H=2, Fo=16, urow=False)]


@pytest.mark.parametrize("cfg", CASES, ids=[f"{c['graph']}{c['N']}-{c['H']}x{c['Fo']}" for c in CASES])
def test_finish_is_bitwise_fixup_then_stream(cfg):
    """dWh, ds, dt (and the da records of the main launch) after main + finish against pygat_gat_backward_col +
    pygat_gat_backward_tail on the same tables, every row, bit for bit."""
    import pygat_amd as pg
    from pygat_amd import _lib
    from pygat_amd.graph import slot_edges_for
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    N, H, Fo = cfg["N"], cfg["H"], cfg["Fo"]
    Fp = _lib.padded_width(Fo)
    R = H * Fp
    rowptr, col = (_iso_csr if cfg["graph"] == "iso" else _hub_csr)(N, cfg["iso"], cfg["seed"])
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev),
                        HUB_SLOT_EDGES if cfg["graph"] == "hub" else None)
    g_int = graph.degree_ordered()[0]
    ts = slot_edges_for(R, g_int.slot_edges)
    assert cfg["graph"] != "hub" or ts == HUB_SLOT_EDGES
    t = g_int.fwd.self_loop_tail(ts)
    assert t is not None
    row_first, _, gT = t
    assert N - row_first >= 0.9 * cfg["iso"] * N
    pat = g_int.fwd._base if hasattr(g_int.fwd, "_base") else g_int.fwd
    cut = pat._alt[(ts, True)][2]
    st_full = pat._alt[(ts, True)][0]
    assert st_full.n_cut > 0
    pieces = cut[:st_full.n_cut, 2]
    if cfg["graph"] == "hub":
        print("slot edges", ts, "cut rows", st_full.n_cut, "pieces", sorted(pieces.tolist())[-8:])
        assert int(pieces.max()) > 32 and int(((pieces > 16) & (pieces <= 32)).sum()) >= 1, pieces[:8]
    assert int(cut[:st_full.n_cut, 1].max()) < row_first          # every cut row lies before the tail

    gen = torch.Generator().manual_seed(cfg["seed"] + 100)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev)  # noqa: E731
    Wh, a_pad, ds_in = rnd(N, R) * 0.5, rnd(H, 2, Fp) * 0.4, rnd(N, H) * 0.3
    GR = torch.empty(N, R + 4 * H, device=dev)
    GR[:, :R] = rnd(N, R)
    rec = GR[:, R:].view(N, H, 4)
    rec[:, :, 0] = rnd(N, H) * 0.5                    # s
    rec[:, :, 1] = 3.0 + rnd(N, H).abs()              # m: above every logit of these tables
    rec[:, :, 2] = torch.rand(N, H, generator=gen).to(dev) * 0.9 + 0.1   # 1 / Z
    rec[:, :, 3] = rnd(N, H) * 0.2                    # D
    G, y = rnd(N, H * Fo), rnd(N, H * Fo)
    urow = torch.randperm(N, generator=gen).to(torch.int32).to(dev) if cfg["urow"] else None
    nb_da = lib.pygat_gat_backward_col_da_bytes(gT, H, Fo, H)
    assert (nb_da > 0) == ((H, Fo) == (8, 16))
    assert lib.pygat_gat_backward_col_phases_ok(gT, H, Fo, H) == 1
    part_n = lib.pygat_partials_bytes(g_int.nnz, ts, H, Fp) // 4
    flags, s = _lib.F_ELU, torch.cuda.current_stream().cuda_stream
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731

    def tables():
        nan = float("nan")
        return dict(dWh=torch.full((N, R), nan, device=dev), dt=torch.full((N, H), nan, device=dev), ds=ds_in.clone(),
                    part=torch.full((part_n,), nan, device=dev),
                    da=torch.full((nb_da // 4,), nan, device=dev) if nb_da else None)
    old, new = tables(), tables()
    _lib.check(lib.pygat_gat_backward_col(gT, None, H, Fo, 0.2, p(Wh), p(a_pad), p(GR), None, p(old["ds"]), p(old["dWh"]),
                                          p(old["dt"]), None, p(old["part"]), p(old["da"]), 0, 0, H, s), "col")
    _lib.check(lib.pygat_gat_backward_tail(row_first, N - row_first, H, Fo, flags, p(G), p(y), p(urow), p(old["dWh"]), 0, 0,
                                           p(old["ds"]), p(old["dt"]), s), "tail")
    _lib.check(lib.pygat_gat_backward_col_phase(gT, None, H, Fo, 0.2, p(Wh), p(a_pad), p(GR), None, p(new["ds"]), p(new["dWh"]),
                                                p(new["dt"]), None, p(new["part"]), p(new["da"]), 0, 0, H, _lib.F_MAIN_ONLY, s),
               "col main")
    cut_rows = cut[:st_full.n_cut, 1].long()
    torch.cuda.synchronize()
    assert torch.isnan(new["dWh"][cut_rows]).all() and torch.isnan(new["dWh"][row_first:]).all()   # the main launch left them
    _lib.check(lib.pygat_gat_backward_col_finish(gT, H, Fo, p(a_pad), p(new["ds"]), p(new["dWh"]), p(new["dt"]), p(new["part"]), H,
                                                 row_first, N - row_first, flags, p(G), p(y), p(urow), s), "finish")
    torch.cuda.synchronize()
    for k in ("dWh", "ds", "dt") + (("da",) if nb_da else ()):
        assert torch.equal(_bits(old[k]), _bits(new[k])), k
    assert torch.isfinite(new["dWh"]).all() and torch.isfinite(new["dt"]).all() and torch.isfinite(new["ds"]).all()
    # ... and the fix-up phase alone is the old fix-up
    fix = tables()
    fix["part"].copy_(new["part"])
    _lib.check(lib.pygat_gat_backward_col_phase(gT, None, H, Fo, 0.2, p(Wh), p(a_pad), p(GR), None, p(fix["ds"]), p(fix["dWh"]),
                                                p(fix["dt"]), None, p(fix["part"]), None, 0, 0, H, _lib.F_FIXUP_ONLY, s), "col fix")
    torch.cuda.synchronize()
    assert torch.equal(_bits(fix["dWh"][cut_rows]), _bits(old["dWh"][cut_rows])) and torch.equal(_bits(fix["dt"][cut_rows]), _bits(old["dt"][cut_rows]))


def test_finish_refuses_what_it_cannot_take():
    import pygat_amd as pg
    from pygat_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    rowptr, col = _iso_csr(9001, 0.4, 44)
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
    g_int = graph.degree_ordered()[0]
    row_first, _, gT = g_int.fwd.self_loop_tail(64)
    P = 4096
    assert lib.pygat_gat_backward_col_phases_ok(gT, 8, 16, 4) == 0           # two head windows
    assert lib.pygat_gat_backward_col_phases_ok(None, 8, 16, 8) < 0
    f = lib.pygat_gat_backward_col_finish
    assert f(gT, 8, 16, P, P, P, P, P, 4, row_first, 9001 - row_first, 1, P, P, None, None) == -1
    assert b"phases_ok" in lib.pygat_last_error()
    assert f(gT, 8, 16, P, P, P, P, P, 8, row_first, 9002 - row_first, 1, P, P, None, None) == -1
    assert b"outside" in lib.pygat_last_error()
    assert f(gT, 8, 16, P, None, P, P, P, 8, row_first, 9001 - row_first, 1, P, P, None, None) == -1
    assert b"null" in lib.pygat_last_error()
    ph = lib.pygat_gat_backward_col_phase
    assert ph(gT, None, 8, 16, 0.2, P, P, P, None, P, P, P, None, P, None, 0, 0, 8, 3, None) == -1
    assert b"phase=3" in lib.pygat_last_error()
    assert ph(gT, None, 8, 16, 0.2, P, P, P, None, P, P, P, None, P, None, 0, 0, 4, _lib.F_MAIN_ONLY, None) == -1
    assert b"one head window" in lib.pygat_last_error()


def _call_spy(monkeypatch):
    """The names of the C entry points ops calls, in order."""
    from pygat_amd import ops
    calls = []

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            if not name.startswith("pygat_") or fn.restype is not C.c_int:
                return fn

            def wrapped(*a):
                calls.append(name[len("pygat_"):])
                return fn(*a)
            return wrapped
    monkeypatch.setattr(ops, "lib", Spy(getattr(ops.lib, "_lib", ops.lib)))
    return calls


def _level(N, Fin, H, Fo, seed, skip=False):
    rowptr, col = _iso_csr(N, 0.5, seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Fin, generator=g)
    W = torch.randn(H, Fin, Fo, generator=g) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)
    a = torch.randn(H, 2 * Fo, generator=g) * 0.4
    Ws = torch.randn(H, Fin, Fo, generator=g) * 0.1 if skip else None
    G = torch.randn(N, H * Fo, generator=g)
    return rowptr, col, x, W, a, Ws, G


def test_headline_path_makes_the_merged_launch(monkeypatch):
    """8 heads x 16, no skip projection, the level renumbering itself: main launch + finish instead of column pass + stream, no
    launch between them, and out / dW / da are the old sequence's bits."""
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    rowptr, col, x, W, a, _, G = _level(20000, 128, 8, 16, 45)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)

    def run(min_bytes):
        monkeypatch.setattr(ops, "COL_FINISH_MIN_BYTES", min_bytes)
        calls = _call_spy(monkeypatch)
        graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
        Wd, ad = W.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
        out = pg.GATLevelFn.apply(x.to(dev), Wd, ad, None, graph, 0.2, True)
        n_fwd = len(calls)
        out.backward(G.to(dev))
        torch.cuda.synchronize()
        return out.detach().cpu(), Wd.grad.cpu(), ad.grad.cpu(), calls[n_fwd:]
    o0, dW0, da0, c0 = run(1 << 60)
    o1, dW1, da1, c1 = run(0)
    assert c0 == ["gat_backward_prepare", "gat_backward_col", "gat_backward_tail", "a_grad_fold", "wgrad_blocked"], c0
    assert c1 == ["gat_backward_prepare", "gat_backward_col_phases_ok", "gat_backward_col_phase", "gat_backward_col_finish",
                  "a_grad_fold", "wgrad_blocked"], c1
    assert torch.equal(o1, o0) and torch.equal(dW1, dW0) and torch.equal(da1, da0)
    assert torch.isfinite(dW1).all() and torch.isfinite(da1).all()


@pytest.mark.parametrize("kind", ["skip", "ranged"])
def test_other_levels_keep_the_two_launches(kind, monkeypatch):
    """A skip projection's weight gradient reads every row's Gp (the tail goes through pygat_gat_backward_col_tail) and a ranged
    backward has no tail route: both keep pygat_gat_backward_col with its own fix-up launch, whatever the threshold."""
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    rowptr, col, x, W, a, Ws, G = _level(12000, 64, 8, 16, 46, skip=(kind == "skip"))
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "COL_FINISH_MIN_BYTES", 0)
    calls = _call_spy(monkeypatch)
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
    Wd, ad = W.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    Wsd = Ws.to(dev).requires_grad_(True) if Ws is not None else None
    out = pg.GATLevelFn.apply(x.to(dev), Wd, ad, Wsd, graph, 0.2, True, (2, 4) if kind == "ranged" else None)
    out.backward(G.to(dev))
    torch.cuda.synchronize()
    assert "gat_backward_col" in calls and "gat_backward_col_finish" not in calls and "gat_backward_col_phase" not in calls, calls
    if kind == "skip":
        assert "gat_backward_col_tail" in calls and "gat_backward_tail" not in calls, calls
    else:
        assert "gat_backward_tail" not in calls and "gat_backward_col_tail" not in calls, calls
    assert torch.isfinite(Wd.grad).all() and torch.isfinite(ad.grad).all()


@pytest.mark.parametrize("H,Fo,Fin", [(8, 16, 128), (6, 12, 64), (8, 16, 100)])
def test_wgrad_reduce_writes_dw_bitwise(H, Fo, Fin):
    """pygat_wgrad (plain X^T dWh, split-K on the streamed-K kernel) against the same GEMM reduced into a packed [Fin, R] table
    and unpacked by pygat_unpack_wgrad -- the two launches its reduce replaces."""
    from pygat_amd import _lib, ops
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    N = 20000
    Fp = _lib.padded_width(Fo)
    R = H * Fp
    gen = torch.Generator().manual_seed(47)
    X = torch.randn(N, Fin, generator=gen).to(dev)
    dWh = torch.randn(N, R, generator=gen).to(dev)
    split_k = ops._split_k(Fin, R, N, streamed_k=True, mode="split-bf16")
    assert split_k > 1
    s = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(lib.pygat_wgrad_workspace_bytes(Fin, H, Fo, split_k) // 4, device=dev)
    dW = torch.full((H, Fin, Fo), float("nan"), device=dev)
    _lib.check(lib.pygat_wgrad(N, Fin, H, Fo, X.data_ptr(), Fin, dWh.data_ptr(), None, None, dW.data_ptr(), split_k, ws.data_ptr(),
                               0, 0, 0, s), "wgrad")
    packed = torch.empty(Fin, R, device=dev)
    ops.gemm(True, False, Fin, R, N, X, Fin, dWh, R, [(R, packed, R)], split_k=split_k, mode="split-bf16")
    ref = torch.empty(H, Fin, Fo, device=dev)
    _lib.check(lib.pygat_unpack_wgrad(H, Fin, Fo, packed.data_ptr(), R, 0, ref.data_ptr(), s), "unpack")
    torch.cuda.synchronize()
    assert torch.equal(_bits(dW), _bits(ref))
    assert torch.allclose(dW, (X.double().t() @ dWh.double()).view(Fin, H, Fp)[:, :, :Fo].permute(1, 0, 2).float(), rtol=1e-4, atol=1e-2)
