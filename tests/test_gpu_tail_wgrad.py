"""The weight gradient that forms the self-loop-only tail's dWh rows itself (pygat_wgrad_tail_blocked: the streamed-K split
kernel reads dWh before row_first and G / y behind it): bit for bit the dW of pygat_gat_backward_tail + pygat_wgrad_blocked, the
fp64 product under tests/parity.py's rule, "not taken" for what its kernel does not run, and ops picks it where -- and only
where -- nothing else reads the tail's dWh, ds and dt rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from parity import close_grad
from test_gpu_col_finish import _bits, _call_spy, _level

pytestmark = pytest.mark.gpu

H, FO = 8, 16
R = H * FO
NOT_TAKEN = 1


def _slab(n, split_k):
    """Rows per slab and slab count of the streamed-K split kernel (csrc/k1_gemm_x3.hip launch_tn_x3w, one 128 x 128 tile)."""
    cdiv = lambda a, b: -(-a // b)  # noqa: E731
    kps16 = cdiv(cdiv(n, split_k), 48) * 48
    sw = min(cdiv(n, kps16), 256)
    kps = cdiv(cdiv(n, sw), 96) * 96
    return kps, cdiv(n, kps)


# n, row_first, Fin, split_k, urow, elu -- between them: row_first not a multiple of 32 and strictly inside a slab (a, b, c, e), in
# the first slab (b), n - 1 (c), on a slab border (d: every slab all prefix or all tail); a partial last step of the last slab
# (n % 96 != 0 and n % 32 != 0: a, b, c, e); both row maps, with and without ELU.  Fin 128 and 96 (a tile of 128 rows of C cut by
# M).  Fin 64: the streamed-K split kernel does not take 64 rows of C (try_gemm_tn_x3: M <= 64; pygat_wgrad_blocked runs its
# fp32-MFMA sibling there), so the entry must answer "not taken" -- test_fin64_is_not_taken.
CASES = [dict(id="a", n=9001, row_first=3961, Fin=128, split_k=8, urow=False, elu=True),
         dict(id="b", n=9001, row_first=37, Fin=96, split_k=8, urow=True, elu=True),
         dict(id="c", n=9001, row_first=9000, Fin=128, split_k=8, urow=True, elu=False),
         dict(id="d", n=20000, row_first=7680, Fin=128, split_k=64, urow=False, elu=False),
         dict(id="e", n=12345, row_first=5000, Fin=128, split_k=46, urow=True, elu=True)]
_cache = {}


def _run(cfg):
    """Both sequences on one case, once: the stream into a full dWh + pygat_wgrad_blocked, and the new entry on a dWh whose tail
    rows are NaN.  -> dict of CPU tensors."""
    if cfg["id"] in _cache:
        return _cache[cfg["id"]]
    from pygat_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    n, rf, Fin, split_k = cfg["n"], cfg["row_first"], cfg["Fin"], cfg["split_k"]
    kps, slabs = _slab(n, split_k)
    assert slabs >= 3 and n >= 4096
    if cfg["id"] in "abce":
        assert rf % 32 != 0 and rf % kps != 0 and n % 96 != 0 and n % 32 != 0
    if cfg["id"] == "b":
        assert rf < kps
    if cfg["id"] == "d":
        assert rf % kps == 0
    gen = torch.Generator().manual_seed(n + rf)
    X = torch.randn(n, Fin, generator=gen)
    G = torch.randn(n, R, generator=gen)
    y = torch.randn(n, R, generator=gen)
    pick = torch.rand(n, R, generator=gen)
    y[pick < 0.1] = 0.0            # ELU' = 0 + 1 exactly
    y[pick > 0.9] = -1.0           # ELU' = 0 exactly
    assert (y > 0).any() and (y == 0).any() and (y == -1).any()
    dWh = torch.randn(n, R, generator=gen)
    urow = None
    if cfg["urow"]:                # any order before the tail, increasing on it (CSRGraph.degree_ordered sorts stably)
        perm = torch.randperm(n, generator=gen)
        urow = torch.cat([perm[:rf], perm[rf:].sort().values]).to(torch.int32)
        assert bool((urow[rf + 1:] > urow[rf:-1]).all()) if n - rf > 1 else True
    flags = _lib.F_ELU if cfg["elu"] else 0
    s = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    Xd, Gd, yd, ud = X.to(dev), G.to(dev), y.to(dev), (urow.to(dev) if urow is not None else None)
    full = dWh.to(dev)
    full[rf:] = float("nan")
    ws = torch.empty(lib.pygat_wgrad_workspace_bytes(Fin, H, FO, split_k) // 4, device=dev)
    _lib.check(lib.pygat_gat_backward_tail(rf, n - rf, H, FO, flags, p(Gd), p(yd), p(ud), p(full), 0, 0, None, None, s), "tail")
    dW_old = torch.full((H, Fin, FO), float("nan"), device=dev)
    _lib.check(lib.pygat_wgrad_blocked(n, Fin, H, FO, p(Xd), Fin, None, p(full), None, None, p(dW_old), split_k, p(ws), 0, 0, 0, s),
               "wgrad")
    torch.cuda.synchronize()
    holed = dWh.to(dev)
    holed[rf:] = float("nan")      # the tail rows of dWh must not be read
    ws.fill_(float("nan"))
    dW_new = torch.full((H, Fin, FO), float("nan"), device=dev)
    rc = lib.pygat_wgrad_tail_blocked(n, Fin, H, FO, p(Xd), Fin, None, p(holed), p(dW_new), split_k, p(ws), rf, flags, p(Gd), p(yd),
                                      p(ud), 0, s)
    assert rc == 0, (rc, lib.pygat_last_error())
    torch.cuda.synchronize()
    out = dict(X=X, G=G, y=y, dWh=dWh, urow=urow, dW_old=dW_old.cpu(), dW_new=dW_new.cpu(), tail_rows=full[rf:].cpu())
    _cache[cfg["id"]] = out
    return out


@pytest.mark.parametrize("cfg", CASES, ids=[c["id"] for c in CASES])
def test_entry_is_bitwise_stream_then_wgrad(cfg):
    r = _run(cfg)
    assert torch.isfinite(r["dW_old"]).all() and torch.isfinite(r["dW_new"]).all()
    assert torch.equal(_bits(r["dW_new"]), _bits(r["dW_old"]))


@pytest.mark.parametrize("cfg", CASES, ids=[c["id"] for c in CASES])
def test_entry_against_fp64(cfg):
    """The same dW against X^T [dWh ; G_u ELU'(y_u)] formed in fp64 from the fp32 inputs; ref32 = the same product in fp32 on
    the CPU (tests/parity.py: max(1e-5, 4 x its error)).  Independent of the stream: both paths wrong alike would pass the
    bitwise test above."""
    r = _run(cfg)
    n, rf = cfg["n"], cfg["row_first"]
    u = r["urow"][rf:].long() if r["urow"] is not None else torch.arange(rf, n)

    def product(dt):
        g, yy = r["G"][u].to(dt), r["y"][u].to(dt)
        tail = g * torch.where(yy > 0, torch.ones_like(yy), yy + 1) if cfg["elu"] else g
        B = torch.cat([r["dWh"][:rf].to(dt), tail])
        return torch.einsum("nk,nhf->hkf", r["X"].to(dt), B.view(n, H, FO))
    e, own = close_grad(r["dW_new"], product(torch.float64).numpy(), product(torch.float32).double().numpy(), f"dW {cfg['id']}")
    print(f"wgrad_tail {cfg}: err {e:.2e} (fp32 CPU {own:.2e})")
    if cfg["elu"]:                 # the stream's rows are what the reference here forms, exactly (one fp32 multiply)
        g, yy = r["G"][u], r["y"][u]
        assert torch.equal(_bits(r["tail_rows"]), _bits(g * torch.where(yy > 0, torch.ones_like(yy), yy + 1)))


@pytest.mark.parametrize("n,rf,split_k", [(9001, 37, 8), (20000, 7680, 64)])
def test_fin64_is_not_taken(n, rf, split_k):
    """Fin = 64 at 8 x 16: "not taken", nothing launched -- the level then runs the stream and pygat_wgrad_blocked."""
    from pygat_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    X, G, y, dWh = (torch.randn(n, w, device=dev) for w in (64, R, R, R))
    ws = torch.full((lib.pygat_wgrad_workspace_bytes(64, H, FO, split_k) // 4,), float("nan"), device=dev)
    dW = torch.full((H, 64, FO), float("nan"), device=dev)
    assert lib.pygat_wgrad_tail_blocked(n, 64, H, FO, X.data_ptr(), 64, None, dWh.data_ptr(), dW.data_ptr(), split_k, ws.data_ptr(), rf,
                                        _lib.F_ELU, G.data_ptr(), y.data_ptr(), None, 0, None) == NOT_TAKEN
    torch.cuda.synchronize()
    assert torch.isnan(dW).all() and torch.isnan(ws).all()


def test_entry_refuses_what_its_kernel_does_not_run():
    """Every condition under which pygat_wgrad_blocked would not run the streamed-K split kernel with its dW-writing reduce, and
    what the tail rows need on top: "not taken", before any launch (dW and the workspace stay NaN).  A ds column term and a head
    range are not expressible in this entry's arguments: ops keeps such levels off it (test_other_levels_keep_their_sequences)."""
    from pygat_amd import _lib
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    n, Fin, rf, split_k = 9001, 128, 3000, 8
    X = torch.randn(n, Fin + 4, device=dev)
    G, y, dWh = torch.randn(n, R + 4, device=dev), torch.randn(n, R + 4, device=dev), torch.randn(n, R, device=dev)
    ws = torch.full((lib.pygat_wgrad_workspace_bytes(Fin, H, FO, 64) // 4,), float("nan"), device=dev)
    dW = torch.full((H, Fin, FO), float("nan"), device=dev)
    blk = _lib.ColBlocks(64, n * 64)
    base = dict(n=n, Fin=Fin, H=H, Fo=FO, X=X.data_ptr(), ldx=Fin + 4, blk=None, dWh=dWh.data_ptr(), split_k=split_k, flags=_lib.F_ELU,
                G=G.data_ptr(), y=y.data_ptr(), mode=0)

    def call(**kw):
        a = dict(base, **kw)
        return lib.pygat_wgrad_tail_blocked(a["n"], a["Fin"], a["H"], a["Fo"], a["X"], a["ldx"], a["blk"], a["dWh"], dW.data_ptr(),
                                            a["split_k"], ws.data_ptr(), rf, a["flags"], a["G"], a["y"], None, a["mode"], None)
    assert call(mode=1) == NOT_TAKEN                                   # fp32-mfma products
    assert call(X=X.data_ptr() + 4) == NOT_TAKEN                       # X not 16-byte aligned
    assert call(ldx=Fin + 3) == NOT_TAKEN                              # ... nor its rows
    assert call(G=G.data_ptr() + 8) == NOT_TAKEN and call(y=y.data_ptr() + 4) == NOT_TAKEN and call(dWh=dWh.data_ptr() + 4) == NOT_TAKEN
    assert call(flags=_lib.F_ELU | _lib.F_SKIP) == NOT_TAKEN           # a skip projection reads every row's Gp
    assert call(Fo=12) == NOT_TAKEN                                    # F' != Fp: G / y rows are not dWh rows
    assert call(blk=C.byref(blk), ldx=64) == NOT_TAKEN                 # a column-blocked x takes the general kernel
    assert call(split_k=1) == NOT_TAKEN and call(n=4000) == NOT_TAKEN and call(Fin=64, H=4) == NOT_TAKEN   # no streamed-K kernel
    assert call(n=200000, split_k=8) == NOT_TAKEN                      # 25 000 rows a slab: more ids than the LDS holds
    assert call(mode=7) == -1 and b"unknown product mode" in lib.pygat_last_error()
    assert call(G=None) == -1 and call(n=rf) == -1
    torch.cuda.synchronize()
    assert torch.isnan(dW).all() and torch.isnan(ws).all()


def _run_level(monkeypatch, data, min_bytes, skip=False, ranged=False):
    import pygat_amd as pg
    from pygat_amd import ops
    dev = torch.device("cuda", 0)
    rowptr, col, x, W, a, Ws, G = data
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "TAIL_WGRAD_MIN_BYTES", min_bytes)
    calls = _call_spy(monkeypatch)
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=dev), torch.as_tensor(col, device=dev))
    Wd, ad = W.to(dev).requires_grad_(True), a.to(dev).requires_grad_(True)
    Wsd = Ws.to(dev).requires_grad_(True) if skip else None
    out = pg.GATLevelFn.apply(x.to(dev), Wd, ad, Wsd, graph, 0.2, True, (2, 4) if ranged else None)
    n_fwd = len(calls)
    out.backward(G.to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu(), Wd.grad.cpu(), ad.grad.cpu(), calls[n_fwd:]


def test_level_takes_the_entry_and_keeps_its_bits(monkeypatch):
    """8 heads x 16 on a 20 000-node graph, half its nodes isolated: with the threshold at 0 the backward is prepare -> column
    pass (main + its own fix-up) -> a-gradient fold -> pygat_wgrad_tail_blocked, no tail stream in any form; out, dW and da are
    the bits of the sequence above the threshold."""
    data = _level(20000, 128, H, FO, 48)
    o0, dW0, da0, c0 = _run_level(monkeypatch, data, 1 << 60)
    o1, dW1, da1, c1 = _run_level(monkeypatch, data, 0)
    assert "gat_backward_tail" in c0 and "wgrad_tail_blocked" not in c0, c0
    assert c1 == ["gat_backward_prepare", "gat_backward_col", "a_grad_fold", "wgrad_tail_blocked"], c1
    assert torch.equal(o1, o0) and torch.equal(_bits(dW1), _bits(dW0)) and torch.equal(_bits(da1), _bits(da0))
    assert torch.isfinite(dW1).all() and torch.isfinite(da1).all()


@pytest.mark.parametrize("kind", ["skip", "ranged"])
def test_other_levels_keep_their_sequences(kind, monkeypatch):
    """A skip projection's weight gradient reads every row's Gp and a ranged backward has no tail route: the threshold does not
    move their call sequences."""
    data = _level(12000, 64, H, FO, 49, skip=(kind == "skip"))
    seqs = [_run_level(monkeypatch, data, mb, skip=(kind == "skip"), ranged=(kind == "ranged")) for mb in (1 << 60, 0)]
    assert seqs[0][3] == seqs[1][3] and "wgrad_tail_blocked" not in seqs[1][3], seqs[1][3]
    assert "gat_backward_col" in seqs[1][3] and "wgrad_blocked" in seqs[1][3]
    for q in range(3):
        assert torch.equal(_bits(seqs[0][q]), _bits(seqs[1][q]))


def test_tail_wgrad_kernel_footprint():
    """gemm_tn_x3w_kernel<true> as the loaded code object reports it: no scratch, and registers for two waves per SIMD (one
    8-wave work-group per CU: 512 / 2 = 256 a lane)."""
    from pygat_amd._lib import lib
    regs, scratch = C.c_int(-1), C.c_int(-1)
    assert lib.pygat_kernel_footprint(b"tn_x3w_tail", C.byref(regs), C.byref(scratch)) == 0, lib.pygat_last_error()
    assert 0 < regs.value <= 256 and scratch.value == 0, (regs.value, scratch.value)
