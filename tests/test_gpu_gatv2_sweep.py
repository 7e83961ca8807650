"""The GATv2 level (SpGraphAttentionLayerV2, layers.py:234-316; K2's V2 variant, csrc/k6_gatv2_backward.hip) against fp64 at
every shape it can be asked to run:
  a. one (H, F') per lane shape (LPR, VEC) pick_lanes (csrc/attn_common.h) can choose for a V2 row of R = H * Fp floats;
  b. a 24-seed shape fuzz;
  c. the cut-row ladder: chains of more than 32 pieces through the list-driven fix-ups of both backward passes;
  d. explicit dropout masks at wide rows (the perm_t mask path of the column pass at VEC 3 and 4);
  e. the internal node order and the self-loop-only tail at R = 512 and 1024, fused and with a skip projection;
  f. the 32768-node R-MAT graph against the C oracle;
  g. the width fences (H * Fp <= 1024, F' <= 256), raised before any kernel runs.
Whole levels go through parity.check_level_v2 (the flip-aware rule for per-feature LeakyReLU kinks) unless a case says
otherwise."""
import re

import numpy as np
import pytest
import torch

import parity
from ladder_case import _ladder_graph
from oracle import gat_oracle as O
from tail_case import _iso_csr, _spy
from test_gpu_gatv2 import v2params
from test_gpu_parity import pg  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _asym_csr(N, seed, p=0.04, hub=(5, 150)):
    """An asymmetric pattern with self loops and one hub ROW (its column stays ordinary)."""
    rng = np.random.default_rng(seed)
    dense = (rng.random((N, N)) < p) | np.eye(N, dtype=bool)
    hn, hd = hub
    if N > hn:
        dense[hn, rng.choice(N, size=min(hd, N), replace=False)] = True
    rowptr = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)
    return rowptr, np.nonzero(dense)[1].astype(np.int32)


def _data(N, Fin, H, Fo, skip, concat, seed):
    W, a, Sk = v2params(H, Fin, Fo, skip, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(N, Fin, dtype=torch.float64, generator=gen)
    G = torch.randn(N, H * Fo if concat else Fo, dtype=torch.float64, generator=gen)
    return x, W, a, Sk, G


def run_v2(pg, x, rowptr, col, W, a, Sk, concat, G, slot=64, need_dx=True, graph=None):  # noqa: F811
    g = graph if graph is not None else pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV),
                                                    slot_edges=slot)
    xd = x.float().to(DEV).requires_grad_(need_dx)
    Wd = W.float().to(DEV).requires_grad_(True)
    ad = a.float().to(DEV).requires_grad_(True)
    Sd = Sk.float().to(DEV).requires_grad_(True) if Sk is not None else None
    out = pg.GATv2LevelFn.apply(xd, Wd, ad, Sd, g, 0.2, concat)
    out.backward(G.float().to(DEV))
    torch.cuda.synchronize()
    grads = {"dX": xd.grad, "dW": Wd.grad, "da": ad.grad}
    if Sd is not None:
        grads["dW_skip"] = Sd.grad
    return out, grads, g


def check_v2(res, x, rowptr, col, W, a, Sk, concat, G, what):
    out, grads, _ = res
    grads = {n: (None if v is None else v.cpu()) for n, v in grads.items()}
    return parity.check_level_v2(out.detach().cpu(), grads, x.numpy(), rowptr, col, W.numpy(), a.numpy(), 0.2, concat, G.numpy(),
                                 None if Sk is None else Sk.numpy(), what=what)


# ----------------------------------------------------------------------------------------------------------------------------
# a. every lane shape: R = H * Fp -> NCH = R / 4 float4 chunks -> LPR = next pow2 >= NCH (<= 64), VEC = ceil(NCH / 64)
LANES = [  # (H, F', Fin, LPR, VEC)
    (1, 3, 8, 1, 1),        # R 4   (F' 3 padded to 4)
    (2, 4, 12, 2, 1),       # R 8
    (1, 13, 10, 4, 1),      # R 16  (F' 13 padded to 16)
    (8, 4, 16, 8, 1),       # R 32
    (4, 16, 20, 16, 1),     # R 64
    (2, 64, 24, 32, 1),     # R 128
    (4, 50, 32, 64, 1),     # R 256 (F' 50 padded to 64)
    (8, 64, 16, 64, 2),     # R 512
    (6, 121, 24, 64, 3),    # R 768 (F' 121 padded to 128)
    (4, 256, 32, 64, 4),    # R 1024, the widest row GATv2LevelFn takes
    (8, 128, 16, 64, 4),    # R 1024
]
# each lane shape twice: concat / no skip / 4-edge slots / symmetric pattern, and mean / skip / 64-edge slots / asymmetric
VARIANTS = [(True, False, 4, True), (False, True, 64, False)]


@pytest.mark.parametrize("variant", VARIANTS, ids=["concat-slot4-sym", "mean-skip-slot64-asym"])
@pytest.mark.parametrize("H,Fo,Fin,lpr,vec", LANES, ids=[f"R{h * max(4, 1 << (f - 1).bit_length())}-{h}x{f}" for h, f, *_ in LANES])
def test_v2_every_lane_shape(pg, H, Fo, Fin, lpr, vec, variant):  # noqa: F811
    from pygat_amd._lib import padded_width
    concat, skip, slot, sym = variant
    R = H * padded_width(Fo)
    nch = R // 4
    assert (lpr, vec) == ((1 << (nch - 1).bit_length(), 1) if nch <= 64 else (64, -(-nch // 64)))   # the table is pick_lanes'
    N = 240
    if sym:
        rowptr, col = O.random_symmetric_csr(N, 5, 20 + H, hub=(4, 150))
    else:
        rowptr, col = _asym_csr(N, 30 + H)
    x, W, a, Sk, G = _data(N, Fin, H, Fo, skip, concat, 40 + Fo)
    check_v2(run_v2(pg, x, rowptr, col, W, a, Sk, concat, G, slot=slot), x, rowptr, col, W, a, Sk, concat, G,
             f"v2 lanes LPR {lpr} VEC {vec} [{H}x{Fo}, Fin {Fin}, concat {concat}, skip {skip}, slot {slot}, sym {sym}]")


# ----------------------------------------------------------------------------------------------------------------------------
# b. fuzz
@pytest.mark.parametrize("seed", range(24))
def test_v2_fuzz_level(pg, seed):  # noqa: F811
    rng = np.random.default_rng(2000 + seed)
    N = 1 if seed == 0 else int(rng.integers(1, 401))
    redraws = 0
    while True:           # a draw wider than the V2 row limit is drawn again (the fence has its own test), never narrowed
        H = int(rng.choice([1, 2, 3, 4, 6, 8]))
        Fo = int(rng.choice([1, 3, 4, 5, 16, 17, 64, 100, 121, 256]))
        if H * max(4, 1 << (Fo - 1).bit_length()) <= 1024:
            break
        redraws += 1
    Fin = int(rng.integers(1, 70))
    skip, concat = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    slot = int(rng.choice([4, 8, 16, 64]))
    if N == 1:
        rowptr, col = np.array([0, 1], np.int32), np.array([0], np.int32)
    elif rng.integers(0, 2):
        rowptr, col = O.random_symmetric_csr(N, float(rng.uniform(0.5, 12)), seed, hub=(0, int(rng.integers(1, N + 1))))
    else:
        dense = (rng.random((N, N)) < rng.uniform(0.01, 0.3)) | np.eye(N, dtype=bool)
        rowptr = np.concatenate([[0], np.cumsum(dense.sum(1))]).astype(np.int32)
        col = np.nonzero(dense)[1].astype(np.int32)
    x, W, a, Sk, G = _data(N, Fin, H, Fo, skip, concat, 300 + seed)
    tag = f"v2 fuzz {seed}: N={N} H={H} Fo={Fo} Fin={Fin} skip={skip} concat={concat} slot={slot} E={len(col)} redraws={redraws}"
    check_v2(run_v2(pg, x, rowptr, col, W, a, Sk, concat, G, slot=slot), x, rowptr, col, W, a, Sk, concat, G, tag)


# ----------------------------------------------------------------------------------------------------------------------------
# c. cut chains of every length
def _pieces(pattern, slot):
    cut = pattern._alt[(slot, True)][2]
    return cut[:, 2].cpu().numpy() if cut is not None else np.zeros(0, np.int32)


@pytest.mark.parametrize("H,Fo", [(1, 16), (2, 64), (8, 64), (4, 256)])     # R 16 / 128 / 512 / 1024
def test_v2_cut_rows_of_every_length(pg, H, Fo):  # noqa: F811
    rowptr, col = _ladder_graph()
    N, Fin = len(rowptr) - 1, 32
    x, W, a, _, G = _data(N, Fin, H, Fo, False, True, 50 + H)
    for slot in (4, 8):
        res = run_v2(pg, x, rowptr, col, W, a, None, True, G, slot=slot)
        g = res[2]
        pf, pb = _pieces(g.fwd, slot), _pieces(g.bwd, slot)
        # the column pass walks g.bwd, the row pass g.fwd: both lists hold every chain length from 2 up
        for p in (pf, pb):
            assert len(p) and p.min() == 2
            if slot == 4:
                assert p.max() > 32 and (p > 32).sum() >= 2, p.max()     # whole-work-group chains in both passes
        check_v2(res, x, rowptr, col, W, a, None, True, G,
                 f"v2 cut rows {H}x{Fo}, {slot}-edge slots (chains up to {pf.max()} / {pb.max()} pieces)")


# ----------------------------------------------------------------------------------------------------------------------------
# d. dropout masks at wide rows (check_autograd: explicit masks, N = 60)
@pytest.mark.parametrize("H,Fin,Fo,skip,concat", [(4, 16, 256, False, True), (6, 12, 121, True, False)])
def test_v2_dropout_explicit_masks_wide(pg, H, Fin, Fo, skip, concat):  # noqa: F811
    from pygat_amd.gatv2 import gatv2_level
    N, p = 60, 0.5
    rowptr, col = O.random_symmetric_csr(N, 5, 3, hub=(2, 40))
    E = len(col)
    W, a, Sk = v2params(H, Fin, Fo, skip, 6)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(N, Fin, dtype=torch.float64, generator=gen)
    G = torch.randn(N, H * Fo if concat else Fo, dtype=torch.float64, generator=gen)
    keep = lambda *s: (torch.rand(*s, generator=gen) >= p).double() / (1 - p)  # noqa: E731
    mx, mi, mj, matt = keep(H, N, Fin), keep(H, N, Fo), keep(H, N, Fo), keep(E, H)
    leaves = [x, W, a] + ([Sk] if skip else [])

    def oracle(*lv):
        c = lambda m: m.to(lv[0].dtype)  # noqa: E731
        outs = [O.sparse_head_forward_v2(lv[0], rowptr, col, lv[1][h], lv[2][h], 0.2, concat, lv[3][h] if skip else None,
                                         c(mx[h]), c(mi[h]), c(mj[h]), c(matt[:, h])) for h in range(H)]
        return torch.cat(outs, 1) if concat else torch.mean(torch.stack(outs, 1), 1)
    g = pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV), slot_edges=16)
    xd = x.float().to(DEV).requires_grad_(True)
    Ws = [W[h].float().to(DEV).requires_grad_(True) for h in range(H)]
    As = [a[h].float().to(DEV).reshape(1, -1).requires_grad_(True) for h in range(H)]
    Ss = [Sk[h].float().to(DEV).requires_grad_(True) for h in range(H)] if skip else None
    masks = dict(x=mx.float().to(DEV), whi=mi.float().to(DEV), whj=mj.float().to(DEV), att=matt.float().to(DEV))
    out = gatv2_level(xd, g, Ws, As, Ss, 0.2, concat, p, masks=masks)
    out.backward(G.float().to(DEV))
    got = [xd.grad, torch.stack([w.grad for w in Ws]), torch.stack([w.grad.reshape(-1) for w in As])]
    if skip:
        got.append(torch.stack([w.grad for w in Ss]))
    rep, _ = parity.check_autograd(out, got, oracle, leaves, G, ["dX", "dW", "da", "dW_skip"],
                                   what=f"v2 dropout wide[{H},{Fin},{Fo},{skip},{concat}]")
    print(f"v2 dropout wide[{H}x{Fo}]: " + ", ".join(f"{k} {v:.2e}" for k, v in rep.items()))


# ----------------------------------------------------------------------------------------------------------------------------
# e. internal order and the self-loop-only tail at wide rows
def _force_tail_routes(monkeypatch):
    from pygat_amd import ops
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES", 0)
    monkeypatch.setattr(ops, "RENUMBER_MIN_BYTES_TAIL", 0)
    monkeypatch.setattr(ops, "DA_MIN_BYTES", 0)


@pytest.mark.parametrize("skip", [False, True], ids=["fused-tail", "skip-tail"])
@pytest.mark.parametrize("H,Fo", [(8, 64), (4, 256)])      # R 512 / 1024
def test_v2_tail_wide_rows_against_oracle(pg, monkeypatch, H, Fo, skip):  # noqa: F811
    """GATv2LevelFn renumbering itself (no gradient into x), the tail through both streams.  Without a skip projection the
    backward tail is pygat_gat_backward_tail writing dWW at stride 2R; with one, dWW[tail:] = [Gp | 0] is copied from GRW."""
    from pygat_amd import gatv2, ops
    N, Fin = 9000, 16
    rowptr, col = _iso_csr(N, 0.5, 95 + H)
    x, W, a, Sk, G = _data(N, Fin, H, Fo, skip, True, 60 + H)
    _force_tail_routes(monkeypatch)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(gatv2, "lib", ops.lib)
    res = run_v2(pg, x, rowptr, col, W, a, Sk, True, G, need_dx=False)
    g = res[2]
    assert g._ordered is not None and (seen["fwd_stream"], seen["bwd_stream"]) == (1, 0 if skip else 1), seen
    check_v2(res, x, rowptr, col, W, a, Sk, True, G, f"v2 tail {H}x{Fo}, skip {skip}")


# ----------------------------------------------------------------------------------------------------------------------------
# f. the 32768-node R-MAT graph against the C oracle (fp64 build = truth, fp32 build = the reference's precision).  `out` and da
# by the rule of test_gpu_fullsize.test_fullsize_gatv2_level_against_c_oracle (4 x the fp32 C oracle's own error).  dW / dX:
# at 8 x 16 by the flip-aware rule (parity.close_level_grads_v2, z and de in fp64 chunks).  At 4 x 64 and 4 x 256 neither rule
# can price them: 100-400 M (edge, feature) pairs give each fp32 run its own handful of LeakyReLU branch flips, and one flip at
# a low-degree row moves dW by up to ~1.  Measured on this graph: the HIP residual of every worst dW column is exactly rank one,
# [X_i ; X_j] of an existing edge (|cos| 1.0000) whose z is 1e-7 .. 3e-5 of |Whi| + |Whj| -- a flip, not a kernel error --
# but 4 x the fp32 oracle (which drew milder flips) is a lottery, and the flip fit hits KINK_MAX (2174 pairs in the band at
# 4 x 256) and the count leash (the fit settles on 45 flips against the fp32 oracle's 6 at 4 x 64).  Those two run the
# VEC 1 / VEC 4 rows and both node orders on a large graph for `out`, da and the route.
@pytest.mark.parametrize("H,Fo,x_grad", [(8, 16, True), (4, 64, True), (4, 256, True), (4, 256, False)],
                         ids=["8x16", "4x64", "4x256", "4x256-internal-order"])
def test_v2_midsize_against_c_oracle(pg, monkeypatch, H, Fo, x_grad):  # noqa: F811
    from oracle import c_oracle
    from pygat_amd import gatv2, ops
    from pygat_amd._lib import padded_width
    from pygat_amd.rmat import rmat_csr
    rowptr, col = rmat_csr(15, 200_000, seed=7, device=DEV)
    graph = pg.CSRGraph(rowptr, col)
    N, Fin = graph.n, 64
    g = torch.Generator(device=DEV).manual_seed(H + Fo)
    X = torch.randn(N, Fin, generator=g, device=DEV).requires_grad_(x_grad)
    W = (torch.randn(H, 2 * Fin, Fo, generator=g, device=DEV) * (1.414 * (2.0 / (2 * Fin + Fo)) ** 0.5)).requires_grad_(True)
    a = (torch.randn(H, Fo, generator=g, device=DEV) * (1.414 * (2.0 / (1 + Fo)) ** 0.5)).requires_grad_(True)
    G = torch.randn(N, H * Fo, generator=g, device=DEV)
    seen = _spy(monkeypatch)
    monkeypatch.setattr(gatv2, "lib", ops.lib)
    out = gatv2.GATv2LevelFn.apply(X, W, a, None, graph, 0.2, True)
    out.backward(G)
    torch.cuda.synchronize()
    internal = graph._ordered is not None
    if x_grad:
        assert not internal and seen["fwd_stream"] == 0, seen            # caller order: a gradient into x keeps it
    else:
        assert N * 2 * H * padded_width(Fo) * 4 >= ops.RENUMBER_MIN_BYTES   # worth renumbering on its own ...
        assert internal and (seen["fwd_stream"], seen["bwd_stream"]) == (1, 1), seen   # ... and the tail streams ran
    args = (X.detach().cpu().numpy(), rowptr.cpu().numpy(), col.cpu().numpy(), W.detach().cpu().numpy(), a.detach().cpu().numpy(),
            0.2, True, G.cpu().numpy())
    tp = c_oracle.transpose_pattern(args[1], args[2])
    r64 = c_oracle.level_v2(*args, want_dx=x_grad, tp=tp, dtype=np.float64)
    r32 = c_oracle.level_v2(*args, want_dx=x_grad, tp=tp)
    route = "internal order + tail" if internal else "caller order"
    e, e32 = parity.close_grad(out.detach(), r64["out"], r32["out"], f"v2 midsize {H}x{Fo} out")
    ea, ea32 = parity.close_grad(a.grad, r64["da"], r32["da"], f"v2 midsize {H}x{Fo} da")
    msg = f"v2 midsize[{H}x{Fo}, {route}]: out err {e:.2e} (fp32 oracle {e32:.2e}); da err {ea:.2e} (fp32 oracle {ea32:.2e})"
    if (H, Fo) == (8, 16):
        grads = {"dX": X.grad.cpu() if x_grad else None, "dW": W.grad.cpu(), "da": a.grad.cpu()}
        rep = parity.close_level_grads_v2(grads, *args, what=f"v2 midsize {H}x{Fo}", refs=(r64, r32))
        msg += f"; {rep['flips']}; " + ", ".join(f"{n} {rep['hip'][n]:.2e} (fp32 oracle {rep['fp32'][n]:.2e})" for n in rep["hip"])
    print(msg)


# ----------------------------------------------------------------------------------------------------------------------------
# g. width fences, raised before the level's projection or attention kernels run
HOST_QUERIES = {"pygat_head_group"}      # shape queries of _Level: no launch


def _no_kernels(monkeypatch):
    """Record every library entry point and GEMM the level calls, host-side shape queries excepted."""
    from pygat_amd import gatv2, ops
    called = []

    class Guard:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)

            def wrapped(*args):
                if name not in HOST_QUERIES:
                    called.append(name)
                return fn(*args)
            return wrapped
    monkeypatch.setattr(ops, "lib", Guard(ops.lib))
    monkeypatch.setattr(gatv2, "lib", Guard(gatv2.lib))
    real_gemm = ops.gemm

    def gemm(*args, **kw):
        called.append("gemm")
        return real_gemm(*args, **kw)
    monkeypatch.setattr(ops, "gemm", gemm)
    monkeypatch.setattr(gatv2, "gemm", gemm)
    return called


@pytest.mark.parametrize("H,Fo,Fp", [(5, 256, 256), (9, 128, 128), (2, 257, None)], ids=["5x256", "9x128", "2x257"])
def test_v2_width_fences(pg, monkeypatch, H, Fo, Fp):  # noqa: F811
    from pygat_amd.gatv2 import GATv2LevelFn
    N, Fin = 50, 8
    rowptr, col = O.random_symmetric_csr(N, 4, 1)
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV))
    x = torch.randn(N, Fin, device=DEV)
    W = torch.randn(H, 2 * Fin, Fo, device=DEV, requires_grad=True)
    a = torch.randn(H, Fo, device=DEV, requires_grad=True)
    called = _no_kernels(monkeypatch)
    if Fp is not None:
        msg = f"pygat_amd: GATv2 row too wide: H x padded F' = {H} x {Fp} = {H * Fp} > 1024; shard the heads"
    else:
        msg = f"pygat_amd: head width {Fo} unsupported (1..256)"
    with pytest.raises(ValueError, match="^" + re.escape(msg) + "$") as exc:
        GATv2LevelFn.apply(x, W, a, None, graph, 0.2, True)
    assert called == [], called
    print(f"GATv2LevelFn {H}x{Fo}: {exc.type.__name__}: {exc.value}")


def test_v1_head_width_fence(pg, monkeypatch):  # noqa: F811
    N, Fin, H, Fo = 50, 8, 2, 257
    rowptr, col = O.random_symmetric_csr(N, 4, 1)
    graph = pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV))
    x = torch.randn(N, Fin, device=DEV)
    W = torch.randn(H, Fin, Fo, device=DEV, requires_grad=True)
    a = torch.randn(H, 2 * Fo, device=DEV, requires_grad=True)
    called = _no_kernels(monkeypatch)
    with pytest.raises(ValueError, match="^" + re.escape("pygat_amd: head width 257 unsupported (1..256)") + "$") as exc:
        pg.GATLevelFn.apply(x, W, a, None, graph, 0.2, True)
    assert called == [], called
    print(f"GATLevelFn {H}x{Fo}: {exc.type.__name__}: {exc.value}")
