"""Train-mode dropout with SEEDED masks: the kernels against tests/philox_ref.py bit for bit, and the seeded level against
the oracle (fp64 autograd) under the masks the reference generator rebuilds from the seed.

Everything the kernels draw is a function of (seed, stream id, element): Philox-4x32-10 in three counter layouts
(pygat_amd/csrc/rng.h, k7_dropout.hip, k9_sparse.hip).  philox_ref.py restates them in NumPy, so
  * pygat_dropout_mask / _mask2 / _bits / _expand are compared EXACTLY (torch.equal),
  * pygat_dropout_head_sum and the seeded pygat_project_sparse / pygat_wgrad_sparse against fp64 products under the
    reference masks (tests/parity.py close_grad), the sparse pair also bitwise against the same calls on explicit bytes,
  * GATLevelDropoutFn with a seed, on every projection path (mask bytes through the MFMA and the narrow kernels, the wide
    operand, sparse features) and every backward flavour, against oracle.level_forward under level_masks(seed): out, dX,
    dW, da, dW_skip under the one rule of tests/parity.py -- the forward AND the backward have to draw the masks the
    reference generator says they draw.
Seeds carry a non-zero high half (the model draws them from randint(0, 2**62)).
"""
import functools

import numpy as np
import pytest
import torch

import philox_ref as R
from oracle import gat_oracle as O
from parity import KINK_TAU, check_autograd, close_grad
from test_gpu_parity import params, pg  # noqa: F401
from test_gpu_sparse_features import _features

pytestmark = pytest.mark.gpu

SEED_LO = 12345
SEED_HI = 0x2F00_0000_0000_0000 + 12345       # same low half: the two differ in the high 32 bits only
SEEDS = [SEED_LO, SEED_HI]
DEV = "cuda:0"
GUARD = -7.0


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _guarded(count):
    """[count + 4] floats filled with GUARD: the kernel writes the first `count`."""
    return torch.full((count + 4,), GUARD, device=DEV)


def _guard_ok(buf, count):
    return bool((buf[count:] == GUARD).all())


# ---------------------------------------------------------------------------------------------------
# the mask kernels, exactly
# ---------------------------------------------------------------------------------------------------
COUNTS = (1, 3, 4, 5, 1023, 1024, 1025, 4099)
STREAMS = (1, 2, 3, 0xFFFFFFFF)


@pytest.mark.parametrize("seed", SEEDS)
def test_flat_mask_equals_the_reference(pg, seed):  # noqa: F811
    from pygat_amd._lib import lib, check
    sd = _seed(seed)
    for p in (0.0, 0.1, 0.6, 1.0):
        for stream in STREAMS:
            for count in COUNTS:
                buf = _guarded(count)
                assert buf.data_ptr() % 16 == 0
                check(lib.pygat_dropout_mask(count, p, sd.data_ptr(), stream, buf.data_ptr(), None), "dropout_mask")
                ref = _t(R.flat_mask(seed, stream, count, p))
                assert torch.equal(buf[:count], ref), f"dropout_mask: seed {seed:#x} p {p} stream {stream:#x} count {count}"
                assert _guard_ok(buf, count), f"dropout_mask wrote behind element {count}"


def test_both_halves_of_the_seed_and_the_stream_id_take_part(pg):  # noqa: F811
    from pygat_amd._lib import lib, check
    n = 4099
    got = {}
    for seed, stream in ((SEED_LO, 2), (SEED_HI, 2), (SEED_HI, 3)):
        m = torch.empty(n, device=DEV)
        check(lib.pygat_dropout_mask(n, 0.6, _seed(seed).data_ptr(), stream, m.data_ptr(), None), "dropout_mask")
        got[seed, stream] = m
    assert not torch.equal(got[SEED_LO, 2], got[SEED_HI, 2])
    assert not torch.equal(got[SEED_HI, 2], got[SEED_HI, 3])


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("count1,count2", [(1, 1), (1023, 7), (1024, 1025), (4099, 4097), (5, 2051)])
def test_mask2_equals_the_reference_and_two_single_masks(pg, seed, count1, count2):  # noqa: F811
    """The second mask's counters start at 0 again, whatever padding the first mask's share of the launch has."""
    from pygat_amd._lib import lib, check
    sd = _seed(seed)
    for p in (0.1, 0.6):
        for s1, s2 in ((2, 3), (0xFFFFFFFF, 1)):
            b1, b2 = _guarded(count1), _guarded(count2)
            check(lib.pygat_dropout_mask2(p, sd.data_ptr(), count1, s1, b1.data_ptr(), count2, s2, b2.data_ptr(), None), "dropout_mask2")
            for buf, count, stream in ((b1, count1, s1), (b2, count2, s2)):
                assert torch.equal(buf[:count], _t(R.flat_mask(seed, stream, count, p))), f"mask2 ({count1}, {count2}) stream {stream:#x} p {p}"
                assert _guard_ok(buf, count), f"dropout_mask2 wrote behind element {count}"
                single = torch.empty(count, device=DEV)
                check(lib.pygat_dropout_mask(count, p, sd.data_ptr(), stream, single.data_ptr(), None), "dropout_mask")
                assert torch.equal(buf[:count], single)


@pytest.mark.parametrize("n,Fin", [(1, 1), (3, 5), (257, 37), (130, 128)])
def test_mask_bytes_equal_the_reference(pg, n, Fin):  # noqa: F811
    from pygat_amd._lib import lib, check
    for seed in SEEDS:
        sd = _seed(seed)
        for H in range(1, 9):
            for p in (0.1, 0.6):
                bits = torch.full((n * Fin + 4,), 0xA5, dtype=torch.uint8, device=DEV)
                check(lib.pygat_dropout_bits(n, Fin, H, p, sd.data_ptr(), 1, bits.data_ptr(), None), "dropout_bits")
                ref = _t(R.head_bits(seed, 1, n, Fin, H, p))
                assert torch.equal(bits[:n * Fin].view(n, Fin), ref), f"dropout_bits: seed {seed:#x} H {H} p {p}"
                assert int(bits[:n * Fin].max()) < (1 << H)                    # bits at and above H are zero
                assert bool((bits[n * Fin:] == 0xA5).all())


EXPAND_SHAPES = [(129, 37, 3), (3, 5, 2), (70, 300, 8), (5, 20, 9), (1, 1, 1)]    # H*Fin = 111, 10, 2400 (three chunks), 180, 1


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,Fin,H", EXPAND_SHAPES)
def test_expand_draws_the_wide_masks(pg, seed, n, Fin, H):  # noqa: F811
    """A'[i, h*Fin + k] = x[i,k] m_h[i,k] with the masks drawn in the kernel: x = 1 gives the masks themselves, a random x
    the exact fp32 products; ldo = H*Fin (vector stores where H*Fin is a multiple of 4) and ldo = H*Fin + 1 (scalar stores)."""
    from pygat_amd._lib import lib, check
    sd, HF, p = _seed(seed), H * Fin, 0.6
    M = _t(R.wide_mask(seed, 1, n, Fin, H, p)).permute(1, 0, 2).contiguous()       # [n, H, Fin]
    xr = torch.randn(n, Fin, generator=torch.Generator().manual_seed(n + Fin)).to(DEV)
    for x in (torch.ones(n, Fin, device=DEV), xr):
        want = (x[:, None, :] * M).view(n, HF)
        for ldo in (HF, HF + 1):
            out = torch.full((n, ldo), GUARD, device=DEV)
            check(lib.pygat_dropout_expand(n, Fin, H, x.data_ptr(), Fin, None, p, sd.data_ptr(), 1, out.data_ptr(), ldo, None),
                  "dropout_expand")
            assert torch.equal(out[:, :HF], want), f"dropout_expand ({n}, {Fin}, {H}) ldo {ldo}"
            assert bool((out[:, HF:] == GUARD).all())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n,Fin,H", EXPAND_SHAPES)
def test_head_sum_redraws_the_wide_masks(pg, seed, n, Fin, H):  # noqa: F811
    """dx[i,k] (+)= sum_h m_h[i,k] dxe[i, h*Fin + k]: the backward's re-draw of the forward's masks."""
    from pygat_amd._lib import lib, check
    sd, HF, p = _seed(seed), H * Fin, 0.6
    M = torch.as_tensor(R.wide_mask(seed, 1, n, Fin, H, p)).permute(1, 0, 2)       # [n, H, Fin]
    gen = torch.Generator().manual_seed(n * 7 + H)
    dxe = torch.randn(n, HF, generator=gen); base = torch.randn(n, Fin, generator=gen)
    dxe_d = dxe.to(DEV)
    ref64 = (M.double() * dxe.view(n, H, Fin).double()).sum(1)
    ref32 = (M * dxe.view(n, H, Fin)).sum(1)
    for accumulate in (0, 1):
        dx = base.to(DEV).clone() if accumulate else torch.full((n, Fin), float("nan"), device=DEV)
        check(lib.pygat_dropout_head_sum(n, Fin, H, dxe_d.data_ptr(), HF, None, p, sd.data_ptr(), 1, dx.data_ptr(), Fin, accumulate,
                                         None), "dropout_head_sum")
        r64 = ref64 + base.double() if accumulate else ref64
        r32 = (ref32 + base).double() if accumulate else ref32.double()
        close_grad(dx, r64, r32, f"dropout_head_sum ({n}, {Fin}, {H}) accumulate {accumulate}")


# ---------------------------------------------------------------------------------------------------
# sparse features: decisions drawn per non-zero from the seed = the same calls on the reference's bytes
# ---------------------------------------------------------------------------------------------------
def _sparse_x(n, fin, density, seed):
    """_features' rows (an empty row, a full row, an empty column) and a column every other row has (several segments)."""
    x = _features(n, fin, density, seed)
    x[:, 7] = torch.rand(n, generator=torch.Generator().manual_seed(seed + 1)) + 0.1
    x[3] = 0
    return x / x.sum(1, keepdim=True).clamp(min=1e-6)


@pytest.mark.parametrize("n,fin,H,Fo,skip", [(300, 129, 1, 7, False), (300, 150, 5, 8, True), (260, 300, 8, 8, False)])
def test_sparse_kernels_draw_the_reference_bytes(pg, n, fin, H, Fo, skip):  # noqa: F811
    """pygat_project_sparse / pygat_wgrad_sparse with a seed and bits = NULL against fp64 products under
    philox_ref.head_bits, and BITWISE against the same calls given those bytes and no seed: the two differ only in
    where a non-zero's keep nibble comes from (k9_sparse.hip sp_keep4), the walk, the summation order and the scale are
    the same code."""
    from pygat_amd._lib import lib, check
    from pygat_amd.features import SparseFeatures
    p, seed = 0.6, SEED_HI
    Fp = pg.padded_width(Fo); R_ = H * Fp
    x = _sparse_x(n, fin, 0.02, n + fin)
    assert float(x[3].abs().max()) == 0.0 and int((x[11] > 0).sum()) == fin - 1 and int((x[:, 7] > 0).sum()) == n - 1
    g = torch.Generator().manual_seed(H + Fo)
    W = torch.randn(H, fin, Fo, generator=g) * 0.3; a = torch.randn(H, 2 * Fo, generator=g) * 0.3
    Ws = torch.randn(H, fin, Fo, generator=g) * 0.3 if skip else None
    bits_np = R.head_bits(seed, 1, n, fin, H, p)
    bits = _t(bits_np)
    scale = float(R.threshold(p)[1])
    M = [torch.as_tensor(((bits_np >> h) & 1).astype(np.float32)) * scale for h in range(H)]
    xs = SparseFeatures(x.to(DEV))
    assert xs.nseg > fin
    ldw = -(-(R_ * (2 if skip else 1) + 2 * H) // 4) * 4
    Wcat = torch.empty(fin, ldw, device=DEV); a_pad = torch.empty(H, 2, Fp, device=DEV)
    Wd, ad, Wsd = W.to(DEV).contiguous(), a.to(DEV).contiguous(), (Ws.to(DEV).contiguous() if skip else None)
    check(lib.pygat_pack_params(H, fin, Fo, Wd.data_ptr(), ad.data_ptr(), Wsd.data_ptr() if skip else None, Wcat.data_ptr(), ldw,
                                a_pad.data_ptr(), None))
    dWh = torch.zeros(n, H, Fp); dWh[:, :, :Fo] = torch.randn(n, H, Fo, generator=g)
    RW = R_ + 4 * H
    GR = torch.randn(n, RW, generator=g)
    dWh_d, GR_d = dWh.view(n, R_).to(DEV).contiguous(), GR.to(DEV).contiguous()
    sd = _seed(seed)

    def run(seed_ptr, bits_ptr):
        nan = float("nan")
        Wh = torch.full((n, R_), nan, device=DEV); Sk = torch.full((n, R_), nan, device=DEV) if skip else None
        check(lib.pygat_project_sparse(n, fin, H, Fo, xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(), Wcat.data_ptr(), ldw,
                                       p, seed_ptr, 1, bits_ptr, Wh.data_ptr(), Sk.data_ptr() if skip else None, None, None),
              "project_sparse")
        dW = torch.full((H, fin, Fo), nan, device=DEV); dWs = torch.full((H, fin, Fo), nan, device=DEV) if skip else None
        wss = torch.empty(lib.pygat_wgrad_sparse_workspace_bytes(xs.nseg, H, Fo, int(skip)) // 4 + 4, device=DEV)
        check(lib.pygat_wgrad_sparse(n, fin, H, Fo, xs.nseg, xs.colseg.data_ptr(), xs.seg_col.data_ptr(), xs.seg_begin.data_ptr(),
                                     xs.seg_end.data_ptr(), xs.trow.data_ptr(), xs.tval.data_ptr(), p, seed_ptr, 1, bits_ptr,
                                     dWh_d.data_ptr(), GR_d.data_ptr() if skip else None, RW, wss.data_ptr(), dW.data_ptr(),
                                     dWs.data_ptr() if skip else None, None), "wgrad_sparse")
        torch.cuda.synchronize()
        return Wh, Sk, dW, dWs

    seeded = run(sd.data_ptr(), None)
    given = run(None, bits.data_ptr())
    Wh, Sk, dW, dWs = seeded
    for h in range(H):
        xm = x * M[h]
        close_grad(Wh.view(n, H, Fp)[:, h, :Fo], xm.double() @ W[h].double(), (xm @ W[h]).double(), f"seeded Wh head {h}")
        assert Fp == Fo or float(Wh.view(n, H, Fp)[:, h, Fo:].abs().max()) == 0.0
        d = dWh[:, h, :Fo]
        close_grad(dW[h], xm.double().t() @ d.double(), (xm.t() @ d).double(), f"seeded dW head {h}")
        if skip:
            close_grad(Sk.view(n, H, Fp)[:, h, :Fo], xm.double() @ Ws[h].double(), (xm @ Ws[h]).double(), f"seeded Sk head {h}")
            gph = GR[:, h * Fp:h * Fp + Fo]
            close_grad(dWs[h], xm.double().t() @ gph.double(), (xm.t() @ gph).double(), f"seeded dWskip head {h}")
    for name, s_, g_ in zip(("Wh", "Sk", "dW", "dWskip"), seeded, given):
        assert (s_ is None and g_ is None) or torch.equal(s_, g_), f"{name}: a seed and its reference bytes give different bits"


# ---------------------------------------------------------------------------------------------------
# the seeded LEVEL against the oracle under the reference generator's masks
# ---------------------------------------------------------------------------------------------------
N_LEVEL, ALPHA = 300, 0.2      # three 128-row GEMM tiles, the last one ragged


@functools.lru_cache(maxsize=None)
def _level_graph():
    """Hub rows cut by many slot borders (slot_edges = 16), most rows with several edges: the order of the attention
    mask along a row matters."""
    rowptr, col = O.random_symmetric_csr(N_LEVEL, 5, 3, hub=(2, 200))
    assert int(np.diff(rowptr).max()) >= 200 and float((np.diff(rowptr) > 1).mean()) > 0.9
    return rowptr, col


#                 H  Fin  Fo  skip  concat  path      data seed
CASES = {
    "mfma8":    (8, 200, 8, False, True, "mfma", 4),
    "mfma4":    (4, 150, 16, True, False, "mfma", 6),
    "narrow1":  (1, 64, 7, False, False, "narrow", 4),
    "narrow8":  (8, 64, 3, False, True, "narrow", 7),
    "wide9":    (9, 20, 8, True, True, "wide", 4),                # H > 8
    "windows":  (3, 9, 128, True, True, "wide", 4),               # rows of 384 floats, backward in head windows of 256
    "forced":   (8, 200, 8, False, True, "wide", 5),              # FORCE_WIDE
    "sparse8":  (8, 300, 8, False, True, "sparse", 4),
    "sparse4":  (4, 129, 16, True, False, "sparse", 6),
    "sparse8x16s": (8, 200, 16, True, True, "sparse", 9),         # 256 masked columns: four per lane (k9_sparse.hip)
    "sparse8x32s": (8, 200, 32, True, True, "sparse", 5),         # 512 masked columns: eight per lane
}
DATA_SEED = {("mfma8", 0.1): 5}       # where a case's seed puts a logit near the kink at another dropout rate
RUNS = ([(name, 0.6, None) for name in CASES] + [("mfma8", 0.1, None), ("wide9", 0.1, None)]
        + [(name, 0.6, fl) for name in ("mfma8", "wide9") for fl in ("rowlocal", "rowsum", "two-gather")])


def _level_case(name, p, seed):
    """Inputs (fp64, CPU), the reference generator's masks for `seed` and the oracle closure of one case."""
    H, Fin, Fo, skip, concat, path, data_seed = CASES[name]
    data_seed = DATA_SEED.get((name, p), data_seed)
    rowptr, col = _level_graph()
    E = len(col)
    W, a, Sk = params(H, Fin, Fo, skip, data_seed)
    gen = torch.Generator().manual_seed(data_seed + 1)
    if path == "sparse":
        x = _sparse_x(N_LEVEL, Fin, 0.03, data_seed).double()
    else:
        x = torch.randn(N_LEVEL, Fin, dtype=torch.float64, generator=gen)
    G = torch.randn(N_LEVEL, H * Fo if concat else Fo, dtype=torch.float64, generator=gen)
    import pygat_amd
    mk = R.level_masks(seed, p, H, N_LEVEL, Fin, Fo, pygat_amd.padded_width(Fo), E, "wide" if path == "wide" else "bits")
    mx, mwh, matt = (torch.as_tensor(mk[k]).double() for k in ("x", "wh", "att"))
    leaves = [x, W, a] + ([Sk] if skip else [])

    def oracle(*lv):       # (the att mask is [H, E] in the oracle)
        m = dict(x=mx.to(lv[0].dtype), wh=mwh.to(lv[0].dtype), att=matt.t().contiguous().to(lv[0].dtype))
        return O.level_forward(lv[0], (rowptr, col), lv[1], lv[2], ALPHA, concat, lv[3] if skip else None, "sparse", m)
    return dict(x=x, W=W, a=a, Sk=Sk, G=G, leaves=leaves, oracle=oracle, masks=(mx, mwh, matt), graph=(rowptr, col))


def _kink_margin(c):
    """min |z| / (|s_i| + |t_j|) over the edges and heads of the fp64 oracle under the case's masks (a
    logit within 8e-6 of that scale takes either LeakyReLU branch in fp32).  Edges with |s_i| + |t_j| = 0 are left out:
    both Wh rows are dropped whole there, z is an exact 0 in every precision (a sum of products with 0), and nothing flows
    back through s_i or t_j (the Wh mask zeroes that gradient)."""
    rowptr, col = c["graph"]
    src = np.repeat(np.arange(N_LEVEL), np.diff(rowptr))
    mx, mwh, _ = c["masks"]
    H, _, Fo = c["W"].shape
    best = float("inf")
    for h in range(H):
        Wh = ((c["x"] * mx[h]) @ c["W"][h]) * mwh[h]
        s, t = (Wh @ c["a"][h, :Fo]).numpy(), (Wh @ c["a"][h, Fo:]).numpy()
        z, sc = s[src] + t[col], np.abs(s[src]) + np.abs(t[col])
        live = sc > 0
        best = min(best, float((np.abs(z[live]) / sc[live]).min()))
    return best


@pytest.mark.parametrize("name,p,flavour", RUNS, ids=[f"{n}-p{p}-{f or 'default'}" for n, p, f in RUNS])
def test_seeded_level_equals_the_oracle_under_the_reference_masks(pg, monkeypatch, name, p, flavour):  # noqa: F811
    """check_autograd has no LeakyReLU-kink treatment, so every case's data seed keeps all logits out of the rounding band
    (asserted below; on a trip change the data seed, not the rule)."""
    from pygat_amd import dropout as D
    from pygat_amd._lib import lib
    from pygat_amd.features import SparseFeatures
    H, Fin, Fo, skip, concat, path, _ = CASES[name]
    c = _level_case(name, p, SEED_HI)
    margin = _kink_margin(c)
    assert margin > KINK_TAU, f"{name}: an edge at {margin:.2e} of the LeakyReLU kink: pick another data seed"
    monkeypatch.setattr(D, "FORCE_WIDE", name == "forced")
    monkeypatch.setattr(pg.ops, "TWO_GATHER_BACKWARD", None)
    monkeypatch.setattr(pg.ops, "BACKWARD_FLAVOUR", flavour)
    monkeypatch.setattr(pg.ops, "BWD_WINDOW_FLOATS", 256 if name == "windows" else None)
    rowptr, col = c["graph"]
    g = pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV), slot_edges=16)
    sparse = path == "sparse"
    xd = c["x"].float().to(DEV).requires_grad_(not sparse)
    Wd = c["W"].float().to(DEV).requires_grad_(True)
    ad = c["a"].float().to(DEV).requires_grad_(True)
    Sd = c["Sk"].float().to(DEV).requires_grad_(True) if skip else None
    xs = SparseFeatures(xd) if sparse else None
    if sparse:
        assert 0.02 < xs.density < 0.05
    out = D.GATLevelDropoutFn.apply(xd, Wd, ad, Sd, g, ALPHA, concat, p, None, None, None, _seed(SEED_HI), xs)
    # which path ran: a change of the dispatch must not silently empty a case
    ctx = out.grad_fn
    narrow = bool(lib.pygat_dropout_narrow(Fin, H, Fo, int(skip)))
    assert ctx.use_bits == (path != "wide")
    assert (ctx.xs is not None) == sparse
    assert narrow == (path == "narrow")
    assert ctx.flavour == (flavour or ("rowlocal" if ctx.L.R <= 256 else "rowsum"))
    if name == "windows":
        assert ctx.L.hg < H
    out.backward(c["G"].float().to(DEV))
    assert (xd.grad is None) == sparse                               # no dX on the sparse-feature path
    got = [xd.grad, Wd.grad, ad.grad] + ([Sd.grad] if skip else [])
    check_autograd(out, got, c["oracle"], c["leaves"], c["G"], ["dX", "dW", "da", "dW_skip"],
                   what=f"seeded dropout {name} p={p} {flavour or 'default'}")


def test_layer_in_train_mode_draws_the_seed_the_level_is_given(pg):  # noqa: F811
    """The public layer takes its mask seed from torch's generator with randint(0, 2**62) on the device: the same draw, made
    by hand after the same manual_seed, handed to the level directly gives the same output bit for bit."""
    from pygat_amd import dropout as D
    Fin, Fo, p = 64, 7, 0.6
    rowptr, col = _level_graph()
    g = pg.CSRGraph(torch.as_tensor(rowptr, device=DEV), torch.as_tensor(col, device=DEV), slot_edges=16)
    torch.manual_seed(3)
    layer = pg.SpGraphAttentionLayer(Fin, Fo, p, ALPHA, concat=False).to(DEV).train()
    x = torch.randn(N_LEVEL, Fin, generator=torch.Generator().manual_seed(9)).to(DEV)
    torch.manual_seed(77)
    seed = torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=DEV)
    assert int(seed) >> 32 != 0
    torch.manual_seed(77)
    y = layer(x, g)
    direct = D.GATLevelDropoutFn.apply(x, layer.W.detach()[None], layer.a.detach().reshape(1, -1), None, g, ALPHA, False, p,
                                       None, None, None, seed, None)
    assert y.grad_fn.use_bits and y.grad_fn.xs is None
    assert torch.equal(y.detach(), direct)
    other = D.GATLevelDropoutFn.apply(x, layer.W.detach()[None], layer.a.detach().reshape(1, -1), None, g, ALPHA, False, p,
                                      None, None, None, seed + (1 << 32), None)
    assert not torch.equal(direct, other)
