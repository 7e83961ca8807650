"""The parity rule of tests/parity.py, checked on the CPU against the oracle itself: it accepts the fp32 run of the
oracle, accepts a LeakyReLU branch flip at an edge whose logit sits inside the rounding band of the kink (and reports
it), and REJECTS the same flip anywhere else -- i.e. the flip-aware comparison cannot explain away a kernel that takes
the wrong branch at an ordinary edge."""
import numpy as np
import pytest
import torch

import parity
from oracle import gat_oracle as O


def _case(seed=0, N=60, H=3, Fin=12, Fo=8):
    rng = np.random.default_rng(seed)
    rowptr, col = O.random_symmetric_csr(N, 5, seed, hub=(1, 30))
    X = rng.standard_normal((N, Fin)); W = rng.standard_normal((H, Fin, Fo)) * 0.4
    a = rng.standard_normal((H, 2 * Fo)) * 0.4
    G = rng.standard_normal((N, H * Fo))
    return X, rowptr, col, W, a, G


def _as_got(r):
    return {"dX": r["dX"], "dW": r["dW"], "da": r["da"]}


def _put_edge_on_the_kink(X, rowptr, col, W, a, h, e, eps):
    """Shift a_src of head h along Wh_i so that the logit of edge e becomes eps * (|s| + |t|)."""
    Fo = W.shape[2]
    i = int(np.searchsorted(rowptr, e, side="right") - 1); j = int(col[e])
    whi, whj = X[i] @ W[h], X[j] @ W[h]
    for _ in range(30):
        s, t = whi @ a[h, :Fo], whj @ a[h, Fo:]
        want = eps * (abs(s) + abs(t))
        a[h, :Fo] += (want - (s + t)) * whi / (whi @ whi)
    return a


def test_fp32_oracle_passes_and_reports_no_flip_without_kinks():
    X, rowptr, col, W, a, G = _case()
    r32 = O.csr_layer_fwd_bwd(X.astype(np.float32), rowptr, col, W.astype(np.float32), a.astype(np.float32), 0.2, True,
                              G.astype(np.float32))
    rep = parity.check_level(r32["out"], _as_got(r32), X, rowptr, col, W, a, 0.2, True, G, what="fp32 oracle", verbose=False)
    assert rep["candidates"] == 0 and rep["hip_flips"] == []


def test_flip_inside_the_band_is_explained_and_counted():
    X, rowptr, col, W, a, G = _case(1)
    h, e = 1, 37
    a = _put_edge_on_the_kink(X, rowptr, col, W, a, h, e, 1e-7)
    flips = np.zeros((W.shape[0], len(col)), dtype=bool); flips[h, e] = True
    other = O.csr_layer_fwd_bwd(X, rowptr, col, W, a, 0.2, True, G, flips=flips)       # fp64, other branch at that edge
    rep = parity.check_level(other["out"], _as_got(other), X, rowptr, col, W, a, 0.2, True, G, what="in-band flip", verbose=False)
    assert rep["hip_flips"] == [(h, e)] and rep["candidates"] >= 1
    assert max(rep["hip"].values()) < 1e-6           # nothing but the flip (and (1 - alpha)|z| ~ 1e-7 in the forward) separates the two fp64 runs


def test_flip_outside_the_band_is_rejected():
    X, rowptr, col, W, a, G = _case(2)
    ref = O.csr_layer_fwd_bwd(X, rowptr, col, W, a, 0.2, True, G)
    rel = np.abs(ref["z"]) / ref["zscale"]
    # an ordinary edge with a sizeable gradient through it: far from the kink
    score = np.where(rel > 100 * parity.KINK_TAU, np.abs(ref["de"]), 0.0)
    h, e = np.unravel_index(np.argmax(score), score.shape)
    flips = np.zeros_like(rel, dtype=bool); flips[h, e] = True
    wrong = O.csr_layer_fwd_bwd(X, rowptr, col, W, a, 0.2, True, G, flips=flips)
    assert max(np.abs(wrong[n] - ref[n]).max() for n in ("dX", "dW", "da")) > 1e-4     # the flip is visible ...
    with pytest.raises(AssertionError):                                               # ... and nothing may explain it away
        parity.check_level(wrong["out"], _as_got(wrong), X, rowptr, col, W, a, 0.2, True, G, what="wrong branch", verbose=False)


def test_too_many_flips_are_rejected(monkeypatch):
    """The leash on the count: more than FLIP_FACTOR x the fp32 oracle's flips + FLIP_SLACK in-band flips fail."""
    X, rowptr, col, W, a, G = _case(3, H=1)
    monkeypatch.setattr(parity, "FLIP_SLACK", 1)
    monkeypatch.setattr(parity, "FLIP_FACTOR", 0)      # (the fp32 oracle run inside the rule may flip at these edges too)
    edges = [5, 50, 90]
    flips = np.zeros((1, len(col)), dtype=bool)
    # three edges of different rows / columns put on the kink one after another (each fix leaves the earlier ones
    # within the band: the shifts are along different Wh rows and tiny)
    for _ in range(200):
        for e in edges:
            a = _put_edge_on_the_kink(X, rowptr, col, W, a, 0, e, 1e-8)
    ref = O.csr_layer_fwd_bwd(X, rowptr, col, W, a, 0.2, True, G)
    rel = np.abs(ref["z"]) / ref["zscale"]
    inband = [e for e in edges if rel[0, e] <= parity.KINK_TAU]
    if len(inband) < 2:
        pytest.skip("could not put two edges on the kink at once for this seed")
    flips[0, inband] = True
    other = O.csr_layer_fwd_bwd(X, rowptr, col, W, a, 0.2, True, G, flips=flips)
    with pytest.raises(AssertionError, match="other LeakyReLU branch"):
        parity.check_level(other["out"], _as_got(other), X, rowptr, col, W, a, 0.2, True, G, what="flip count", verbose=False)


# ---------------------------------------------------------------------------------------------------------------------------
# The GATv2 rule (parity.close_level_grads_v2): kinks per (edge, head, feature)
def _case_v2(seed=0, N=60, H=3, Fin=12, Fo=8, skip=False, hub=(1, 30)):
    rng = np.random.default_rng(seed)
    rowptr, col = O.random_symmetric_csr(N, 5, seed, hub=hub)
    X = rng.standard_normal((N, Fin))
    W = rng.standard_normal((H, 2 * Fin, Fo)) * (1.414 * (2.0 / (2 * Fin + Fo)) ** 0.5)
    a = rng.standard_normal((H, Fo)) * (1.414 * (2.0 / (1 + Fo)) ** 0.5)
    Sk = rng.standard_normal((H, Fin, Fo)) * 0.3 if skip else None
    G = rng.standard_normal((N, H * Fo))
    return X, rowptr, col, W, a, Sk, G


def _v2_forced(X, rowptr, col, W, a, alpha, concat, G, Sk=None, force=(), dtype=torch.float32, bug=None):
    """A GATv2 level written out by hand (numpy, `dtype`): forward and backward, independent of the autograd oracle.
    force: (h, e, f) triples whose LeakyReLU branch is the OTHER one than the fp64 logit's sign (an injected flip).
    bug: a plausible kernel bug -- "agg_whj" (aggregate Whj at the neighbour), "no_D" (de without D_i), "col_slope" (the
    slope taken on the wrong side of the kink in the dWhj column sums only)."""
    dt = np.float32 if dtype == torch.float32 else np.float64
    X64 = np.asarray(X, np.float64); W64 = np.asarray(W, np.float64)
    X_, W_, a_, G_ = (np.asarray(v, np.float64).astype(dt) for v in (X, W, a, G))
    Sk_ = None if Sk is None else np.asarray(Sk, np.float64).astype(dt)
    rowptr = np.asarray(rowptr, np.int64); col = np.asarray(col, np.int64)
    N, Fin = X_.shape; H, _, Fo = W_.shape
    src = np.repeat(np.arange(N), np.diff(rowptr))
    outs, dX, dW, da = [], np.zeros_like(X_), np.zeros_like(W_), np.zeros_like(a_)
    dSk = None if Sk is None else np.zeros_like(Sk_)
    for h in range(H):
        Whi, Whj = X_ @ W_[h, :Fin], X_ @ W_[h, Fin:]
        z = Whi[src] + Whj[col]
        pos = z > 0
        z64 = (X64 @ W64[h, :Fin])[src] + (X64 @ W64[h, Fin:])[col]
        for (hh, e, f) in force:
            if hh == h:
                pos[e, f] = not (z64[e, f] > 0)
        lr = np.where(pos, z, dt(alpha) * z)
        ev = lr @ a_[h]
        m = np.full(N, -np.inf, dt); np.maximum.at(m, src, ev)
        p = np.exp(ev - m[src])
        Z = np.zeros(N, dt); np.add.at(Z, src, p)
        al = p / Z[src]
        V = Whj if bug == "agg_whj" else Whi
        hp = np.zeros((N, Fo), dt); np.add.at(hp, src, al[:, None] * V[col])
        pre = hp if Sk_ is None else hp + X_ @ Sk_[h]
        out = np.where(pre > 0, pre, np.expm1(np.minimum(pre, 0))) if concat else pre
        outs.append(out)
        Gh = G_[:, h * Fo:(h + 1) * Fo] if concat else G_ / dt(H)
        Gp = Gh * np.where(pre > 0, 1.0, np.exp(np.minimum(pre, 0))).astype(dt) if concat else Gh
        dp = np.einsum("ef,ef->e", Gp[src], V[col])
        D = np.zeros(N, dt); np.add.at(D, src, al * dp)
        de = al * (dp - (0 if bug == "no_D" else D[src]))
        slope = np.where(pos, dt(1), dt(alpha))
        q = de[:, None] * a_[h][None, :] * slope
        qc = de[:, None] * a_[h][None, :] * (np.where(pos, dt(alpha), dt(1)) if bug == "col_slope" else slope)
        dWhi = np.zeros((N, Fo), dt); dWhj = np.zeros((N, Fo), dt)
        np.add.at(dWhi if bug != "agg_whj" else dWhj, col, al[:, None] * Gp[src])
        np.add.at(dWhi, src, q)
        np.add.at(dWhj, col, qc)
        da[h] = de @ lr
        dW[h, :Fin] = X_.T @ dWhi; dW[h, Fin:] = X_.T @ dWhj
        dX += dWhi @ W_[h, :Fin].T + dWhj @ W_[h, Fin:].T
        if Sk_ is not None:
            dSk[h] = X_.T @ Gp
            dX += Gp @ Sk_[h].T
    out = np.concatenate(outs, 1) if concat else np.mean(np.stack(outs, 1), 1)
    return dict(out=out, dX=dX, dW=dW, da=da, dW_skip=dSk)


def _put_feature_on_the_kink(X, rowptr, col, W, h, e, f, eps):
    """Shift column f of W_h's left half along X_i so that z_ijf = Whi_i[f] + Whj_j[f] becomes eps * (|Whi| + |Whj|)."""
    Fin = X.shape[1]
    i = int(np.searchsorted(rowptr, e, side="right") - 1); j = int(col[e])
    for _ in range(30):
        wi, wj = X[i] @ W[h, :Fin, f], X[j] @ W[h, Fin:, f]
        want = eps * (abs(wi) + abs(wj))
        W[h, :Fin, f] += (want - (wi + wj)) * X[i] / (X[i] @ X[i])
    return W


def _got(r, skip=False):
    g = {"dX": r["dX"], "dW": r["dW"], "da": r["da"]}
    if skip:
        g["dW_skip"] = r["dW_skip"]
    return g


@pytest.mark.parametrize("N,H,Fin,Fo,skip,concat", [(300, 4, 32, 256, False, True),     # R = 1024: 4 heads x 256
                                                    (200, 3, 24, 100, True, False)])     # F' = 100 (padded to 128), mean, skip
def test_v2_fp32_oracle_passes(N, H, Fin, Fo, skip, concat):
    X, rowptr, col, W, a, Sk, G = _case_v2(4, N, H, Fin, Fo, skip, hub=(3, min(N - 1, 150)))
    if not concat:
        G = G[:, :Fo]
    r32 = parity.v2_oracle(X.astype(np.float32), rowptr, col, W.astype(np.float32), a.astype(np.float32), 0.2, concat,
                           G.astype(np.float32), None if Sk is None else Sk.astype(np.float32), dtype=torch.float32)
    rep = parity.check_level_v2(r32["out"], _got(r32, skip), X, rowptr, col, W, a, 0.2, concat, G, Sk, what=f"fp32 oracle v2 {H}x{Fo}")
    print(f"flips reported (h, e, f): as the HIP side {rep['hip_flips']}, fp32 oracle {rep['fp32_flips']}; "
          f"{rep['candidates']} in-band candidates")
    # the hand-written level agrees as well (the mutants below are edits of it)
    hand = _v2_forced(X, rowptr, col, W, a, 0.2, concat, G, Sk)
    parity.check_level_v2(hand["out"], _got(hand, skip), X, rowptr, col, W, a, 0.2, concat, G, Sk, what="hand-written v2", verbose=False)


def test_v2_flip_inside_the_band_is_explained_and_reported():
    X, rowptr, col, W, a, Sk, G = _case_v2(5)
    # an edge with a sizeable de, one of its features with a sizeable a_f
    k0 = parity.v2_kinks(X, rowptr, col, W, a, 0.2, True, G, tau=np.inf, cap=10 ** 9)
    score = np.abs(k0["de"] * a[k0["h"], k0["f"]])
    q = int(np.argmax(score))
    h, e, f = int(k0["h"][q]), int(k0["e"][q]), int(k0["f"][q])
    W = _put_feature_on_the_kink(X, rowptr, col, W, h, e, f, 1e-7)
    got = _v2_forced(X, rowptr, col, W, a, 0.2, True, G, force=[(h, e, f)])
    rep = parity.check_level_v2(got["out"], _got(got), X, rowptr, col, W, a, 0.2, True, G, what="in-band v2 flip", verbose=False)
    assert (h, e, f) in rep["hip_flips"] and rep["candidates"] >= 1
    assert rep["hip_raw"]["dW"] > 100 * rep["hip"]["dW"]        # the flip was visible and is what got explained


def test_v2_flip_outside_the_band_is_rejected():
    X, rowptr, col, W, a, Sk, G = _case_v2(6)
    k0 = parity.v2_kinks(X, rowptr, col, W, a, 0.2, True, G, tau=np.inf, cap=10 ** 9)
    score = np.where(k0["rel"] > 100 * parity.KINK_TAU, np.abs(k0["de"] * a[k0["h"], k0["f"]]), 0.0)
    q = int(np.argmax(score))
    h, e, f = int(k0["h"][q]), int(k0["e"][q]), int(k0["f"][q])
    got = _v2_forced(X, rowptr, col, W, a, 0.2, True, G, force=[(h, e, f)])
    ref = parity.v2_oracle(X, rowptr, col, W, a, 0.2, True, G)
    assert max(np.abs(got[n] - ref[n]).max() for n in ("dX", "dW", "da")) > 1e-4      # the flip is visible ...
    with pytest.raises(AssertionError):                                               # ... and nothing may explain it away
        parity.check_level_v2(got["out"], _got(got), X, rowptr, col, W, a, 0.2, True, G, what="wrong v2 branch", verbose=False)


@pytest.mark.parametrize("bug", ["agg_whj", "no_D", "col_slope"])
@pytest.mark.parametrize("concat", [True, False])
def test_v2_plausible_kernel_bugs_fail(bug, concat):
    X, rowptr, col, W, a, Sk, G = _case_v2(7, N=80, H=2, Fin=16, Fo=12, skip=not concat)
    if not concat:
        G = G[:, :12]
    got = _v2_forced(X, rowptr, col, W, a, 0.2, concat, G, Sk, bug=bug)
    with pytest.raises(AssertionError) as exc:
        parity.check_level_v2(got["out"], _got(got, Sk is not None), X, rowptr, col, W, a, 0.2, concat, G, Sk,
                              what=f"v2 bug {bug}", verbose=False)
    print(f"{bug}: {str(exc.value).splitlines()[0]}")
