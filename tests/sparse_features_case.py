"""Ground truth, inputs and the case table of the tests of the sparse-feature kernels (pygat_amd/features.py,
csrc/k9_sparse.hip): plain NumPy / torch on the CPU, no GPU.

`sparse_ref` restates in plain loops what SparseFeatures must hold.  `rows_matrix` / `cols_matrix` put a row / a feature
column of every length at which the walk of k9_sparse.hip changes shape: one short of, at and one past a batch of 8, 16, 32
or 64 pairs and a 128-entry segment.  Two value flavours: "norm" (row-normalised floats, the datasets' kind, priced by
parity.close_grad unchanged) and "exact" (small integers everywhere, p = 0.5 so that the threshold is 2^31 and the scale
exactly 2: every partial sum stays below 2^24, any summation order is exact in fp32, and the device has to return the
fp64 result bit for bit -- one wrong keep bit or one lost entry fails, whatever its size).

A case is (matrix kind, H, Fo, skip, with_s, mask kind); its classes -- columns per lane of the forward and the backward
dispatch, hq_shift, padded heads -- are restated here by formula, and `check_grid` asserts the table covers the grid the
tests promise.  tests/test_sparse_features_abi.py rehearses every case with the fp32 CPU product standing in for the
device; the case-table tests of tests/test_gpu_sparse_features.py run them on the device and build no case of their own."""
import functools

import numpy as np
import torch

import philox_ref as R
from parity import close_grad

SEGMENT = 128            # features.py SEGMENT, k9_sparse.hip SP_SEG
MAX_COLUMNS = 512        # features.py MAX_COLUMNS = 64 lanes x 8 columns
N, FIN = 323, 261        # a full row: four batches of 64 and 5 pairs; a full column: two segments of 128 and 67 entries
ROW_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, FIN)
COL_COUNTS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, N)
SEED = 0x2F00_0000_0000_0000 + 777      # a non-zero high half, as the model's randint(0, 2**62) draws
STREAM = 2
P = {"norm": 0.6, "exact": 0.5}
FLAVOURS = ("norm", "exact")
LIMIT = float(1 << 24)


def padded_width(Fo):
    """pygat_padded_width: 4, 8, 16, ... 256 (tests/test_abi.py pins the library's to the same values)."""
    w = 4
    while w < Fo:
        w *= 2
    return w


# ---------------------------------------------------------------------------------------------------
# what SparseFeatures must hold
# ---------------------------------------------------------------------------------------------------
def sparse_ref(x):
    """x [n, fin] (anything np.asarray takes) -> dict of int32 / float32 arrays and nseg.  Entries in row-major order
    (rowptr, col, val); the transpose with columns ascending and rows ascending inside a column (trow, tval); every
    column cut into segments of at most SEGMENT entries, at least one (empty) segment per column (colseg, seg_col,
    seg_begin, seg_end index trow / tval)."""
    rows = np.asarray(x, dtype=np.float32).tolist()
    n, fin = len(rows), len(rows[0])
    rowptr, col, val = [0], [], []
    for i in range(n):
        for k in range(fin):
            if rows[i][k] != 0:
                col.append(k); val.append(rows[i][k])
        rowptr.append(len(col))
    trow, tval, colseg, seg_col, seg_begin, seg_end = [], [], [0], [], [], []
    for k in range(fin):
        begin = len(trow)
        for i in range(n):
            if rows[i][k] != 0:
                trow.append(i); tval.append(rows[i][k])
        end = len(trow)
        while True:
            seg_col.append(k); seg_begin.append(begin); seg_end.append(min(begin + SEGMENT, end))
            begin += SEGMENT
            if begin >= end:
                break
        colseg.append(len(seg_col))
    i32 = lambda v: np.asarray(v, dtype=np.int32)  # noqa: E731
    f32 = lambda v: np.asarray(v, dtype=np.float32)  # noqa: E731
    return dict(rowptr=i32(rowptr), col=i32(col), val=f32(val), trow=i32(trow), tval=f32(tval), colseg=i32(colseg),
                seg_col=i32(seg_col), seg_begin=i32(seg_begin), seg_end=i32(seg_end), nseg=len(seg_col))


STRUCTURE_ARRAYS = ("rowptr", "col", "val", "trow", "tval", "colseg", "seg_col", "seg_begin", "seg_end")


# ---------------------------------------------------------------------------------------------------
# matrices with prescribed row / column lengths
# ---------------------------------------------------------------------------------------------------
def _background(n, fin, rng):
    """Every row at a density of its own between 2 and 3 %, random columns."""
    return rng.random((n, fin)) < rng.uniform(0.02, 0.03, size=(n, 1))


def rows_matrix(n, fin, seed):
    """bool [n, fin]: ROW_COUNTS-long rows (`fin` for the full one) at random places, the rest at 2-3 %.
    -> (pattern, {count: row})."""
    rng = np.random.default_rng(seed)
    pat = _background(n, fin, rng)
    counts = sorted({min(c, fin) for c in ROW_COUNTS[:-1]} | {fin})
    where = rng.permutation(n)[:len(counts)]
    for c, i in zip(counts, where):
        pat[i] = False
        pat[i, rng.permutation(fin)[:c]] = True
    return pat, {c: int(i) for c, i in zip(counts, where)}


def cols_matrix(n, fin, seed):
    """The same for feature columns: COL_COUNTS-long columns (`n` for the full one).  -> (pattern, {count: column})."""
    rng = np.random.default_rng(seed)
    pat = _background(n, fin, rng)
    counts = sorted({min(c, n) for c in COL_COUNTS[:-1]} | {n})
    where = rng.permutation(fin)[:len(counts)]
    for c, k in zip(counts, where):
        pat[:, k] = False
        pat[rng.permutation(n)[:c], k] = True
    return pat, {c: int(k) for c, k in zip(counts, where)}


KINDS = {"rows": (rows_matrix, 11), "cols": (cols_matrix, 12)}


@functools.lru_cache(maxsize=None)
def matrix(kind, flavour):
    """float32 torch [N, FIN] of one kind and value flavour (shared, never written to)."""
    build, seed = KINDS[kind]
    pat, where = build(N, FIN, seed)
    counts = pat.sum(1) if kind == "rows" else pat.sum(0)
    for c, at in where.items():
        assert counts[at] == c, (kind, c, at)
    rng = np.random.default_rng(seed + 100)
    if flavour == "exact":
        x = torch.as_tensor(pat * rng.integers(1, 4, size=pat.shape)).float()
    else:
        x = torch.as_tensor(pat * (rng.random(pat.shape) + 0.1)).float()
        x = x / x.sum(1, keepdim=True).clamp(min=1e-6)
    assert bool(((x != 0) == torch.as_tensor(pat)).all())
    return x


@functools.lru_cache(maxsize=None)
def seeded_keep(p):
    """bool [32, N, FIN]: philox_ref's decisions of every head the kernels can draw (head h does not depend on H)."""
    return R.head_keep(SEED, STREAM, N, FIN, 32, p)


@functools.lru_cache(maxsize=None)
def seeded_bits(H, p):
    return R.head_bits(SEED, STREAM, N, FIN, H, p)


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
def _dispatch(ncols):
    """PYGAT_SP_DISPATCH_M: the columns-per-lane instantiation that takes `ncols` output columns."""
    assert 0 < ncols <= MAX_COLUMNS, f"{ncols} output columns: the sparse kernels take {MAX_COLUMNS}"
    per_lane = -(-ncols // 64)
    return next(c for c in (1, 2, 4, 8) if per_lane <= c)


class Case:
    """One case of the table in one value flavour.  `inputs()` are the CPU tensors the device is fed (fp32), `refs()` the
    fp64 products and the same products formed in fp32 on the CPU, in the device's layouts; `price(got)` prices a run."""

    def __init__(self, kind, H, Fo, skip, with_s, mask, flavour):
        assert kind in KINDS and mask in ("none", "bytes", "seed") and flavour in FLAVOURS
        assert not (with_s and mask != "none"), "the score columns are not formed under dropout"
        assert mask != "bytes" or H <= 8, "a byte holds 8 heads"
        self.kind, self.H, self.Fo, self.skip, self.with_s, self.mask, self.flavour = kind, H, Fo, skip, with_s, mask, flavour
        self.Fp = padded_width(Fo)
        self.R = H * self.Fp
        self.ncols_bwd = self.R * (2 if skip else 1)
        self.ncols_fwd = self.ncols_bwd + (H if with_s else 0)
        self.cpl_fwd, self.cpl_bwd = _dispatch(self.ncols_fwd), _dispatch(self.ncols_bwd)
        self.hq_shift = None
        if mask != "none":
            self.hq_shift = 0
            while (4 << self.hq_shift) < H:
                self.hq_shift += 1
        self.padded = self.Fp > Fo
        self.p = P[flavour] if mask != "none" else 0.0
        self.scale = float(R.threshold(self.p)[1])
        self.name = f"{kind}-{H}x{Fo}{'-skip' if skip else ''}{'-s' if with_s else ''}-{mask}-{flavour}"

    # -- inputs ------------------------------------------------------------------------------------
    def keep(self):
        """bool [H, N, FIN] or None."""
        if self.mask == "none":
            return None
        if self.mask == "seed":
            return seeded_keep(self.p)[:self.H]
        rng = np.random.default_rng(1000 + 37 * self.H + self.Fo)           # explicit decisions, nothing to do with Philox
        return rng.random((self.H, N, FIN)) < 1.0 - self.p

    def bits(self):
        """uint8 [N, FIN] of the decisions (H <= 8) or None."""
        k = self.keep()
        if k is None or self.H > 8:
            return None
        b = np.zeros((N, FIN), dtype=np.uint8)
        for h in range(self.H):
            b |= k[h].astype(np.uint8) << np.uint8(h)
        return b

    def inputs(self):
        H, Fo, Fp, R_ = self.H, self.Fo, self.Fp, self.R
        rng = np.random.default_rng(7 * H + Fo + (1 if self.skip else 0))
        if self.flavour == "exact":
            draw = lambda *shape: torch.as_tensor(rng.integers(-3, 4, size=shape)).float()  # noqa: E731
            a = torch.as_tensor(rng.integers(-2, 3, size=(H, 2 * Fo))).float()
        else:
            draw = lambda *shape: torch.as_tensor(rng.standard_normal(shape)).float()  # noqa: E731
            a = draw(H, 2 * Fo) * 0.3
        s = 1.0 if self.flavour == "exact" else 0.3
        W = draw(H, FIN, Fo) * s
        Ws = draw(H, FIN, Fo) * s if self.skip else None
        dWh = torch.zeros(N, H, Fp); dWh[:, :, :Fo] = draw(N, H, Fo)      # padded columns zero
        ldg = R_ + 4 * H                                                   # wider than the R columns the kernel reads
        Gp = draw(N, ldg)
        return dict(x=matrix(self.kind, self.flavour), W=W, a=a, Ws=Ws, dWh=dWh.view(N, R_), Gp=Gp, ldg=ldg)

    # -- ground truth ------------------------------------------------------------------------------
    def refs(self):
        """{name: (ref64, ref32)} with Wh, Sk [N, H, Fp] (padded columns 0), s [N, H], dW, dWskip [H, FIN, Fo]."""
        d, H, Fo, Fp = self.inputs(), self.H, self.Fo, self.Fp
        keep = self.keep()
        out = {}
        for dt in (np.float64, np.float32):
            x = d["x"].numpy().astype(dt)
            xm = np.broadcast_to(x, (H, N, FIN)) if keep is None else x[None] * (keep * dt(self.scale)).astype(dt)
            W, a = d["W"].numpy().astype(dt), d["a"].numpy().astype(dt)
            dWh = d["dWh"].numpy().astype(dt).reshape(N, H, Fp)
            r = {}

            def table(Wx):
                t = np.zeros((N, H, Fp), dtype=dt)
                t[:, :, :Fo] = np.matmul(xm, Wx).transpose(1, 0, 2)
                return t
            r["Wh"] = table(W)
            r["dW"] = np.matmul(xm.transpose(0, 2, 1), dWh[:, :, :Fo].transpose(1, 0, 2))
            if self.skip:
                Gp = d["Gp"].numpy().astype(dt)[:, :self.R].reshape(N, H, Fp)
                r["Sk"] = table(d["Ws"].numpy().astype(dt))
                r["dWskip"] = np.matmul(xm.transpose(0, 2, 1), Gp[:, :, :Fo].transpose(1, 0, 2))
            if self.with_s:
                r["s"] = np.stack([x @ (W[h] @ a[h, :Fo]) for h in range(H)], axis=1)
            if self.flavour == "exact" and dt is np.float64:
                self._assert_exact(np.abs(x), np.abs(W), np.abs(a), np.abs(dWh), d)
            for k, v in r.items():
                out.setdefault(k, []).append(v.astype(np.float64))
        return {k: tuple(v) for k, v in out.items()}

    def _assert_exact(self, x, W, a, dWh, d):
        """Every partial sum of every product, in any order, is an integer below 2^24: bounded by the product of the absolute
        values, the scale included (fp64 side)."""
        Fo, sc = self.Fo, self.scale
        assert sc == 2.0 and R.threshold(self.p)[0] == 1 << 31 if self.mask != "none" else sc == 1.0
        bound = [sc * float(np.matmul(x, W).max()), sc * float(np.matmul(x.T, dWh[:, :, :Fo].transpose(1, 0, 2)).max())]
        if self.skip:
            bound.append(sc * float(np.matmul(x, np.abs(d["Ws"].numpy().astype(np.float64))).max()))
            bound.append(sc * float((x.T @ np.abs(d["Gp"].numpy().astype(np.float64))).max()))
        if self.with_s:
            wa = np.stack([W[h] @ a[h, :Fo] for h in range(self.H)], axis=1)      # the packed score columns themselves
            bound += [float(wa.max()), float((x @ wa).max())]
        assert max(bound) < LIMIT, f"{self.name}: a partial sum can reach {max(bound):.3g} >= 2^24"

    # -- pricing -----------------------------------------------------------------------------------
    def outputs(self):
        return ["Wh", "dW"] + (["Sk", "dWskip"] if self.skip else []) + (["s"] if self.with_s else [])

    def price(self, got):
        """got {name: tensor in the device's layout}: every head against its fp64 product by parity.close_grad, padded columns
        exactly zero; the exact flavour bit for bit."""
        refs, H, Fo, Fp = self.refs(), self.H, self.Fo, self.Fp
        assert sorted(got) == sorted(self.outputs()), (self.name, sorted(got))
        worst = {}
        for name in self.outputs():
            r64, r32 = refs[name]
            g = np.asarray(torch.as_tensor(got[name]).detach().double().cpu().numpy()).reshape(r64.shape)
            for h in range(H):
                sl = (slice(None), h) if name in ("Wh", "Sk", "s") else (h,)
                e, _ = close_grad(g[sl], r64[sl], r32[sl], f"{self.name} {name} head {h}")
                worst[name] = max(worst.get(name, 0.0), e)
            if name in ("Wh", "Sk") and Fp > Fo:
                assert float(np.abs(g[:, :, Fo:]).max()) == 0.0, f"{self.name} {name}: padded columns are not zero"
            if self.flavour == "exact":
                bad = int((g != r64).sum())
                assert bad == 0, f"{self.name} {name}: {bad} of {g.size} entries differ from the exact result"
        return worst

    def rehearse(self):
        """The fp32 CPU products in the device's place.  Exact flavour: they ARE the fp64 products."""
        refs = self.refs()
        if self.flavour == "exact":
            for name, (r64, r32) in refs.items():
                assert np.array_equal(r64, r32), f"{self.name} {name}: the fp32 product is not exact"
        return self.price({name: torch.as_tensor(refs[name][1]).float() for name in self.outputs()})


F, T = False, True
#        kind    H   Fo  skip with_s mask
TABLE = [
    # no mask: forward columns 64, 65, 72, 128, 136, 256, 264, 387, 512; backward 64, 128, 256, 384, 512
    ("rows", 8, 8, F, F, "none"), ("rows", 1, 64, F, T, "none"), ("cols", 8, 8, F, T, "none"), ("cols", 8, 16, F, F, "none"),
    ("rows", 8, 16, F, T, "none"), ("cols", 8, 16, T, F, "none"), ("rows", 8, 16, T, T, "none"), ("cols", 3, 121, F, T, "none"),
    ("rows", 4, 64, T, F, "none"), ("cols", 4, 64, T, F, "none"),
    # explicit bytes: H = 1, 4, 5, 8 (hq_shift 0 and 1) at 1, 2, 4 and 8 columns per lane
    ("rows", 1, 7, F, F, "bytes"), ("cols", 4, 16, T, F, "bytes"), ("rows", 4, 32, T, F, "bytes"), ("cols", 4, 64, T, F, "bytes"),
    ("cols", 5, 8, T, F, "bytes"), ("rows", 8, 8, F, F, "bytes"),
    ("rows", 8, 16, T, F, "bytes"), ("cols", 8, 16, T, F, "bytes"), ("rows", 8, 32, T, F, "bytes"), ("cols", 8, 32, T, F, "bytes"),
    # seeded: H = 1, 5, 8 and, past what a byte holds, 9, 12, 13, 16, 17, 32 (hq_shift 2 and 3)
    ("cols", 1, 7, F, F, "seed"), ("rows", 5, 8, T, F, "seed"),
    ("rows", 8, 16, T, F, "seed"), ("cols", 8, 16, T, F, "seed"), ("rows", 8, 32, T, F, "seed"), ("cols", 8, 32, T, F, "seed"),
    ("rows", 9, 8, F, F, "seed"), ("cols", 9, 8, F, F, "seed"), ("rows", 9, 16, F, F, "seed"), ("cols", 16, 16, F, F, "seed"),
    ("rows", 13, 4, F, F, "seed"), ("cols", 13, 4, F, F, "seed"), ("rows", 16, 8, F, F, "seed"), ("cols", 16, 8, F, F, "seed"),
    ("rows", 12, 16, T, F, "seed"), ("cols", 12, 16, T, F, "seed"),
    ("rows", 17, 7, F, F, "seed"), ("cols", 17, 7, F, F, "seed"), ("rows", 32, 4, F, F, "seed"), ("cols", 32, 4, F, F, "seed"),
    ("rows", 32, 16, F, F, "seed"), ("cols", 32, 16, F, F, "seed"),
]


@functools.lru_cache(maxsize=None)
def cases():
    """{name: Case}: every row of the table in both value flavours."""
    out = {}
    for row in TABLE:
        for fl in FLAVOURS:
            c = Case(*row, fl)
            assert c.name not in out, c.name
            out[c.name] = c
    return out


def case_names():
    return list(cases())


def check_grid():
    """The table covers what the tests promise (the classes of every case come from the formulas above, not from a list)."""
    for fl in FLAVOURS:
        cs = [c for c in cases().values() if c.flavour == fl]
        assert {64, 65, 72, 128, 136, 256, 264, 387, 512} <= {c.ncols_fwd for c in cs}
        assert {64, 128, 256, 384, 512} <= {c.ncols_bwd for c in cs}
        assert (3, 121, False, True) in {(c.H, c.Fo, c.skip, c.with_s) for c in cs}              # 387: padded heads and s
        assert (4, 64, True, False) in {(c.H, c.Fo, c.skip, c.with_s) for c in cs}               # 512 exactly, s = NULL
        unmasked = [c for c in cs if c.mask == "none"]
        assert {("rows", q) for q in (1, 2, 4, 8)} <= {(c.kind, c.cpl_fwd) for c in unmasked}    # row edges meet the forward,
        assert {("cols", q) for q in (1, 2, 4, 8)} <= {(c.kind, c.cpl_bwd) for c in unmasked}    # column edges the backward
        assert {1, 4, 5, 8} <= {c.H for c in cs if c.mask == "bytes"}
        assert {1, 5, 8, 9, 12, 13, 16, 17, 32} <= {c.H for c in cs if c.mask == "seed"}
        masked = [c for c in cs if c.mask != "none"]
        assert all(c.cpl_fwd == c.cpl_bwd for c in masked)                                       # no score columns under a mask
        # every columns-per-lane x hq_shift class that exists (32 heads of 4 columns are 128 columns: no (1, 3))
        assert {(q, s) for q in (1, 2, 4, 8) for s in (0, 1, 2, 3)} - {(1, 3)} == {(c.cpl_fwd, c.hq_shift) for c in masked}
        seeded = {(c.H, c.Fo, c.skip) for c in cs if c.mask == "seed"}
        assert {(16, 8, False), (12, 16, True), (32, 4, False), (32, 16, False)} <= seeded       # hq_shift 2, 3 x CPL 2, 8
        for s in (0, 1, 2, 3):                                                                   # batches of 64, 32, 16, 8 pairs:
            assert {"rows", "cols"} <= {c.kind for c in masked if c.hq_shift == s}               # both kinds of edges
        for m in ("bytes", "seed"):                                                              # the product's wide masked shapes
            for Fo in (16, 32):
                assert {"rows", "cols"} <= {c.kind for c in cs if (c.mask, c.H, c.Fo, c.skip) == (m, 8, Fo, True)}
        assert any(c.padded for c in masked) and any(c.padded for c in unmasked)
        assert any(not c.padded for c in masked) and any(not c.padded for c in unmasked)
