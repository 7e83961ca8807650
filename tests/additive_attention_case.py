"""Ground truth, inputs and the seeded cases of the tests of pygat_amd.additive_attention (csrc/k20_additive_attention.hip,
pygat_amd/additive_attention.py).

Ground truth is torch autograd on the CPU through `additive_attention_ref` -- spmm_ref(edge_softmax_ref(leaky_relu((s_dst[row] +
s_src[col]) + u))), the pattern builders and the two parts from dot_attention_case.py by import -- run in fp64 and in fp32.  Loss
L = <out, G>; G, s_dst, s_src, v and u seeded, fp32-rounded and fed identically to the device and to both ground-truth runs.  Pricing is
parity.check_autograd, unchanged: out by close_fwd, every gradient by close_grad.

The kink.  check_autograd knows nothing of LeakyReLU branch flips, so no case may have one.  Without a logit z = s_dst + s_src is one
correctly rounded add of two fp32 numbers: its sign in fp32 is its sign in fp64 (the exact sum of two floats does not round across
zero, and an exact zero takes the slope in both), so no flip is possible.  With a logit z is two rounded adds, and a case asserts, in
fp64, that no (entry, head) has 0 < |z| <= 2^-20 (|s_dst + s_src| + |u|): an fp32 z carries at most two roundings of 2^-24 relative to
those two magnitudes, a sixteenth of the band.  The cap is zero such entries; the seeds below were chosen so that every case passes.
The module and level cases form s_dst and s_src by fp32 matrix products of at most 24 + 8 terms, whose error is some 32 x 2^-24 =
2^-19 of the terms' magnitude: they assert the wider band 2^-16 max(|s_dst| + |s_src|, the mean magnitude of a score).

`cases()` lists every seeded case; tests/test_additive_attention_abi.py rehearses each of them on the CPU with the fp32 ground-truth
run standing in for the device, tests/test_gpu_additive_attention.py runs them on the device and builds no case of its own."""
import torch

import parity
from dot_attention_bias_case import MASK, first_of_row
from dot_attention_case import LANE_SHAPES, edge_softmax_ref, f32, lonely_hub_graph, nine_hubs, normal, spmm_ref, three_chunk_hub
from pattern_case import ModuleCase as ModuleCaseBase, OpCase, _report, seeded
from pattern_graphs import _asym_graph, _coo, _hub_graph, _rect_coo, _repeat_coo

SLOPE = 0.2
KINK_BAND = 2.0 ** -20
MODULE_BAND = 2.0 ** -16
# the cases whose first seed put an (entry, head) inside the kink band, and how many seeds further they went
NEXT_SEED = {"lanes-asym-12x64-indices-shared": 1, "masked-three_chunk_hub-3x8-graph": 1, "level-hub-3x6": 2, "module-rect-4x8": 1}


def _heads(t, like):
    """A [E] logit against [E, H] scores is shared by the heads."""
    return t[:, None] if t.dim() < like.dim() else t


def logits_z(row, col, s_dst, s_src, u=None):
    """z [E, H] | [E].  The gathers are index_select, whose backward adds the entries of a row or a column one after another in the
    caller's order: ds_src of a hub column is a few numbers, each the sum of thousands, and the fp32 run's own error on them -- what
    the device is priced against -- is then the same from run to run (indexing's backward adds in whatever order its threads meet)."""
    z = s_dst.index_select(0, row) + s_src.index_select(0, col)
    return z if u is None else z + _heads(u, z)


def additive_attention_ref(row, col, n_rows, s_dst, s_src, v, slope, u=None):
    l = torch.nn.functional.leaky_relu(logits_z(row, col, s_dst, s_src, u), slope)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, l), v)


def kinks(row, col, s_dst, s_src, u, band=KINK_BAND, floor=0.0):
    """The number of (entry, head) whose fp64 z lies inside the band around the kink, 0 < |z| <= band max(|s_dst + s_src| + |u|, floor)."""
    st = (s_dst[row] + s_src[col]).double()
    ud = _heads(u.double(), st)
    z = st + ud
    return int(((z != 0) & (z.abs() <= band * (st.abs() + ud.abs()).clamp_min(floor))).sum())


def product_kinks(row, col, s_dst, s_src):
    """... of scores that fp32 matrix products form: z = s_dst + s_src, the band relative to the two magnitudes or, where they cancel
    inside the products, to the mean magnitude of a score."""
    return kinks(row, col, s_dst, torch.zeros_like(s_src), s_src[col], MODULE_BAND, float(s_dst.abs().mean() + s_src.abs().mean()))


class Case(OpCase):
    """One seeded case: the entries (row, col) of a `shape` pattern, s_dst [n_rows, H], s_src [n_cols, H] ~ N(0, std^2), v [n_cols, H, F],
    G [n_rows, H, F] (without the head axis where heads is False) and the logit u: None, "full" ([E, H]; [E] without a head axis),
    "shared" ([E] for H heads), "zeros" or "masked" (MASK on a seeded third of the entries, never on a row's first); `kind` = how the
    device's pattern is built ("indices": EdgePattern.from_indices, entries as given; "graph": CSRGraph.edge_pattern() of the CSR the
    entries came from).  grid: s_dst on the integers + 1/4, s_src and u on the integers, slope 1/2: every z and every l is exact and
    no z is 0."""
    op = "additive_attention"

    def __init__(self, name, row, col, shape, H, F, seed, kind="indices", heads=True, csr=None, std=1.0, logit=None, slope=SLOPE,
                 grid=False):
        self.name, self.row, self.col, self.shape, self.H, self.F, self.kind, self.csr = name, row, col, shape, H, F, kind, csr
        self.slope, self.logit, self.masked = slope, logit, None
        hd = (H,) if heads else ()
        assert heads or H == 1
        E = row.numel()
        self.s_dst, self.s_src = f32(std * normal((shape[0],) + hd, seed)), f32(std * normal((shape[1],) + hd, seed + 1))
        self.v, self.G = f32(normal((shape[1],) + hd + (F,), seed + 2)), f32(normal((shape[0],) + hd + (F,), seed + 3))
        self.u = None
        if logit is not None:
            self.u = f32(std * normal((E,) if logit == "shared" else (E,) + hd, seed + 4))
        if logit == "zeros":
            self.u = torch.zeros_like(self.u)
        if logit == "masked":
            self.masked = (torch.rand(E, generator=torch.Generator().manual_seed(seed + 5)) < 1.0 / 3.0) & ~first_of_row(row)
            self.u[self.masked] = MASK
        if grid:
            self.s_dst, self.s_src = torch.round(2 * self.s_dst.clamp(-2, 2)) + 0.25, torch.round(2 * self.s_src.clamp(-2, 2))
            if self.u is not None:
                self.u = torch.round(2 * self.u.clamp(-2, 2))
        if self.u is not None:
            n = kinks(row, col, self.s_dst, self.s_src, self.u)
            assert n == 0, f"{name}: {n} (entry, head) inside the kink band: take the next seed"

    @property
    def leaves(self):
        return [self.s_dst, self.s_src, self.v] + ([] if self.u is None else [self.u])

    @property
    def names(self):
        return ["ds_dst", "ds_src", "dv"] + ([] if self.u is None else ["du"])

    def ref(self, s_dst, s_src, v, u=None):
        return additive_attention_ref(self.row, self.col, self.shape[0], s_dst, s_src, v, self.slope, u).reshape(-1)

    def composed_ref(self, s_dst, s_src, v, u=None):
        """The composition from parts as a user writes it: the same graph of torch ops, so it rehearses like ref."""
        return self.ref(s_dst, s_src, v, u)

    def coefficients(self, dtype=torch.float64):
        z = logits_z(self.row, self.col, self.s_dst.to(dtype), self.s_src.to(dtype), None if self.u is None else self.u.to(dtype))
        return edge_softmax_ref(self.row, self.shape[0], torch.nn.functional.leaky_relu(z, self.slope))

    def check_masked(self, du):
        if self.masked is not None:
            assert float(du.detach().cpu()[self.masked].abs().max()) == 0.0, f"{self.name}: du at a masked entry is an exact zero"

    def rehearse(self):
        res = self.stand_in()
        if self.masked is not None:
            self.check_masked(res[4])
        return self.price(*res)


class BipartiteGAT(torch.nn.Module):
    """A GAT layer from one node set to another in thirty lines: x_src [M, f_in] and x_dst [N, f_in] share one projection W to H heads
    of F columns and one attention vector a [H, 2 F] (its first half scores the destination, its second the source, as the
    reference's a); `attend(s_dst, s_src, v)` is the attention over the pattern's entries; ELU; the loss of the module case is the sum
    of what it returns."""

    def __init__(self, f_in, H, F, attend, seed):
        super().__init__()
        self.H, self.F, self.attend = H, F, attend
        g = torch.Generator().manual_seed(seed)
        self.W = torch.nn.Parameter(torch.randn(f_in, H * F, generator=g) * (2.0 / (f_in + F)) ** 0.5)
        self.a = torch.nn.Parameter(torch.randn(H, 2 * F, generator=g) * (2.0 / (2 * F + 1)) ** 0.5)

    def forward(self, x_src, x_dst):
        h_src, h_dst = ((x @ self.W).view(-1, self.H, self.F) for x in (x_src, x_dst))
        s_dst, s_src = (h_dst * self.a[:, :self.F]).sum(-1), (h_src * self.a[:, self.F:]).sum(-1)
        return torch.nn.functional.elu(self.attend(s_dst, s_src, h_src))


class ModuleCase(ModuleCaseBase):
    """BipartiteGAT on the rectangular pattern: out and the gradients of its sum with respect to x_src, x_dst, W and a, against the same
    module with the ground truth as `attend`, in fp64."""
    F_IN, H, F = 24, 4, 8
    INPUTS, NAMES, GRADS = ("x_src", "x_dst"), ("W", "a"), ("dx_src", "dx_dst", "dW", "da")

    def __init__(self, name, row, col, shape, seed, kind="indices", csr=None):
        self.name, self.row, self.col, self.shape, self.kind, self.csr, self.seed = name, row, col, shape, kind, csr, seed
        self.slope = SLOPE
        self.x_dst, self.x_src = f32(normal((shape[0], self.F_IN), seed)), f32(normal((shape[1], self.F_IN), seed + 1))
        proto = self.module(None)
        self.weights = [f32(proto.get_parameter(n).detach().double()) for n in self.NAMES]
        self.G = torch.ones(shape[0] * self.H * self.F, dtype=torch.float64)              # the gradient of a sum
        W, a = self.weights
        h_src, h_dst = ((x @ W).view(-1, self.H, self.F) for x in (self.x_src, self.x_dst))
        s_dst, s_src = (h_dst * a[:, :self.F]).sum(-1), (h_src * a[:, self.F:]).sum(-1)
        n = product_kinks(row, col, s_dst, s_src)
        assert n == 0, f"{name}: {n} (entry, head) inside the kink band of the fp32 products: take the next seed"

    def module(self, attend):
        return BipartiteGAT(self.F_IN, self.H, self.F, attend, self.seed + 2)

    def ref_attend(self, s_dst, s_src, v):
        return additive_attention_ref(self.row, self.col, self.shape[0], s_dst, s_src, v, self.slope)


class LevelCase:
    """A square graph and one GAT level of H heads of F columns on it, F no multiple of 4: x [N, f_in], W [H, f_in, F], a [H, 2 F].  The
    level's out [N, H, F] without ELU and without skip, head by head, in fp64 and in fp32: what gat_level(..., concat=False) of one
    head gives, and what additive_attention gives on (Wh . a[:F], Wh . a[F:], Wh) with Wh zero-padded to FP columns."""
    op = "level"
    F_IN, H, F, FP = 16, 3, 6, 8

    def __init__(self, name, csr, seed):
        self.name, self.csr, self.kind, self.slope = name, csr, "graph", SLOPE
        self.row, self.col, N = _coo(csr)
        self.shape = (N, N)
        self.x = f32(normal((N, self.F_IN), seed))
        self.W = f32(normal((self.H, self.F_IN, self.F), seed + 1) * (2.0 / (self.F_IN + self.F)) ** 0.5)
        self.a = f32(normal((self.H, 2 * self.F), seed + 2) * (2.0 / (2 * self.F + 1)) ** 0.5)
        s_dst, s_src, _ = self.tables(torch.float64)
        n = product_kinks(self.row, self.col, s_dst, s_src)
        assert n == 0, f"{name}: {n} (entry, head) inside the kink band of the fp32 products: take the next seed"

    def tables(self, dtype):
        """-> (s_dst [N, H], s_src [N, H], Wh [N, H, F]) of the level, formed in `dtype`."""
        Wh = torch.einsum("nk,hkf->nhf", self.x.to(dtype), self.W.to(dtype))
        a = self.a.to(dtype)
        return (Wh * a[:, None, :self.F].transpose(0, 1)).sum(-1), (Wh * a[:, None, self.F:].transpose(0, 1)).sum(-1), Wh

    def level(self, dtype):
        s_dst, s_src, Wh = self.tables(dtype)
        return additive_attention_ref(self.row, self.col, self.shape[0], s_dst, s_src, Wh, self.slope)

    def price(self, out, what):
        """out [N, H, F] of one run, head by head, by close_fwd against the fp64 level."""
        y64, y32 = self.level(torch.float64), self.level(torch.float32)
        assert out.shape == y64.shape, (what, out.shape)
        return _report(what, {f"head {h}": parity.close_fwd(out[:, h].reshape(-1), y64[:, h].reshape(-1), f"{what} head {h}",
                                                            y32[:, h].reshape(-1)) for h in range(self.H)})

    def rehearse(self):
        return self.price(self.level(torch.float32), self.name)


def _build_cases():
    out = []

    def seed(name=None):
        return 30000 + 10 * len(out) + NEXT_SEED.get(name, 0)

    def add(name, row, col, shape, H, F, **kw):
        out.append(Case(name, row, col, shape, H, F, seed(name), **kw))
        return out[-1]

    for pname, builder in (("hub", _hub_graph), ("asym", _asym_graph)):
        csr = builder()
        row, col, N = _coo(csr)
        for i, (H, F) in enumerate(LANE_SHAPES):
            for kind in ("indices", "graph"):
                # every lane shape without a logit and with a [E, H] one; a [E] one shared by the heads at every other shape
                add(f"lanes-{pname}-{H}x{F}-{kind}", row, col, (N, N), H, F, kind=kind, csr=csr)
                add(f"lanes-{pname}-{H}x{F}-{kind}-logit", row, col, (N, N), H, F, kind=kind, csr=csr, logit="full")
            if H > 1 and i % 2 == 0:
                add(f"lanes-{pname}-{H}x{F}-indices-shared", row, col, (N, N), H, F, logit="shared")
        for logit, tag in ((None, ""), ("full", "-logit")):
            add(f"lanes-{pname}-noaxis-indices{tag}", row, col, (N, N), 1, 16, heads=False, logit=logit)
            add(f"lanes-{pname}-noaxis-graph{tag}", row, col, (N, N), 1, 64, kind="graph", heads=False, csr=csr, logit=logit)
    hub = _hub_graph()
    row, col, N = _coo(hub)
    for pname, builder in (("nine_hubs", nine_hubs), ("three_chunk_hub", three_chunk_hub)):
        lcsr = builder()
        lrow, lcol, lN = _coo(lcsr)
        for H, F in ((8, 16), (3, 8)):
            for kind, logit, tag in (("indices", None, ""), ("graph", None, ""), ("indices", "full", "-logit"), ("graph", "shared", "-shared")):
                add(f"long-{pname}-{H}x{F}-{kind}{tag}", lrow, lcol, (lN, lN), H, F, kind=kind, csr=lcsr, std=3.0, logit=logit)
    for kind, logit, tag in (("indices", None, ""), ("graph", "full", "-logit"), ("indices", "shared", "-shared")):
        add(f"exact-hub-8x16-{kind}{tag}", row, col, (N, N), 8, 16, kind=kind, csr=hub, logit=logit, slope=0.5, grid=True)
    rrow, rcol = _rect_coo()
    add("rect-4x16", rrow, rcol, (300, 500), 4, 16)
    add("rect-3x8-logit", rrow, rcol, (300, 500), 3, 8, logit="full")
    prow, pcol, pN, pairs = _repeat_coo()
    add("repeats-8x16", prow, pcol, (pN, pN), 8, 16).pairs = pairs           # [(k, k')] positions of the repeated (row, col) pairs
    add("repeats-8x16-logit", prow, pcol, (pN, pN), 8, 16, logit="full").pairs = pairs
    lonely = lonely_hub_graph()
    orow, ocol, oN = _coo(lonely)
    for H, F in ((8, 16), (3, 8)):
        for kind, logit, tag in (("indices", None, ""), ("graph", "full", "-logit")):
            add(f"lonely-{H}x{F}-{kind}{tag}", orow, ocol, (oN, oN), H, F, kind=kind, csr=lonely, logit=logit)
    tcsr = three_chunk_hub()
    trow, tcol, tN = _coo(tcsr)
    add("zero-hub-12x64-indices", row, col, (N, N), 12, 64, logit="zeros")
    add("zero-hub-3x8-graph", row, col, (N, N), 3, 8, kind="graph", csr=hub, logit="zeros")
    add("zero-three_chunk_hub-8x16-indices", trow, tcol, (tN, tN), 8, 16, std=3.0, logit="zeros")
    add("masked-hub-8x16-indices", row, col, (N, N), 8, 16, logit="masked")
    add("masked-three_chunk_hub-3x8-graph", trow, tcol, (tN, tN), 3, 8, kind="graph", csr=tcsr, logit="masked")
    add("masked-rect-3x8", rrow, rcol, (300, 500), 3, 8, logit="masked")
    ncsr = nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    add("twice-nine_hubs-8x16-indices-logit", nrow, ncol, (nN, nN), 8, 16, std=3.0, logit="full")
    add("twice-hub-3x8-graph", row, col, (N, N), 3, 8, kind="graph", csr=hub)
    add("composed-hub-8x16-graph", row, col, (N, N), 8, 16, kind="graph", csr=hub)
    add("composed-hub-8x16-indices-logit", row, col, (N, N), 8, 16, std=3.0, logit="full")
    add("composed-rect-3x8-shared", rrow, rcol, (300, 500), 3, 8, logit="shared")
    out.append(LevelCase("level-hub-3x6", hub, seed("level-hub-3x6")))
    out.append(ModuleCase("module-rect-4x8", rrow, rcol, (300, 500), seed("module-rect-4x8")))
    return out


cases, case_names = seeded(_build_cases)
