"""Ground truth, inputs and the seeded cases of the tests of pygat_amd.gatv2_attention (csrc/k21_gatv2_attention.hip,
pygat_amd/gatv2_attention.py).

Ground truth is torch autograd on the CPU through `gatv2_attention_ref` -- spmm_ref(edge_softmax_ref((a * leaky_relu(x_dst[row] +
x_src[col], slope)).sum(-1)), v), the pattern builders and the two parts from dot_attention_case.py by import -- run in fp64 and in
fp32.  The gathers are index_select, for the reason additive_attention_case.py gives: its backward adds the entries of a row or a column
one after another in the caller's order, so the fp32 run's own error on a hub column is the same from run to run.  Loss L = <out, G>;
G, x_dst, x_src, a and v seeded, fp32-rounded and fed identically to the device and to both ground-truth runs.  Pricing is
parity.check_autograd, unchanged: out by close_fwd, every gradient by close_grad.

The kink.  check_autograd knows nothing of LeakyReLU branch flips, so no case priced by it may have one.  Where the tables are the
leaves, t = x_dst + x_src is one correctly rounded add of two fp32 numbers: its sign in fp32 is its sign in fp64 (the exact sum of two
floats does not round across zero, and an exact zero takes the slope in both), so no flip is possible; `t_signs_agree` asserts it.  The
module case forms its two tables by fp32 matrix products of 24 terms, whose error is some 24 x 2^-24 of the terms' magnitude each: it
asserts, in fp64, that no (entry, head, feature) has 0 < |t| <= 2^-16 max(|h_dst| + |h_src|, the mean magnitude of a table).  The level
case is priced by parity.check_level_v2, which is flip-aware per (edge, head, feature).

The attention vector.  a [H, F] is drawn N(0, 1) per head and scaled to the norm std / sqrt(var g), var g = 1 + slope^2 - (1 - slope)^2 /
pi the variance of LeakyReLU(t) for t ~ N(0, 2): the scores of a head then have the standard deviation `std` (1, or 3 for the long
cases, where a few entries dominate a row).

`cases()` lists every seeded case; tests/test_gatv2_attention_abi.py rehearses each of them on the CPU with the fp32 ground-truth run
standing in for the device, tests/test_gpu_gatv2_attention.py runs them on the device and builds no case of its own."""
import math

import numpy as np
import torch

import parity
from dot_attention_case import LANE_SHAPES, edge_softmax_ref, f32, lonely_hub_graph, nine_hubs, normal, spmm_ref, three_chunk_hub
from pattern_case import ModuleCase as ModuleCaseBase, OpCase, seeded
from pattern_graphs import _asym_graph, _coo, _hub_graph, _rect_coo, _repeat_coo

SLOPE = 0.2
MODULE_BAND = 2.0 ** -16
# the cases whose first seed failed an assertion made when a case is built (the module case's kink band), and how many seeds further
# they went.  No case moved on a seed because of its rehearsal.
NEXT_SEED = {"module-rect-2x8": 4}


def scores(row, col, x_dst, x_src, a, slope):
    """s [E, H] | [E]: the GATv2 score of every entry."""
    t = x_dst.index_select(0, row) + x_src.index_select(0, col)
    return (a * torch.nn.functional.leaky_relu(t, slope)).sum(-1)


def linear_scores(row, col, x_dst, x_src, a):
    """The score at slope 1, where LeakyReLU is the identity: a second ground truth."""
    return (a * (x_dst.index_select(0, row) + x_src.index_select(0, col))).sum(-1)


def gatv2_attention_ref(row, col, n_rows, x_dst, x_src, a, v, slope, score=None):
    s = scores(row, col, x_dst, x_src, a, slope) if score is None else score(row, col, x_dst, x_src, a)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s), v)


def t_signs_agree(row, col, x_dst, x_src):
    """Does every t = x_dst[i] + x_src[j] have the same sign in fp32 as in fp64?"""
    t64 = x_dst.double()[row] + x_src.double()[col]
    t32 = x_dst.float()[row] + x_src.float()[col]
    return torch.equal(torch.sign(t64), torch.sign(t32.double()))


def product_kinks(row, col, h_dst, h_src, band=MODULE_BAND):
    """The number of (entry, head, feature) whose fp64 t lies inside the band around the kink, for tables that fp32 matrix products form."""
    hd, hs = h_dst.double()[row], h_src.double()[col]
    floor = float(h_dst.abs().mean() + h_src.abs().mean())
    t = hd + hs
    return int(((t != 0) & (t.abs() <= band * (hd.abs() + hs.abs()).clamp_min(floor))).sum())


def score_unit(slope):
    """The standard deviation of LeakyReLU(t), t ~ N(0, 2)."""
    return math.sqrt(1.0 + slope * slope - (1.0 - slope) ** 2 / math.pi)


class Case(OpCase):
    """One seeded case: the entries (row, col) of a `shape` pattern, x_dst [n_rows, H, F], x_src [n_cols, H, F] ~ N(0, 1), a [H, F] of
    norm std / score_unit per head, G like x_dst (without the head axis where heads is False) and v: None (shared: v is x_src, the
    op's v=None) or a table of its own; `kind` = how the device's pattern is built ("indices": EdgePattern.from_indices, entries as
    given; "graph": CSRGraph.edge_pattern() of the CSR the entries came from)."""
    op = "gatv2_attention"

    def __init__(self, name, row, col, shape, H, F, seed, kind="indices", heads=True, csr=None, std=1.0, shared=True, slope=SLOPE):
        self.name, self.row, self.col, self.shape, self.H, self.F, self.kind, self.csr = name, row, col, shape, H, F, kind, csr
        self.slope, self.shared, self.std = slope, shared, std
        hd = (H,) if heads else ()
        assert heads or H == 1
        self.x_dst, self.x_src = f32(normal((shape[0],) + hd + (F,), seed)), f32(normal((shape[1],) + hd + (F,), seed + 1))
        self.v = None if shared else f32(normal((shape[1],) + hd + (F,), seed + 2))
        self.G = f32(normal((shape[0],) + hd + (F,), seed + 3))
        n = normal(hd + (F,), seed + 4)
        self.a = f32(std * n / n.norm(dim=-1, keepdim=True) / score_unit(slope))

    @property
    def leaves(self):
        return [self.x_dst, self.x_src, self.a] + ([] if self.shared else [self.v])

    @property
    def names(self):
        return ["dx_dst", "dx_src", "da"] + ([] if self.shared else ["dv"])

    def ref(self, x_dst, x_src, a, v=None, score=None):
        return gatv2_attention_ref(self.row, self.col, self.shape[0], x_dst, x_src, a, x_src if v is None else v, self.slope,
                                   score).reshape(-1)

    def linear_ref(self, x_dst, x_src, a, v=None):
        assert self.slope == 1.0
        return self.ref(x_dst, x_src, a, v, linear_scores)

    def scores(self, dtype=torch.float64):
        return scores(self.row, self.col, self.x_dst.to(dtype), self.x_src.to(dtype), self.a.to(dtype), self.slope)

    def coefficients(self, dtype=torch.float64):
        return edge_softmax_ref(self.row, self.shape[0], self.scores(dtype))

    def price_all(self, out, *grads, what=None):
        """... and, at slope 1, against the linear ground truth too."""
        rep = self.price(out, *grads, what=what)
        if self.slope == 1.0:
            self.price(out, *grads, what=(what or self.name) + " (linear)", ref=self.linear_ref)
        return rep

    def rehearse(self):
        assert t_signs_agree(self.row, self.col, self.x_dst, self.x_src), self.name
        return self.price_all(*self.stand_in())


class BipartiteGATv2(torch.nn.Module):
    """A GATv2 layer from one node set to another in thirty lines, as PyG's GATv2Conv shapes it: x_src [M, f_in] goes through W_l and
    x_dst [N, f_in] through W_r to H heads of F columns, one attention vector a [H, F]; `attend(h_dst, h_src, a)` is the attention over
    the pattern's entries, which aggregates the source table; ELU; the loss of the module case is the sum of what it returns."""

    def __init__(self, f_in, H, F, attend, seed):
        super().__init__()
        self.H, self.F, self.attend = H, F, attend
        g = torch.Generator().manual_seed(seed)
        self.W_l = torch.nn.Parameter(torch.randn(f_in, H * F, generator=g) * (2.0 / (f_in + F)) ** 0.5)
        self.W_r = torch.nn.Parameter(torch.randn(f_in, H * F, generator=g) * (2.0 / (f_in + F)) ** 0.5)
        self.a = torch.nn.Parameter(torch.randn(H, F, generator=g) * (2.0 / (F + 1)) ** 0.5)

    def forward(self, x_src, x_dst):
        h_src, h_dst = (x_src @ self.W_l).view(-1, self.H, self.F), (x_dst @ self.W_r).view(-1, self.H, self.F)
        return torch.nn.functional.elu(self.attend(h_dst, h_src, self.a))


class ModuleCase(ModuleCaseBase):
    """BipartiteGATv2 on the rectangular pattern: out and the gradients of its sum with respect to x_src, x_dst, W_l, W_r and a,
    against the same module with the ground truth as `attend`, in fp64."""
    F_IN, H, F = 24, 2, 8
    INPUTS, NAMES, GRADS = ("x_src", "x_dst"), ("W_l", "W_r", "a"), ("dx_src", "dx_dst", "dW_l", "dW_r", "da")

    def __init__(self, name, row, col, shape, seed, kind="indices", csr=None):
        self.name, self.row, self.col, self.shape, self.kind, self.csr, self.seed = name, row, col, shape, kind, csr, seed
        self.slope = SLOPE
        self.x_dst, self.x_src = f32(normal((shape[0], self.F_IN), seed)), f32(normal((shape[1], self.F_IN), seed + 1))
        proto = self.module(None)
        self.weights = [f32(proto.get_parameter(n).detach().double()) for n in self.NAMES]
        self.G = torch.ones(shape[0] * self.H * self.F, dtype=torch.float64)              # the gradient of a sum
        W_l, W_r, _ = self.weights
        h_src, h_dst = (self.x_src @ W_l).view(-1, self.H, self.F), (self.x_dst @ W_r).view(-1, self.H, self.F)
        n = product_kinks(row, col, h_dst, h_src)
        assert n == 0, f"{name}: {n} (entry, head, feature) inside the kink band of the fp32 products: take the next seed"

    def module(self, attend):
        return BipartiteGATv2(self.F_IN, self.H, self.F, attend, self.seed + 2)

    def ref_attend(self, h_dst, h_src, a):
        return gatv2_attention_ref(self.row, self.col, self.shape[0], h_dst, h_src, a, h_src, self.slope)


class LevelCase:
    """A square graph and one level of the reference's SpGraphAttentionLayerV2 on it, H heads of F columns, F no multiple of 4:
    X [N, f_in], W [H, 2 f_in, F] (Whi = X W[:f_in], Whj = X W[f_in:]), a [H, F], concat (ELU), loss <out, G>.  Priced by
    parity.check_level_v2, unchanged: what gatv2_level gives, and what elu(gatv2_attention(pattern, Whi, Whj, a, v=Whi)) gives with
    the tables formed by torch on the device and every column count zero-padded to FP."""
    op = "level"
    F_IN, H, F, FP = 16, 3, 6, 8

    def __init__(self, name, csr, seed):
        self.name, self.csr, self.kind, self.slope = name, csr, "graph", SLOPE
        self.row, self.col, N = _coo(csr)
        self.shape = (N, N)
        self.X = f32(normal((N, self.F_IN), seed))
        self.W = f32(normal((self.H, 2 * self.F_IN, self.F), seed + 1) * (2.0 / (2 * self.F_IN + self.F)) ** 0.5)
        self.a = f32(normal((self.H, self.F), seed + 2) * (2.0 / (1 + self.F)) ** 0.5)
        self.G = f32(normal((N, self.H * self.F), seed + 3))

    def price(self, out, dX, dW, da, what):
        """out [N, H F] and the three gradients of one run, by the flip-aware rule of the GATv2 level."""
        rowptr, col = (np.asarray(t) for t in self.csr)
        return parity.check_level_v2(out, {"dX": dX, "dW": dW, "da": da}, self.X.numpy(), rowptr, col, self.W.numpy(), self.a.numpy(),
                                     self.slope, True, self.G.numpy(), what=what)

    def rehearse(self):
        rowptr, col = (np.asarray(t) for t in self.csr)
        r = parity.v2_oracle(self.X.numpy(), rowptr, col, self.W.numpy(), self.a.numpy(), self.slope, True, self.G.numpy(),
                             dtype=torch.float32)
        return self.price(r["out"], r["dX"], r["dW"], r["da"], self.name)


def _build_cases():
    out = []

    def seed(name=None):
        return 40000 + 10 * len(out) + NEXT_SEED.get(name, 0)

    def add(name, row, col, shape, H, F, **kw):
        out.append(Case(name, row, col, shape, H, F, seed(name), **kw))
        return out[-1]

    # every lane shape on the hub pattern (a row and a column of 699 entries: the long launches of all three passes) and on the
    # asymmetric one, from indices and from a graph, v shared and separate
    for pname, builder in (("hub", _hub_graph), ("asym", _asym_graph)):
        csr = builder()
        row, col, N = _coo(csr)
        for H, F in LANE_SHAPES:
            for kind in ("indices", "graph"):
                for shared in (True, False):
                    add(f"lanes-{pname}-{H}x{F}-{kind}-{'shared' if shared else 'separate'}", row, col, (N, N), H, F, kind=kind, csr=csr,
                        shared=shared)
        add(f"lanes-{pname}-noaxis-indices-shared", row, col, (N, N), 1, 16, heads=False)
        add(f"lanes-{pname}-noaxis-graph-separate", row, col, (N, N), 1, 64, kind="graph", heads=False, csr=csr, shared=False)
    hub = _hub_graph()
    row, col, N = _coo(hub)
    # long rows, and the same patterns with rows and columns swapped: long columns (entries then unsorted: indices only)
    for pname, builder in (("nine_hubs", nine_hubs), ("three_chunk_hub", three_chunk_hub)):
        lcsr = builder()
        lrow, lcol, lN = _coo(lcsr)
        for H, F in ((8, 16), (3, 8)):
            add(f"long-{pname}-{H}x{F}-indices-shared", lrow, lcol, (lN, lN), H, F, csr=lcsr, std=3.0)
            add(f"long-{pname}-{H}x{F}-graph-separate", lrow, lcol, (lN, lN), H, F, kind="graph", csr=lcsr, std=3.0, shared=False)
            add(f"longcol-{pname}-{H}x{F}-shared", lcol, lrow, (lN, lN), H, F, std=3.0)
        add(f"longcol-{pname}-8x16-separate", lcol, lrow, (lN, lN), 8, 16, std=3.0, shared=False)
    rrow, rcol = _rect_coo()
    add("rect-4x16-shared", rrow, rcol, (300, 500), 4, 16)
    add("rect-3x8-separate", rrow, rcol, (300, 500), 3, 8, shared=False)
    prow, pcol, pN, pairs = _repeat_coo()
    add("repeats-8x16-shared", prow, pcol, (pN, pN), 8, 16).pairs = pairs    # [(k, k')] positions of the repeated (row, col) pairs
    add("repeats-8x16-separate", prow, pcol, (pN, pN), 8, 16, shared=False).pairs = pairs
    lonely = lonely_hub_graph()
    orow, ocol, oN = _coo(lonely)
    for H, F in ((8, 16), (3, 8)):
        add(f"lonely-{H}x{F}-indices-shared", orow, ocol, (oN, oN), H, F, csr=lonely)
        add(f"lonely-{H}x{F}-graph-separate", orow, ocol, (oN, oN), H, F, kind="graph", csr=lonely, shared=False)
    for slope in (0.2, 0.0, 1.0):
        add(f"slope-hub-8x16-graph-shared-{slope:g}", row, col, (N, N), 8, 16, kind="graph", csr=hub, slope=slope)
        add(f"slope-rect-3x8-separate-{slope:g}", rrow, rcol, (300, 500), 3, 8, shared=False, slope=slope)
    # v=None against v=x_src.clone(): the same inputs through both kernel variants
    add("same-hub-8x16-indices", row, col, (N, N), 8, 16)
    add("same-hub-12x64-graph", row, col, (N, N), 12, 64, kind="graph", csr=hub)
    tcsr = three_chunk_hub()
    trow, tcol, tN = _coo(tcsr)
    add("same-longcol-three_chunk_hub-3x8", tcol, trow, (tN, tN), 3, 8, std=3.0)
    ncsr = nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    add("twice-hub-3x8-graph-shared", row, col, (N, N), 3, 8, kind="graph", csr=hub)
    add("twice-hub-12x64-indices-separate", row, col, (N, N), 12, 64, shared=False)
    add("twice-longcol-nine_hubs-8x16-shared", ncol, nrow, (nN, nN), 8, 16, std=3.0)
    add("twice-longcol-three_chunk_hub-8x16-separate", tcol, trow, (tN, tN), 8, 16, std=3.0, shared=False)
    add("composed-hub-8x16-graph-shared", row, col, (N, N), 8, 16, kind="graph", csr=hub)
    add("composed-hub-8x16-indices-separate", row, col, (N, N), 8, 16, std=3.0, shared=False)
    add("composed-rect-3x8-shared", rrow, rcol, (300, 500), 3, 8)
    out.append(LevelCase("level-hub-3x6", hub, seed("level-hub-3x6")))
    out.append(ModuleCase("module-rect-2x8", rrow, rcol, (300, 500), seed("module-rect-2x8")))
    # (added last: a case's seed follows from its place in the list)
    add("tail-rect-3x8-shared", rrow, rcol, (310, 520), 3, 8)                # the last 10 rows and 20 columns without entries
    return out


cases, case_names = seeded(_build_cases)
