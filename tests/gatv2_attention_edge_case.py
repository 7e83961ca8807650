"""Ground truth, inputs and the seeded cases of the tests of pygat_amd.gatv2_attention_edge (the EDGE instantiations of
csrc/k21_gatv2_attention.hip, pygat_amd/gatv2_attention.py).

Ground truth is torch autograd on the CPU through `gatv2_attention_edge_ref` -- spmm_ref(edge_softmax_ref((a * leaky_relu((x_dst[row] +
x_src[col]) + e, slope)).sum(-1)), v), the pattern builders and the two parts from dot_attention_case.py and the GATv2 pieces from
gatv2_attention_case.py by import -- run in fp64 and in fp32.  Loss L = <out, G>; G, x_dst, x_src, a, v and e seeded, fp32-rounded and fed
identically to the device and to both ground-truth runs.  Pricing is parity.check_autograd, unchanged: out by close_fwd, every gradient
by close_grad, de one more gradient (the last leaf).

The kink.  check_autograd knows nothing of LeakyReLU branch flips, so no case priced by it may have one.  With three terms t = (x_dst +
x_src) + e is two rounded adds, and its fp32 sign is no longer bound to be its fp64 sign: the first add's rounding error, some 2^-24 of
its size, can carry a sum that nearly cancels across zero.  Every case asserts, when it is built, that sign(t) agrees between the fp64
sum and the fp32 sum in the kernel's order of the two adds (`t3_signs_agree`); a case whose seed fails that goes on to the next seed
through NEXT_SEED: rare, some 1e-8 per element, against the 2e8 elements the cases hold (one case moved on).  The grid case draws all
three tables on the multiples of 2^-10 in [-4, 4]: every sum is then exact in fp32, and some t are exactly 0 -- it pins the
convention at t == 0, the slope in the value and in the derivative, as torch's.  The module case forms its three tables by fp32 matrix
products: it asserts, in fp64, that no (entry, head, feature) lies inside the band of `product_kinks3`, gatv2_attention_case's band
with the third term in it.

The attention vector is gatv2_attention_case's, scaled once more by sqrt(2 / 3): t ~ N(0, 3) with the third term, so the scores of a
head keep the standard deviation `std`.

`cases()` lists every seeded case; tests/test_gatv2_attention_edge_abi.py rehearses each of them on the CPU with the fp32 ground-truth
run standing in for the device, tests/test_gpu_gatv2_attention_edge.py runs them on the device and builds no case of its own."""
import math

import torch

import gatv2_attention_case as plain
from dot_attention_case import LANE_SHAPES, edge_softmax_ref, f32, lonely_hub_graph, nine_hubs, normal, spmm_ref, three_chunk_hub
from pattern_case import ModuleCase, seeded
from pattern_graphs import _asym_graph, _coo, _hub_graph, _rect_coo, _repeat_coo

SLOPE = plain.SLOPE
MODULE_BAND = plain.MODULE_BAND
EDGE_DIM = 6
GRID = 2.0 ** -10
MAX_E_FLOATS = 1 << 23
# the cases whose first seed failed an assertion made when a case is built (a sign of t that differs between fp64 and fp32; the module
# case's kink band), and how many seeds further they went.  No case moved on a seed because of its rehearsal.
NEXT_SEED = {"twice-longcol-three_chunk_hub-8x16-separate": 1}


def t3(row, col, x_dst, x_src, e):
    """t [E, (H,) F] = (x_dst[i] + x_src[j]) + e[c], the kernel's order of the two adds."""
    return (x_dst.index_select(0, row) + x_src.index_select(0, col)) + e


def scores(row, col, x_dst, x_src, a, e, slope):
    """s [E, H] | [E]: the GATv2 score of every entry with its edge features."""
    return (a * torch.nn.functional.leaky_relu(t3(row, col, x_dst, x_src, e), slope)).sum(-1)


def linear_scores(row, col, x_dst, x_src, a, e):
    """The score at slope 1, where LeakyReLU is the identity: a second ground truth."""
    return (a * t3(row, col, x_dst, x_src, e)).sum(-1)


def gatv2_attention_edge_ref(row, col, n_rows, x_dst, x_src, a, v, e, slope, score=None):
    s = scores(row, col, x_dst, x_src, a, e, slope) if score is None else score(row, col, x_dst, x_src, a, e)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s), v)


def t3_signs_agree(row, col, x_dst, x_src, e):
    """Does every t = (x_dst[i] + x_src[j]) + e[c] have the same sign in fp32, two rounded adds in this order, as in fp64?"""
    t64 = t3(row, col, x_dst.double(), x_src.double(), e.double())
    t32 = t3(row, col, x_dst.float(), x_src.float(), e.float())
    return torch.equal(torch.sign(t64), torch.sign(t32.double()))


def product_kinks3(row, col, h_dst, h_src, e, band=MODULE_BAND):
    """The number of (entry, head, feature) whose fp64 t lies inside the band around the kink, for tables that fp32 matrix products
    form: gatv2_attention_case.product_kinks with the third term in the sum and in the magnitude."""
    hd, hs, he = h_dst.double()[row], h_src.double()[col], e.double()
    floor = float(h_dst.abs().mean() + h_src.abs().mean() + e.abs().mean())
    t = hd + hs + he
    return int(((t != 0) & (t.abs() <= band * (hd.abs() + hs.abs() + he.abs()).clamp_min(floor))).sum())


def on_grid(t):
    """t rounded to the multiples of 2^-10 and clamped to [-4, 4]."""
    return (torch.round(t / GRID) * GRID).clamp(-4.0, 4.0)


class EdgeCase(plain.Case):
    """gatv2_attention_case.Case with e [E, H, F] ~ N(0, e_std^2) (without the head axis where heads is False), the last leaf.  zero: e
    is all zeros (and a is the parent's: the inputs of gatv2_attention_case's case of the same arguments).  grid: x_dst, x_src and e
    on the grid of 2^-10."""
    op = "gatv2_attention_edge"

    def __init__(self, name, row, col, shape, H, F, seed, e_std=1.0, zero=False, grid=False, **kw):
        super().__init__(name, row, col, shape, H, F, seed, **kw)
        E = row.numel()
        assert E * H * F <= MAX_E_FLOATS, name
        if zero:
            self.e = torch.zeros((E,) + tuple(self.x_dst.shape[1:]), dtype=torch.float64)
        else:
            self.e = f32(e_std * normal((E,) + tuple(self.x_dst.shape[1:]), seed + 5))
            self.a = f32(self.a * math.sqrt(2.0 / (2.0 + e_std * e_std)))
        if grid:
            self.x_dst, self.x_src, self.e = on_grid(self.x_dst), on_grid(self.x_src), on_grid(self.e)
        self.zero, self.grid = zero, grid
        assert t3_signs_agree(row, col, self.x_dst, self.x_src, self.e), f"{name}: a sign of t differs in fp32: take the next seed"

    @property
    def leaves(self):
        return super().leaves + [self.e]

    @property
    def names(self):
        return super().names + ["de"]

    def ref(self, x_dst, x_src, a, *rest, score=None):
        """rest = ([v,] e)."""
        v, e = (x_src, rest[0]) if self.shared else rest
        return gatv2_attention_edge_ref(self.row, self.col, self.shape[0], x_dst, x_src, a, v, e, self.slope, score).reshape(-1)

    def linear_ref(self, *leaves):
        assert self.slope == 1.0
        return self.ref(*leaves, score=linear_scores)

    def t(self, dtype=torch.float64):
        return t3(self.row, self.col, self.x_dst.to(dtype), self.x_src.to(dtype), self.e.to(dtype))

    def scores(self, dtype=torch.float64):
        return scores(self.row, self.col, self.x_dst.to(dtype), self.x_src.to(dtype), self.a.to(dtype), self.e.to(dtype), self.slope)

    def rehearse(self):
        assert t3_signs_agree(self.row, self.col, self.x_dst, self.x_src, self.e), self.name
        return self.price_all(*self.stand_in())


class BipartiteGATv2Edge(plain.BipartiteGATv2):
    """gatv2_attention_case.BipartiteGATv2 with edge features, as PyG's GATv2Conv(edge_dim=...) shapes them: edge_attr [E, edge_dim]
    goes through lin_edge (no bias) to a row of H heads of F columns per entry; `attend(h_dst, h_src, a, e)`."""

    def __init__(self, f_in, H, F, attend, seed):
        super().__init__(f_in, H, F, attend, seed)
        self.lin_edge = torch.nn.Linear(EDGE_DIM, H * F, bias=False)
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            self.lin_edge.weight.copy_(torch.randn(H * F, EDGE_DIM, generator=g) * (2.0 / (EDGE_DIM + F)) ** 0.5)

    def forward(self, x_src, x_dst, edge_attr):
        h_src, h_dst = (x_src @ self.W_l).view(-1, self.H, self.F), (x_dst @ self.W_r).view(-1, self.H, self.F)
        e = self.lin_edge(edge_attr).view(-1, self.H, self.F)
        return torch.nn.functional.elu(self.attend(h_dst, h_src, self.a, e))


class EdgeModuleCase(ModuleCase):
    """BipartiteGATv2Edge on the rectangular pattern: out and the gradients of its sum with respect to x_src, x_dst, edge_attr, W_l,
    W_r, a and the edge projection's weight, against the same module with the ground truth as `attend`, in fp64."""
    F_IN, H, F = 24, 2, 8
    INPUTS, NAMES = ("x_src", "x_dst", "edge_attr"), ("W_l", "W_r", "a", "lin_edge.weight")
    GRADS = ("dx_src", "dx_dst", "dedge_attr", "dW_l", "dW_r", "da", "dW_edge")

    def __init__(self, name, row, col, shape, seed, kind="indices", csr=None):
        self.name, self.row, self.col, self.shape, self.kind, self.csr, self.seed = name, row, col, shape, kind, csr, seed
        self.slope = SLOPE
        self.x_dst, self.x_src = f32(normal((shape[0], self.F_IN), seed)), f32(normal((shape[1], self.F_IN), seed + 1))
        self.edge_attr = f32(normal((row.numel(), EDGE_DIM), seed + 4))
        proto = self.module(None)
        self.weights = [f32(proto.get_parameter(n).detach().double()) for n in self.NAMES]
        self.G = torch.ones(shape[0] * self.H * self.F, dtype=torch.float64)              # the gradient of a sum
        n = self.kinks()
        assert n == 0, f"{name}: {n} (entry, head, feature) inside the kink band of the fp32 products: take the next seed"

    def kinks(self):
        W_l, W_r, _, W_e = self.weights
        h_src, h_dst = (self.x_src @ W_l).view(-1, self.H, self.F), (self.x_dst @ W_r).view(-1, self.H, self.F)
        return product_kinks3(self.row, self.col, h_dst, h_src, (self.edge_attr @ W_e.t()).view(-1, self.H, self.F))

    def module(self, attend):
        return BipartiteGATv2Edge(self.F_IN, self.H, self.F, attend, self.seed + 2)

    def ref_attend(self, h_dst, h_src, a, e):
        return gatv2_attention_edge_ref(self.row, self.col, self.shape[0], h_dst, h_src, a, h_src, e, self.slope)


def _build_cases():
    out = []

    def seed(name=None):
        return 60000 + 10 * len(out) + NEXT_SEED.get(name, 0)

    def add(name, row, col, shape, H, F, **kw):
        out.append(EdgeCase(name, row, col, shape, H, F, seed(name), **kw))
        return out[-1]

    # every lane shape on the hub pattern (a row and a column of 699 entries: the long launches of all three passes), from indices and
    # from a graph, v shared and separate, and on the asymmetric one (rows of one entry), from indices with v shared and from a graph
    # with v separate
    hub, asym = _hub_graph(), _asym_graph()
    row, col, N = _coo(hub)
    arow, acol, aN = _coo(asym)
    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            for shared in (True, False):
                add(f"lanes-hub-{H}x{F}-{kind}-{'shared' if shared else 'separate'}", row, col, (N, N), H, F, kind=kind, csr=hub,
                    shared=shared)
        add(f"lanes-asym-{H}x{F}-indices-shared", arow, acol, (aN, aN), H, F, csr=asym)
        add(f"lanes-asym-{H}x{F}-graph-separate", arow, acol, (aN, aN), H, F, kind="graph", csr=asym, shared=False)
    add("lanes-hub-noaxis-indices-shared", row, col, (N, N), 1, 16, heads=False)
    add("lanes-asym-noaxis-graph-separate", arow, acol, (aN, aN), 1, 64, kind="graph", heads=False, csr=asym, shared=False)
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
    add("lonely-8x16-indices-shared", orow, ocol, (oN, oN), 8, 16, csr=lonely)
    add("lonely-3x8-graph-separate", orow, ocol, (oN, oN), 3, 8, kind="graph", csr=lonely, shared=False)
    # e of zeros on the inputs of gatv2_attention_case's case of the same name: the bits of gatv2_attention
    tcsr = three_chunk_hub()
    trow, tcol, tN = _coo(tcsr)
    for zname in ("lanes-hub-8x16-graph-shared", "lanes-hub-12x64-indices-separate", "lanes-hub-4x256-indices-shared",
                  "lanes-asym-3x8-graph-separate", "longcol-three_chunk_hub-3x8-shared", "rect-3x8-separate"):
        p = plain.cases()[zname]
        z = EdgeCase("zero-" + zname, p.row, p.col, p.shape, p.H, p.F, 0, zero=True, kind=p.kind, csr=p.csr, std=p.std, shared=p.shared)
        z.x_dst, z.x_src, z.v, z.G, z.a, z.inner = p.x_dst, p.x_src, p.v, p.G, p.a, p
        out.append(z)
    for slope in (0.2, 0.0, 1.0):
        add(f"slope-hub-8x16-graph-shared-{slope:g}", row, col, (N, N), 8, 16, kind="graph", csr=hub, slope=slope)
        add(f"slope-rect-3x8-separate-{slope:g}", rrow, rcol, (300, 500), 3, 8, shared=False, slope=slope)
    ncsr = nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    add("twice-hub-3x8-graph-shared", row, col, (N, N), 3, 8, kind="graph", csr=hub)
    add("twice-hub-12x64-indices-separate", row, col, (N, N), 12, 64, shared=False)
    add("twice-longcol-nine_hubs-8x16-shared", ncol, nrow, (nN, nN), 8, 16, std=3.0)
    add("twice-longcol-three_chunk_hub-8x16-separate", tcol, trow, (tN, tN), 8, 16, std=3.0, shared=False)
    add("composed-hub-8x16-graph-shared", row, col, (N, N), 8, 16, kind="graph", csr=hub)
    add("composed-rect-3x8-separate", rrow, rcol, (300, 500), 3, 8, shared=False)
    add("strided-rect-4x16-shared", rrow, rcol, (300, 500), 4, 16)
    add("strided-hub-3x8-graph-separate", row, col, (N, N), 3, 8, kind="graph", csr=hub, shared=False)
    add("tail-rect-3x8-shared", rrow, rcol, (310, 520), 3, 8)                # the last 10 rows and 20 columns without entries
    add("grid-hub-8x16-indices-separate", row, col, (N, N), 8, 16, shared=False, grid=True)
    out.append(EdgeModuleCase("module-rect-2x8", rrow, rcol, (300, 500), seed("module-rect-2x8")))
    return out


cases, case_names = seeded(_build_cases)
