"""Ground truth, inputs and the seeded cases of the tests of pygat_amd.dot_attention and pygat_amd.edge_dot
(csrc/k19_dot_attention.hip, pygat_amd/dot_attention.py).

Ground truth is torch autograd on the CPU through `dot_attention_ref` -- the gathered product, spmm_case.spmm_ref and
edge_softmax_case.edge_softmax_ref -- in any dtype.  Loss L = <out, G>; G, q, k, v ~ N(0, 1), seeded, fp32-rounded and fed identically to
the device and to both ground-truth runs.  Pricing is parity.check_autograd, unchanged: out by close_fwd, dq, dk, dv by close_grad.
`cases()` lists every seeded case; tests/test_dot_attention_abi.py rehearses each of them on the CPU with the fp32 ground-truth run
standing in for the device, tests/test_gpu_dot_attention.py runs them on the device and builds no case of its own."""
import math

import torch

from bf16_table_case import hub_graph as lonely_hub_graph
from edge_softmax_case import edge_softmax_ref
from long_row_cases import nine_hubs, three_chunk_hub
from pattern_case import ModuleCase as ModuleCaseBase, OpCase, seeded
from pattern_graphs import _asym_graph, _coo, _hub_graph, _rect_coo, _repeat_coo
from spmm_case import f32, normal, spmm_ref

# (H, F) of the lane-shape cases: chunks of 4 floats per row -> the lane layout (csrc/k19_dot_attention.hip)
LANE_SHAPES = ((1, 4), (1, 8), (3, 8), (8, 16), (6, 16), (4, 64), (16, 16), (3, 64), (12, 64), (4, 256), (64, 16), (1, 256))


def dot_attention_ref(row, col, n_rows, q, k, v, scale):
    s = (q[row] * k[col]).sum(-1) * scale
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s), v)


def edge_dot_ref(row, col, q, k, scale):
    return (q[row] * k[col]).sum(-1) * scale


class Case(OpCase):
    """One seeded dot_attention case: the entries (row, col) of a `shape` pattern, q [n_rows, H, F], k, v [n_cols, H, F], G like q
    (without the head axis where heads is False); `kind` = how the device's pattern is built ("indices": EdgePattern.from_indices,
    entries as given; "graph": CSRGraph.edge_pattern() of the CSR the entries came from).  scale: None = the op's default
    1 / sqrt(F), "sharp" = 3 / sqrt(F) (logits of std 3: a few entries dominate a row), or a number.  grid: q and k on the integer
    grid round(2 clamp(x, -2, 2)), so that with scale 1 every score is a whole number below 2^24 in any summation order."""
    op = "dot_attention"

    def __init__(self, name, row, col, shape, H, F, seed, kind="indices", scale=None, heads=True, csr=None, grid=False):
        self.name, self.row, self.col, self.shape, self.H, self.F, self.kind, self.csr = name, row, col, shape, H, F, kind, csr
        dims = (H, F) if heads else (F,)
        assert heads or H == 1
        self.q, self.k = f32(normal((shape[0],) + dims, seed)), f32(normal((shape[1],) + dims, seed + 1))
        self.v, self.G = f32(normal((shape[1],) + dims, seed + 2)), f32(normal((shape[0],) + dims, seed + 3))
        if grid:
            self.q, self.k = torch.round(2 * self.q.clamp(-2, 2)), torch.round(2 * self.k.clamp(-2, 2))
        self.fed_scale = 3.0 / math.sqrt(F) if scale == "sharp" else scale      # what the op is given (None: its default)
        self.scale = 1.0 / math.sqrt(F) if self.fed_scale is None else float(self.fed_scale)

    names = ["dq", "dk", "dv"]

    @property
    def leaves(self):
        return [self.q, self.k, self.v]

    def ref(self, q, k, v):
        return dot_attention_ref(self.row, self.col, self.shape[0], q, k, v, self.scale).reshape(-1)

    def scores(self, dtype=torch.float64):
        return edge_dot_ref(self.row, self.col, self.q.to(dtype), self.k.to(dtype), self.scale)

    def price(self, out, dq, dk, dv, what=None):
        """out and the three gradients of one run against the ground truth -> (report, out in fp64 shaped like q)."""
        return self.price_y64(out, dq, dk, dv, what=what)


class ComposedCase(Case):
    """The same result from parts -- spmm(edge_softmax(edge_dot(q, k, scale)), v) -- priced against the fused op's ground truth."""

    def composed_ref(self, q, k, v):
        row, col, n = self.row, self.col, self.shape[0]
        return spmm_ref(row, col, n, edge_softmax_ref(row, n, edge_dot_ref(row, col, q, k, self.scale)), v).reshape(-1)

    def rehearse(self):
        self.price(*self.stand_in(), what=self.name + " fused")
        return self.price(*self.stand_in(self.composed_ref), what=self.name + " from parts")


class DotCase(OpCase):
    """One seeded edge_dot case: u [E, H] | [E] against (q[row] * k[col]).sum(-1) * scale, loss <u, G>."""
    op = "edge_dot"

    def __init__(self, name, row, col, shape, H, F, seed, kind="indices", scale=1.0, heads=True, csr=None):
        self.name, self.row, self.col, self.shape, self.H, self.F, self.kind, self.csr = name, row, col, shape, H, F, kind, csr
        dims = (H, F) if heads else (F,)
        assert heads or H == 1
        self.q, self.k = f32(normal((shape[0],) + dims, seed)), f32(normal((shape[1],) + dims, seed + 1))
        self.G = f32(normal((row.numel(), H) if heads else (row.numel(),), seed + 2))
        self.scale = self.fed_scale = float(scale)

    names = ["dq", "dk"]

    @property
    def leaves(self):
        return [self.q, self.k]

    def ref(self, q, k):
        return edge_dot_ref(self.row, self.col, q, k, self.scale).reshape(-1)


class AttentionModule(torch.nn.Module):
    """A graph-transformer layer in thirty lines: three projections of x [N, f_in] to H heads of F columns, attention over the pattern's
    entries by `attend(q, k, v)`; the loss of the module case is the sum of what it returns."""

    def __init__(self, f_in, H, F, attend, seed):
        super().__init__()
        self.H, self.F, self.attend = H, F, attend
        self.query, self.key, self.value = (torch.nn.Linear(f_in, H * F, bias=False) for _ in range(3))
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for lin in (self.query, self.key, self.value):
                lin.weight.copy_(torch.randn(H * F, f_in, generator=g) * (2.0 / (f_in + F)) ** 0.5)

    def forward(self, x):
        q, k, v = (lin(x).view(-1, self.H, self.F) for lin in (self.query, self.key, self.value))
        return self.attend(q, k, v)


class ModuleCase(ModuleCaseBase):
    """AttentionModule on the hub pattern: out and the gradients of its sum with respect to x and the three weights, against the same
    module with the ground truth as `attend`, in fp64."""
    F_IN, H, F = 48, 4, 16
    INPUTS, NAMES, GRADS = ("x",), ("query.weight", "key.weight", "value.weight"), ("dx", "dWq", "dWk", "dWv")

    def __init__(self, name, row, col, N, seed, kind="graph", csr=None):
        self.name, self.row, self.col, self.shape, self.kind, self.csr, self.seed = name, row, col, (N, N), kind, csr, seed
        self.x = f32(normal((N, self.F_IN), seed))
        self.scale = 1.0 / math.sqrt(self.F)
        self.fed_scale = None
        proto = self.module(None)
        self.weights = [f32(proto.get_parameter(n).detach().double()) for n in self.NAMES]
        self.G = torch.ones(N * self.H * self.F, dtype=torch.float64)                  # the gradient of a sum

    def module(self, attend):
        return AttentionModule(self.F_IN, self.H, self.F, attend, self.seed + 1)

    def ref_attend(self, q, k, v):
        return dot_attention_ref(self.row, self.col, self.shape[0], q, k, v, self.scale)


def _build_cases():
    out = []
    for pname, builder in (("hub", _hub_graph), ("asym", _asym_graph)):
        csr = builder()
        row, col, N = _coo(csr)
        for H, F in LANE_SHAPES:
            for kind in ("indices", "graph"):
                out.append(Case(f"lanes-{pname}-{H}x{F}-{kind}", row, col, (N, N), H, F, 1000 + 10 * len(out), kind=kind, csr=csr))
        out.append(Case(f"lanes-{pname}-noaxis-indices", row, col, (N, N), 1, 16, 1000 + 10 * len(out), heads=False))
        out.append(Case(f"lanes-{pname}-noaxis-graph", row, col, (N, N), 1, 64, 1000 + 10 * len(out), kind="graph", heads=False, csr=csr))
    csr = _hub_graph()
    row, col, N = _coo(csr)
    out.append(Case("sharp-hub-4x256-indices", row, col, (N, N), 4, 256, 2000, scale="sharp"))
    for pname, builder in (("nine_hubs", nine_hubs), ("three_chunk_hub", three_chunk_hub)):
        lcsr = builder()
        lrow, lcol, lN = _coo(lcsr)
        for H, F in ((8, 16), (3, 8)):
            for kind in ("indices", "graph"):
                out.append(Case(f"long-{pname}-{H}x{F}-{kind}", lrow, lcol, (lN, lN), H, F, 3000 + 10 * len(out), kind=kind, scale="sharp",
                                csr=lcsr))
    for kind in ("indices", "graph"):
        out.append(Case(f"exact-hub-8x16-{kind}", row, col, (N, N), 8, 16, 4000, kind=kind, scale=1.0, csr=csr, grid=True))
    rrow, rcol = _rect_coo()
    out.append(Case("rect-4x16", rrow, rcol, (300, 500), 4, 16, 5000))
    out.append(Case("rect-3x8", rrow, rcol, (300, 500), 3, 8, 5010))
    prow, pcol, pN, pairs = _repeat_coo()
    out.append(Case("repeats-8x16", prow, pcol, (pN, pN), 8, 16, 6000))
    out[-1].pairs = pairs                                        # [(k, k')] positions of the repeated (row, col) pairs
    lonely = lonely_hub_graph()
    orow, ocol, oN = _coo(lonely)
    for H, F in ((8, 16), (3, 8)):
        for kind in ("indices", "graph"):
            out.append(Case(f"lonely-{H}x{F}-{kind}", orow, ocol, (oN, oN), H, F, 7000 + H, kind=kind, csr=lonely))
    ncsr = nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    out.append(Case("twice-nine_hubs-8x16-indices", nrow, ncol, (nN, nN), 8, 16, 7400, scale="sharp"))
    out.append(Case("twice-hub-3x8-graph", row, col, (N, N), 3, 8, 7410, kind="graph", csr=csr))
    out.append(ComposedCase("composed-hub-8x16-graph", row, col, (N, N), 8, 16, 7500, kind="graph", csr=csr))
    out.append(ComposedCase("composed-hub-8x16-indices", row, col, (N, N), 8, 16, 7510, scale="sharp"))
    acsr = _asym_graph()
    arow, acol, aN = _coo(acsr)
    out.append(DotCase("dot-hub-8x16-indices", row, col, (N, N), 8, 16, 7600, scale=0.25))
    out.append(DotCase("dot-asym-3x7-graph", arow, acol, (aN, aN), 3, 7, 7610, kind="graph", csr=acsr))
    out.append(DotCase("dot-rect-3x7-indices", rrow, rcol, (300, 500), 3, 7, 7620, scale=3.0 / math.sqrt(7)))
    out.append(DotCase("dot-hub-noaxis-indices", row, col, (N, N), 1, 16, 7630, heads=False))
    out.append(ModuleCase("module-hub-4x16-graph", row, col, N, 7700, csr=csr))
    return out


cases, case_names = seeded(_build_cases)
