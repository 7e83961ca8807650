"""The seeded cases of pygat_amd.dot_attention_edge: dot_attention with a feature row per entry on the key and the value side (the EDGE
instantiations of csrc/k19_dot_attention.hip, pygat_amd/dot_attention.py).

Patterns, inputs, the ground truth's parts and the module come from dot_attention_case.py and dot_attention_bias_case.py by import; a
case here wraps a dot_attention_case.Case and adds e ([E, H, F]; [E, F] without a head axis): seeded, N(0, 1) x a per-case std,
fp32-rounded and fed identically to the device and to both ground-truth runs, and optionally a bias.  Ground truth is
spmm_ref(edge_softmax_ref(scale * <q[row], k[col] + e> + bias), .) applied to v[col] + e, written per entry, through torch autograd on the
CPU.  Loss L = <out, G>.  Pricing is parity.check_autograd, unchanged: out by close_fwd, dq, dk, dv, de and, where there is a bias, db by
close_grad.  `cases()` lists every case; tests/test_dot_attention_edge_abi.py rehearses each on the CPU with the fp32 ground-truth run
standing in for the device, tests/test_gpu_dot_attention_edge.py runs them on the device."""
import torch

import dot_attention_bias_case as biased
import dot_attention_case as base
from dot_attention_bias_case import MASK, _masked, first_of_row  # noqa: F401
from dot_attention_case import LANE_SHAPES
from edge_softmax_case import edge_softmax_ref
from pattern_case import OpCase, seeded
from pattern_graphs import _coo
from spmm_case import f32, normal, spmm_ref

EDGE_DIM = 6           # columns of the module case's edge_attr
MAX_E_FLOATS = 1 << 23


def edge_scores(row, col, q, k, e, scale, bias=None):
    s = (q[row] * (k[col] + e)).sum(-1) * scale
    if bias is not None:
        s = s + (bias[:, None] if bias.dim() < s.dim() else bias)
    return s


def edge_ref(row, col, n_rows, q, k, v, e, scale, bias=None):
    """The op per entry: the softmax of every row over scale <q_i, k_j + e_c> (+ bias_c), times v_j + e_c."""
    alpha = edge_softmax_ref(row, n_rows, edge_scores(row, col, q, k, e, scale, bias))
    return spmm_ref(row, torch.arange(row.numel()), n_rows, alpha, v[col] + e)


def composed_ref(row, col, n_rows, q, k, v, e, scale, bias=None):
    """The chain of parts a user would write without the fused op: two score terms, a softmax, an SpMM and a scatter of alpha e."""
    s = base.edge_dot_ref(row, col, q, k, scale) + scale * (q[row] * e).sum(-1)
    if bias is not None:
        s = s + (bias[:, None] if bias.dim() < s.dim() else bias)
    alpha = edge_softmax_ref(row, n_rows, s)
    return spmm_ref(row, col, n_rows, alpha, v) + torch.zeros_like(q).index_add(0, row, alpha[..., None] * e)


class EdgeCase(OpCase):
    """`inner` (a dot_attention_case.Case: entries, q, k, v, G, scale, kind) with `e` [E, H, F] | [E, F] and, optionally, `bias`
    [E, H] | [E]; masked: bool [E], the entries whose bias is MASK in every head, or None.  `e` is given as a function that makes
    it: it is drawn again from its seed wherever it is asked for, so the cases together do not hold every e at once."""
    op = "dot_attention_edge"

    def __init__(self, name, inner, make_e, bias=None, masked=None):
        self.name, self.inner, self.make_e, self.bias, self.masked = name, inner, make_e, bias, masked
        e = make_e()
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "q", "k", "v", "G", "scale", "fed_scale"):
            setattr(self, attr, getattr(inner, attr))
        assert tuple(e.shape) == (self.row.numel(),) + tuple(self.q.shape[1:]) and torch.equal(f32(e), e)
        assert e.numel() <= MAX_E_FLOATS, (name, e.numel())
        assert bias is None or (torch.equal(f32(bias), bias) and bias.shape in ((self.row.numel(), self.H), (self.row.numel(),)))
        self.names = ["dq", "dk", "dv", "de"] + ([] if bias is None else ["db"])

    @property
    def e(self):
        return self.make_e()

    @property
    def leaves(self):
        return [self.q, self.k, self.v, self.e] + ([] if self.bias is None else [self.bias])

    def ref(self, q, k, v, e, b=None):
        return edge_ref(self.row, self.col, self.shape[0], q, k, v, e, self.scale, b).reshape(-1)

    def composed(self, q, k, v, e, b=None):
        return composed_ref(self.row, self.col, self.shape[0], q, k, v, e, self.scale, b).reshape(-1)

    def key_terms(self, dtype=torch.float64):
        """(scale <q_i, k_j>, scale <q_i, e_c>) [E, H]: the two parts of the score."""
        q, k, e = (t.to(dtype) for t in (self.q, self.k, self.e))
        return (q[self.row] * k[self.col]).sum(-1) * self.scale, (q[self.row] * e).sum(-1) * self.scale

    def coefficients(self, dtype=torch.float64):
        b = None if self.bias is None else self.bias.to(dtype)
        s = edge_scores(self.row, self.col, self.q.to(dtype), self.k.to(dtype), self.e.to(dtype), self.scale, b)
        return edge_softmax_ref(self.row, self.shape[0], s)

    def check_masked(self, res):
        """de (every element) and db at a masked entry are exact zeros: both p and ds are 0 there."""
        if self.masked is not None:
            de, db = res[4].detach().cpu(), res[5].detach().cpu()
            assert float(de[self.masked].abs().max()) == 0.0, f"{self.name}: de at a masked entry is an exact zero"
            assert float(db[self.masked].abs().max()) == 0.0, f"{self.name}: db at a masked entry is an exact zero"
            assert float(de[~self.masked].abs().max()) > 0.0

    def rehearse(self):
        res = self.stand_in()
        self.check_masked(res)
        return self.price(*res)


class ComposedEdgeCase(EdgeCase):
    """The fused op against the chain of parts, both priced against the fused op's ground truth."""

    def rehearse(self):
        self.price(*self.stand_in(), what=self.name + " fused")
        return self.price(*self.stand_in(self.composed), what=self.name + " from parts")


class EdgeModuleCase(base.ModuleCase):
    """The AttentionModule of dot_attention_case with e = lin_edge(edge_attr).view(E, H, F), edge_attr [E, EDGE_DIM] seeded: out and
    the gradients reaching x, the three weights and lin_edge.weight, against the same module with the ground truth as `attend`."""
    op = "module_edge"
    NAMES, GRADS = base.ModuleCase.NAMES + ("lin_edge.weight",), base.ModuleCase.GRADS + ("dWe",)

    def __init__(self, name, row, col, N, seed, kind="graph", csr=None):
        self.edge_attr = f32(normal((row.numel(), EDGE_DIM), seed + 7))
        super().__init__(name, row, col, N, seed, kind=kind, csr=csr)

    def module(self, attend):
        case = self

        class WithEdges(base.AttentionModule):
            def __init__(self):
                super().__init__(case.F_IN, case.H, case.F, attend, case.seed + 1)
                self.lin_edge = torch.nn.Linear(EDGE_DIM, case.H * case.F, bias=False)
                self.register_buffer("edge_attr", case.edge_attr.float())
                with torch.no_grad():
                    w = torch.randn(case.H * case.F, EDGE_DIM, generator=torch.Generator().manual_seed(case.seed + 2))
                    self.lin_edge.weight.copy_(w * (2.0 / (EDGE_DIM + case.F)) ** 0.5)

            def forward(self, x):
                q, k, v = (lin(x).view(-1, self.H, self.F) for lin in (self.query, self.key, self.value))
                e = self.lin_edge(self.edge_attr.to(x.dtype)).view(-1, self.H, self.F)
                return self.attend(q, k, v, e)
        return WithEdges()

    def ref_attend(self, q, k, v, e):
        return edge_ref(self.row, self.col, self.shape[0], q, k, v, e, self.scale)


def _e(inner, seed, std=1.0):
    shape = (inner.row.numel(),) + tuple(inner.q.shape[1:])
    return lambda: f32(std * normal(shape, seed))


def _zero_e(inner):
    shape = (inner.row.numel(),) + tuple(inner.q.shape[1:])
    return lambda: torch.zeros(shape, dtype=torch.float64)


def _build_cases():
    out = []
    hub = base._hub_graph()
    row, col, N = _coo(hub)
    asym = base._asym_graph()
    arow, acol, aN = _coo(asym)

    def seed():
        return 40000 + 10 * len(out)

    def add(name, inner, std=1.0, bias=None, masked=False, cls=EdgeCase):
        """bias: None | "heads" ([E, H]) | "shared" ([E])."""
        b = which = None
        if bias is not None:
            b = biased._bias(inner.row.numel(), inner.H, seed() + 5, shared=bias == "shared")
            if masked:
                b, which = _masked(b, inner.row, seed() + 6)
        out.append(cls(name, inner, _e(inner, seed() + 4, std), b, which))
        return out[-1]

    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            add(f"lanes-hub-{H}x{F}-{kind}", base.Case("", row, col, (N, N), H, F, seed(), kind=kind, csr=hub))
    for H, F in ((3, 8), (8, 16), (12, 64)):
        add(f"lanes-asym-{H}x{F}-indices", base.Case("", arow, acol, (aN, aN), H, F, seed()))
    add("lanes-hub-noaxis-indices", base.Case("", row, col, (N, N), 1, 16, seed(), heads=False))
    add("lanes-hub-noaxis-graph", base.Case("", row, col, (N, N), 1, 64, seed(), kind="graph", heads=False, csr=hub))
    add("bias-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), bias="heads")
    add("bias-hub-3x8-graph", base.Case("", row, col, (N, N), 3, 8, seed(), kind="graph", csr=hub), bias="heads")
    add("bias-shared-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), bias="shared")
    add("masked-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), bias="heads", masked=True)
    for pname, builder in (("nine_hubs", base.nine_hubs), ("three_chunk_hub", base.three_chunk_hub)):
        lcsr = builder()
        lrow, lcol, lN = _coo(lcsr)
        for H, F in ((8, 16), (3, 8)):
            for kind in ("indices", "graph"):
                add(f"long-{pname}-{H}x{F}-{kind}", base.Case("", lrow, lcol, (lN, lN), H, F, seed(), kind=kind, csr=lcsr), std=3.0)
    rrow, rcol = base._rect_coo()
    add("rect-3x8", base.Case("", rrow, rcol, (300, 500), 3, 8, seed()))
    add("rect-4x16", base.Case("", rrow, rcol, (300, 500), 4, 16, seed()))
    prow, pcol, pN, pairs = base._repeat_coo()
    add("repeats-8x16", base.Case("", prow, pcol, (pN, pN), 8, 16, seed())).pairs = pairs
    lonely = base.lonely_hub_graph()
    orow, ocol, oN = _coo(lonely)
    for H, F in ((8, 16), (3, 8)):
        for kind in ("indices", "graph"):
            add(f"lonely-{H}x{F}-{kind}", base.Case("", orow, ocol, (oN, oN), H, F, seed(), kind=kind, csr=lonely))
    for name in ("twice-nine_hubs-8x16-indices", "lanes-hub-12x64-indices", "lanes-hub-3x8-graph"):      # the plain file's own cases
        inner = base.cases()[name]
        out.append(EdgeCase("zero-" + name, inner, _zero_e(inner)))
    bc = biased.cases()["lanes-hub-8x16-indices"]                                                        # ... and one of the bias file's
    out.append(EdgeCase("zero-bias-lanes-hub-8x16-indices", bc.inner, _zero_e(bc.inner), bc.bias))
    ncsr = base.nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    add("twice-nine_hubs-8x16-indices", base.Case("", nrow, ncol, (nN, nN), 8, 16, seed()), std=3.0, bias="heads")
    add("twice-hub-3x8-graph", base.Case("", row, col, (N, N), 3, 8, seed(), kind="graph", csr=hub))
    add("composed-hub-8x16-graph", base.Case("", row, col, (N, N), 8, 16, seed(), kind="graph", csr=hub), cls=ComposedEdgeCase)
    add("composed-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed(), scale="sharp"), bias="heads", cls=ComposedEdgeCase)
    out.append(EdgeModuleCase("module-hub-4x16-graph", row, col, N, seed(), csr=hub))
    return out


cases, case_names = seeded(_build_cases)
