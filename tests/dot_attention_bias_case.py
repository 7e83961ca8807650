"""The seeded cases of pygat_amd.dot_attention with a per-entry bias on the score (the BIAS instantiations of
csrc/k19_dot_attention.hip, pygat_amd/dot_attention.py).

Patterns, inputs, the ground truth's parts and the module come from dot_attention_case.py by import; a case here wraps one of its
`Case`s and adds the bias ([E, H], or [E]: shared by the heads, or all there is without a head axis), seeded, fp32-rounded and fed
identically to the device and to both ground-truth runs.  Ground truth is dot_attention_ref with `+ bias` on the scores, through
torch autograd on the CPU.  Loss L = <out, G>.  Pricing is parity.check_autograd, unchanged: out by close_fwd, dq, dk, dv and db (the
gradient of the bias, a fourth leaf) by close_grad.  `cases()` lists every case; tests/test_dot_attention_bias_abi.py rehearses each
on the CPU with the fp32 ground-truth run standing in for the device, tests/test_gpu_dot_attention_bias.py runs them on the device."""
import torch

import dot_attention_case as base
from dot_attention_case import LANE_SHAPES, edge_dot_ref
from edge_softmax_case import edge_softmax_ref
from pattern_case import OpCase, seeded
from pattern_graphs import _coo
from spmm_case import f32, normal, spmm_ref

MASK = float(torch.tensor(-9e15).float())      # the reference's own "no edge here" as fp32 holds it: finite, exp(MASK - m) an exact zero
N_TYPES = 5


def biased_ref(row, col, n_rows, q, k, v, scale, bias):
    """dot_attention_ref with the bias on the scores; bias [E] is shared by the heads of a [E, H] score."""
    s = edge_dot_ref(row, col, q, k, scale)
    s = s + (bias[:, None] if bias.dim() < s.dim() else bias)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s), v)


def first_of_row(row):
    """bool [E]: the entry is the first of its row in the caller's order."""
    E = row.numel()
    first = torch.full((int(row.max()) + 1,), E, dtype=torch.long).scatter_reduce(0, row, torch.arange(E), "amin")
    return first[row] == torch.arange(E)


class BiasCase(OpCase):
    """`inner` (a dot_attention_case.Case: entries, q, k, v, G, scale, kind) with `bias` [E, H] | [E]; masked: bool [E], the entries
    whose bias is MASK in every head, or None."""
    op = "dot_attention_bias"

    def __init__(self, name, inner, bias, masked=None):
        self.name, self.inner, self.bias, self.masked = name, inner, bias, masked
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "q", "k", "v", "G", "scale", "fed_scale"):
            setattr(self, attr, getattr(inner, attr))
        assert bias.shape in ((self.row.numel(), self.H), (self.row.numel(),)) and (self.q.dim() == 3 or bias.dim() == 1)
        assert torch.equal(f32(bias), bias)

    names = ["dq", "dk", "dv", "db"]

    @property
    def leaves(self):
        return [self.q, self.k, self.v, self.bias]

    def ref(self, q, k, v, b):
        return biased_ref(self.row, self.col, self.shape[0], q, k, v, self.scale, b).reshape(-1)

    def coefficients(self, dtype=torch.float64):
        """The softmax coefficients [E, H] of the ground truth."""
        s = edge_dot_ref(self.row, self.col, self.q.to(dtype), self.k.to(dtype), self.scale)
        b = self.bias.to(dtype)
        s = s + (b[:, None] if b.dim() < s.dim() else b)
        return edge_softmax_ref(self.row, self.shape[0], s)

    def db_row_sums(self, db):
        """The sums of db over the entries of every row, [n_rows, H] in fp64 on the host (0 in exact arithmetic: the coefficients of
        a row add up to 1 whatever is added to all of its scores)."""
        d = db.detach().double().cpu().reshape(self.row.numel(), -1)
        return torch.zeros(self.shape[0], d.shape[1], dtype=torch.float64).index_add(0, self.row, d)

    def check_masked(self, db):
        if self.masked is not None:
            assert float(db.detach().cpu()[self.masked].abs().max()) == 0.0, f"{self.name}: db at a masked entry is an exact zero"

    def rehearse(self):
        res = self.stand_in()
        self.check_masked(res[4])
        return self.price(*res)


class BiasModuleCase(base.ModuleCase):
    """The AttentionModule of dot_attention_case with bias = emb(edge_type), emb an nn.Embedding(N_TYPES, H), the per-entry types
    seeded: out and the gradients reaching x, the three weights and the embedding table, against the same module with the ground
    truth as `attend`, in fp64."""
    op = "module_bias"
    NAMES, GRADS = base.ModuleCase.NAMES + ("emb.weight",), base.ModuleCase.GRADS + ("dEmb",)

    def __init__(self, name, row, col, N, seed, kind="graph", csr=None):
        self.types = torch.randint(0, N_TYPES, (row.numel(),), generator=torch.Generator().manual_seed(seed + 7))
        super().__init__(name, row, col, N, seed, kind=kind, csr=csr)

    def module(self, attend):
        case = self

        class Biased(base.AttentionModule):
            def __init__(self):
                super().__init__(case.F_IN, case.H, case.F, attend, case.seed + 1)
                self.emb = torch.nn.Embedding(N_TYPES, case.H)
                self.register_buffer("types", case.types.clone())
                with torch.no_grad():
                    self.emb.weight.copy_(torch.randn(N_TYPES, case.H, generator=torch.Generator().manual_seed(case.seed + 2)))

            def forward(self, x):
                q, k, v = (lin(x).view(-1, self.H, self.F) for lin in (self.query, self.key, self.value))
                return self.attend(q, k, v, self.emb(self.types))
        return Biased()

    def ref_attend(self, q, k, v, b):
        return biased_ref(self.row, self.col, self.shape[0], q, k, v, self.scale, b)


def _bias(E, H, seed, std=1.0, shared=False):
    return f32(std * normal((E,) if shared else (E, H), seed))


def _masked(bias, row, seed):
    """-> (bias with MASK on a seeded third of the entries, never on the first entry of a row in the caller's order; which)."""
    which = (torch.rand(row.numel(), generator=torch.Generator().manual_seed(seed)) < 1.0 / 3.0) & ~first_of_row(row)
    bias = bias.clone()
    bias[which] = MASK
    return bias, which


def _build_cases():
    out = []
    hub = base._hub_graph()
    row, col, N = _coo(hub)
    E = row.numel()
    asym = base._asym_graph()
    arow, acol, aN = _coo(asym)

    def seed():
        return 20000 + 10 * len(out)

    def add(name, inner, **kw):
        masked, shared = kw.pop("masked", False), kw.pop("shared", False)
        bias = _bias(inner.row.numel(), inner.H, seed() + 4, shared=shared or inner.q.dim() == 2, **kw)
        which = None
        if masked:
            bias, which = _masked(bias, inner.row, seed() + 5)
        out.append(BiasCase(name, inner, bias, which))
        return out[-1]

    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            add(f"lanes-hub-{H}x{F}-{kind}", base.Case("", row, col, (N, N), H, F, seed(), kind=kind, csr=hub))
    for H, F in ((3, 8), (8, 16), (12, 64)):
        add(f"lanes-asym-{H}x{F}-indices", base.Case("", arow, acol, (aN, aN), H, F, seed()))
    add("lanes-hub-noaxis-indices", base.Case("", row, col, (N, N), 1, 16, seed(), heads=False))
    add("lanes-hub-noaxis-graph", base.Case("", row, col, (N, N), 1, 64, seed(), kind="graph", heads=False, csr=hub))
    add("shared-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), shared=True)
    add("shared-hub-3x8-graph", base.Case("", row, col, (N, N), 3, 8, seed(), kind="graph", csr=hub), shared=True)
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
    add("masked-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), masked=True)
    tcsr = base.three_chunk_hub()
    trow, tcol, tN = _coo(tcsr)
    add("masked-three_chunk_hub-3x8-graph", base.Case("", trow, tcol, (tN, tN), 3, 8, seed(), kind="graph", csr=tcsr), masked=True)
    add("masked-rect-3x8", base.Case("", rrow, rcol, (300, 500), 3, 8, seed()), masked=True)
    lonely = base.lonely_hub_graph()
    orow, ocol, oN = _coo(lonely)
    for H, F in ((8, 16), (3, 8)):
        for kind in ("indices", "graph"):
            add(f"lonely-{H}x{F}-{kind}", base.Case("", orow, ocol, (oN, oN), H, F, seed(), kind=kind, csr=lonely))
    for name in ("twice-nine_hubs-8x16-indices", "lanes-hub-12x64-indices", "lanes-hub-3x8-graph"):      # the unbiased file's own cases
        inner = base.cases()[name]
        out.append(BiasCase("zero-" + name, inner, torch.zeros(inner.row.numel(), inner.H, dtype=torch.float64)))
    inner = base.Case("", row, col, (N, N), 8, 16, seed())
    plain = add("shift-hub-8x16-plain", inner)
    c = f32(3.0 * normal((N, 8), seed() + 6))
    out.append(BiasCase("shift-hub-8x16-shifted", inner, f32(plain.bias + c[row])))
    ncsr = base.nine_hubs()
    nrow, ncol, nN = _coo(ncsr)
    add("twice-nine_hubs-8x16-indices", base.Case("", nrow, ncol, (nN, nN), 8, 16, seed()), std=3.0)
    add("twice-hub-3x8-graph", base.Case("", row, col, (N, N), 3, 8, seed(), kind="graph", csr=hub))
    add("composed-hub-8x16-graph", base.Case("", row, col, (N, N), 8, 16, seed(), kind="graph", csr=hub))
    add("composed-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed(), scale="sharp"))
    out.append(BiasModuleCase("module-hub-4x16-graph", row, col, N, seed(), csr=hub))
    assert E == row.numel()
    return out


cases, case_names = seeded(_build_cases)
