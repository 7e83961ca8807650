"""The seeded cases of pygat_amd.dot_attention_dropout (the DROP instantiations of csrc/k19_dot_attention.hip,
pygat_amd/dot_attention.py): dot_attention with seeded dropout on the softmax coefficients.

Patterns, inputs and the ground truth's parts come from dot_attention_case.py and dot_attention_bias_case.py by import; a case here
wraps one of the former's `Case`s and adds p, the seed of the mask and, optionally, a bias ([E, H] or [E]).  The mask is
philox_ref.flat_mask(seed, STREAM_ATT, E * H, p).reshape(E, H) -- NumPy, no device -- at the caller's entry index.  Ground truth is

    spmm_ref(edge_softmax_ref(scale * <q_i, k_j> + bias) * mask, v)

through torch autograd on the CPU: the softmax over ALL entries of a row, the mask after it.  Loss L = <out, G>.  Pricing is
parity.check_autograd, unchanged: out by close_fwd, dq, dk, dv (and db) by close_grad, i.e. max(1e-5, 4 x the fp32 ground-truth run's
own error).  `cases()` lists every case; tests/test_dot_attention_dropout_abi.py rehearses each on the CPU with the fp32 ground-truth
run standing in for the device, tests/test_gpu_dot_attention_dropout.py runs them on the device."""
import numpy as np
import torch

import dot_attention_bias_case as biased
import dot_attention_case as base
import philox_ref
from dot_attention_case import LANE_SHAPES, edge_dot_ref
from edge_softmax_case import edge_softmax_ref
from pattern_case import DropoutChecks, OpCase, seeded
from pattern_graphs import _coo
from spmm_case import f32, normal, spmm_ref

STREAM_ATT = 3                      # pygat_amd.dropout.STREAM_ATT (asserted by the CPU tests): the stream of the attention mask
P_NEAR_0 = 2.0 ** -33               # keep threshold 0xFFFFFFFF and a factor of 1.0f: everything but a word of 0xFFFFFFFF is kept as it is
MASK = biased.MASK


def flat_words(seed, count):
    """uint32 [count]: the words the flat layout draws for elements 0..count-1 on STREAM_ATT (philox_ref's flat counters)."""
    q = np.arange((count + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, STREAM_ATT), np.full_like(q, 0xFFFFFFFF)], axis=-1)
    return philox_ref.philox4x32_10(ctr, philox_ref._key(seed)).reshape(-1)[:count]


def dropout_ref(row, col, n_rows, q, k, v, scale, bias, mask):
    """mask [E, H] (or [E] without a head axis), pre-scaled, any dtype: cast to the scores'."""
    s = edge_dot_ref(row, col, q, k, scale)
    if bias is not None:
        s = s + (bias[:, None] if bias.dim() < s.dim() else bias)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s) * mask.to(s.dtype).reshape(s.shape), v)


class DropCase(DropoutChecks, OpCase):
    """`inner` (a dot_attention_case.Case: entries, q, k, v, G, scale, kind) under dropout p with the mask of `seed`; bias: None,
    [E, H] or [E]; masked: bool [E], the entries whose bias is MASK, or None."""
    op = "dot_attention_dropout"

    def __init__(self, name, inner, p, seed, bias=None, masked=None):
        self.name, self.inner, self.p, self.seed, self.bias, self.masked = name, inner, p, seed, bias, masked
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "q", "k", "v", "G", "scale", "fed_scale"):
            setattr(self, attr, getattr(inner, attr))
        E = self.row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))      # float32 [E, H]
        assert bias is None or (bias.shape in ((E, self.H), (E,)) and (self.q.dim() == 3 or bias.dim() == 1))
        assert bias is None or torch.equal(f32(bias), bias)

    @property
    def leaves(self):
        return [self.q, self.k, self.v] + ([] if self.bias is None else [self.bias])

    @property
    def names(self):
        return ["dq", "dk", "dv"] + ([] if self.bias is None else ["db"])

    def ref(self, q, k, v, b=None):
        return dropout_ref(self.row, self.col, self.shape[0], q, k, v, self.scale, b, self.mask).reshape(-1)

    def scores(self, dtype=torch.float64):
        """The scores [E, H] the softmax of the ground truth runs over (the bias included)."""
        s = edge_dot_ref(self.row, self.col, self.q.to(dtype), self.k.to(dtype), self.scale).reshape(self.row.numel(), self.H)
        if self.bias is not None:
            s = s + self.bias.to(dtype).reshape(self.row.numel(), -1)
        return s

    def check_masked(self, db):
        if self.masked is not None:
            assert float(db.detach().cpu()[self.masked].abs().max()) == 0.0, f"{self.name}: db at a masked entry is an exact zero"

    def rehearse(self):
        res = self.stand_in()
        self.check_all_dropped(res[0])
        if self.bias is not None:
            self.check_masked(res[4])
        return self.price(*res)


class DropModuleCase(biased.BiasModuleCase):
    """dot_attention_bias_case's module (three nn.Linear projections, bias = nn.Embedding(edge_type)) with the new op as `attend`:
    out and the gradients reaching x, the three weights and the embedding table, against the module with the ground truth, in fp64."""
    op = "module_dropout"

    def __init__(self, name, row, col, N, seed, p, kind="graph", csr=None):
        super().__init__(name, row, col, N, seed, kind=kind, csr=csr)
        self.p, self.mask_seed = p, seed + 11
        E = row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(self.mask_seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))

    def ref_attend(self, q, k, v, b):
        return dropout_ref(self.row, self.col, self.shape[0], q, k, v, self.scale, b, self.mask)


def one_entry_rows(N=300, M=400, seed=77):
    """(row, col): exactly one entry per row of a [N x M] pattern, the rows in a seeded shuffle -- unsorted, so only the permutation
    finds an entry's index -- and the columns seeded with repeats."""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(N, generator=g), torch.randint(0, M, (N,), generator=g)


def _build_cases():
    out = []
    hub = base._hub_graph()
    row, col, N = _coo(hub)
    asym = base._asym_graph()
    arow, acol, aN = _coo(asym)

    def seed():
        return 40000 + 10 * len(out)

    def add(name, inner, p=0.5, bias=None, masked=False, std=1.0):
        b = which = None
        if bias is not None:
            b = biased._bias(inner.row.numel(), inner.H, seed() + 4, std=std, shared=bias == "shared" or inner.q.dim() == 2)
            if masked:
                b, which = biased._masked(b, inner.row, seed() + 5)
        out.append(DropCase(name, inner, p, seed() + 6, b, which))
        return out[-1]

    # every lane shape, with and without a permutation, with and without a [E, H] bias
    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            for bias in (None, "heads"):
                add(f"lanes-hub-{H}x{F}-{kind}-{'bias' if bias else 'plain'}",
                    base.Case("", row, col, (N, N), H, F, seed(), kind=kind, csr=hub), bias=bias)
    for kind, F in (("indices", 16), ("graph", 64)):
        for bias in (None, "shared"):
            add(f"lanes-hub-noaxis-{kind}-{'bias' if bias else 'plain'}",
                base.Case("", row, col, (N, N), 1, F, seed(), kind=kind, heads=False, csr=hub), bias=bias)
    add("lanes-hub-8x16-indices-shared", base.Case("", row, col, (N, N), 8, 16, seed()), bias="shared")
    add("lanes-hub-12x64-graph-shared", base.Case("", row, col, (N, N), 12, 64, seed(), kind="graph", csr=hub), bias="shared")
    for H, F in ((3, 8), (8, 16), (12, 64)):
        add(f"lanes-asym-{H}x{F}-indices-plain", base.Case("", arow, acol, (aN, aN), H, F, seed()))
        add(f"lanes-asym-{H}x{F}-graph-bias", base.Case("", arow, acol, (aN, aN), H, F, seed(), kind="graph", csr=asym), bias="heads")
    # long rows: scores of std 3, p = 0.5 and 0.9
    ncsr, tcsr = base.nine_hubs(), base.three_chunk_hub()
    nrow, ncol, nN = _coo(ncsr)
    trow, tcol, tN = _coo(tcsr)
    for p in (0.5, 0.9):
        add(f"long-nine_hubs-8x16-graph-p{p}", base.Case("", nrow, ncol, (nN, nN), 8, 16, seed(), kind="graph", scale="sharp", csr=ncsr), p=p)
        add(f"long-nine_hubs-3x8-indices-bias-p{p}", base.Case("", nrow, ncol, (nN, nN), 3, 8, seed(), scale="sharp"), p=p, bias="heads")
        add(f"long-three_chunk_hub-3x8-graph-p{p}", base.Case("", trow, tcol, (tN, tN), 3, 8, seed(), kind="graph", scale="sharp", csr=tcsr),
            p=p)
    add("long-three_chunk_hub-8x16-indices-bias-p0.5", base.Case("", trow, tcol, (tN, tN), 8, 16, seed(), scale="sharp"), bias="heads")
    add("long-nine_hubs-12x64-graph-bias-p0.9", base.Case("", nrow, ncol, (nN, nN), 12, 64, seed(), kind="graph", scale="sharp", csr=ncsr),
        p=0.9, bias="heads")
    # rectangular, unsorted, repeats
    rrow, rcol = base._rect_coo()
    add("rect-3x8-plain", base.Case("", rrow, rcol, (300, 500), 3, 8, seed()))
    add("rect-4x16-bias", base.Case("", rrow, rcol, (300, 500), 4, 16, seed()), bias="heads")
    prow, pcol, pN, pairs = base._repeat_coo()
    add("repeats-8x16-plain", base.Case("", prow, pcol, (pN, pN), 8, 16, seed())).pairs = pairs
    # rows whose entries are all dropped: p = 0.9 on the asymmetric pattern, whose rows are short
    add("gone-asym-8x16-indices-plain", base.Case("", arow, acol, (aN, aN), 8, 16, seed()), p=0.9)
    add("gone-asym-3x8-graph-bias", base.Case("", arow, acol, (aN, aN), 3, 8, seed(), kind="graph", csr=asym), p=0.9, bias="heads")
    # -9e15 on a third of the entries, and dropout on top
    add("masked-hub-8x16-indices", base.Case("", row, col, (N, N), 8, 16, seed()), bias="heads", masked=True)
    add("masked-three_chunk_hub-3x8-graph", base.Case("", trow, tcol, (tN, tN), 3, 8, seed(), kind="graph", csr=tcsr), bias="heads",
        masked=True)
    add("masked-rect-3x8", base.Case("", rrow, rcol, (300, 500), 3, 8, seed()), p=0.9, bias="heads", masked=True)
    # exactly one entry per row
    orow, ocol = one_entry_rows()
    for H, F in ((8, 16), (3, 8), (12, 64)):
        add(f"single-{H}x{F}", base.Case("", orow, ocol, (300, 400), H, F, seed()))
    add("single-8x16-bias", base.Case("", orow, ocol, (300, 400), 8, 16, seed()), bias="heads")
    # p next to 0: everything is kept, by the DROP kernels
    add("near0-hub-8x16-indices-plain", base.Case("", row, col, (N, N), 8, 16, seed()), p=P_NEAR_0)
    add("near0-hub-12x64-graph-bias", base.Case("", row, col, (N, N), 12, 64, seed(), kind="graph", csr=hub), p=P_NEAR_0, bias="heads")
    add("twice-nine_hubs-8x16-indices-bias", base.Case("", nrow, ncol, (nN, nN), 8, 16, seed(), scale="sharp"), bias="heads", std=3.0)
    add("twice-hub-3x8-graph-plain", base.Case("", row, col, (N, N), 3, 8, seed(), kind="graph", csr=hub))
    add("composed-hub-8x16-graph-bias", base.Case("", row, col, (N, N), 8, 16, seed(), kind="graph", csr=hub), bias="heads")
    add("composed-hub-8x16-indices-plain", base.Case("", row, col, (N, N), 8, 16, seed(), scale="sharp"))
    add("capture-hub-8x16-indices-bias", base.Case("", row, col, (N, N), 8, 16, seed()), bias="heads")
    out.append(DropModuleCase("module-hub-4x16-graph", row, col, N, seed(), 0.5, csr=hub))
    return out


cases, case_names = seeded(_build_cases)
