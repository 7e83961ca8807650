"""The seeded cases of pygat_amd.gatv2_attention_dropout (the DROP instantiations of the two row passes of
csrc/k21_gatv2_attention.hip, pygat_amd/gatv2_attention.py): gatv2_attention with seeded dropout on the softmax coefficients.

Patterns, inputs and the ground truth's parts come from gatv2_attention_case.py by import; a case here wraps one of its `Case`s and adds
p and the seed of the mask.  The mask is philox_ref.flat_mask(seed, STREAM_ATT, E * H, p).reshape(E, H) -- NumPy, no device -- at the
caller's entry index: the mask of dot_attention_dropout.  Ground truth is

    spmm_ref(edge_softmax_ref((a * leaky_relu(x_dst[row] + x_src[col])).sum(-1)) * mask, v)

through torch autograd on the CPU in fp64: the softmax over ALL entries of a row, the mask after it.  Loss L = <out, G>.  Pricing is
parity.check_autograd, unchanged: out by close_fwd, every gradient by close_grad, i.e. max(1e-5, 4 x the fp32 ground-truth run's own
error).  The LeakyReLU kink is handled as the wrapped case handles it: the tables are the leaves, t is one correctly rounded add, and
the rehearsal asserts t_signs_agree; the module case asserts its band when it is built (and takes the next seed when that fails).
The wrapped cases are the parent file's own wherever it has the pattern and shape, inputs and seeds as they stand there.
`cases()` lists every case; tests/test_gatv2_attention_dropout_abi.py rehearses each on the CPU with the fp32 ground-truth run standing
in for the device, tests/test_gpu_gatv2_attention_dropout.py runs them on the device."""
import torch

import gatv2_attention_case as base
import philox_ref
from additive_attention_dropout_case import _wrapped
from dot_attention_case import LANE_SHAPES, edge_softmax_ref, nine_hubs, spmm_ref, three_chunk_hub
from pattern_case import DropoutChecks, OpCase, seeded
from pattern_graphs import _coo, _rect_coo
from dot_attention_dropout_case import P_NEAR_0, one_entry_rows
from gatv2_attention_case import scores, t_signs_agree

STREAM_ATT = 3                      # pygat_amd.dropout.STREAM_ATT (asserted by the CPU tests): the stream of the attention mask


def dropout_ref(row, col, n_rows, x_dst, x_src, a, v, slope, mask):
    """mask [E, H] (or [E] without a head axis), pre-scaled, any dtype: cast to the scores'."""
    s = scores(row, col, x_dst, x_src, a, slope)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, s) * mask.to(s.dtype).reshape(s.shape), v)


class DropCase(DropoutChecks, OpCase):
    """`inner` (a gatv2_attention_case.Case: entries, x_dst, x_src, a, v | shared, G, slope, kind) under dropout p with the mask of
    `seed`."""
    op = "gatv2_attention_dropout"

    def __init__(self, name, inner, p, seed):
        self.name, self.inner, self.p, self.seed = name, inner, p, seed
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "x_dst", "x_src", "a", "v", "G", "slope", "shared", "leaves", "names"):
            setattr(self, attr, getattr(inner, attr))
        E = self.row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))      # float32 [E, H]

    def ref(self, x_dst, x_src, a, v=None):
        return dropout_ref(self.row, self.col, self.shape[0], x_dst, x_src, a, x_src if v is None else v, self.slope,
                           self.mask).reshape(-1)

    def rehearse(self):
        assert t_signs_agree(self.row, self.col, self.x_dst, self.x_src), self.name
        res = self.stand_in()
        self.check_all_dropped(res[0])
        return self.price(*res)


class DropModuleCase(base.ModuleCase):
    """gatv2_attention_case's BipartiteGATv2 with the new op as `attend`: out and the gradients reaching x_src, x_dst, W_l, W_r and a,
    against the module with the ground truth, in fp64."""
    op = "module_dropout"

    def __init__(self, name, row, col, shape, seed, p, kind="indices", csr=None):
        super().__init__(name, row, col, shape, seed, kind=kind, csr=csr)
        self.p, self.mask_seed = p, seed + 11
        E = row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(self.mask_seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))

    def ref_attend(self, h_dst, h_src, a):
        return dropout_ref(self.row, self.col, self.shape[0], h_dst, h_src, a, h_src, self.slope, self.mask)


def _build_cases():
    """Wherever gatv2_attention_case.py has the case -- pattern, lane shape, kind and v -- it is wrapped as it stands, inputs and seed
    included: what the op without dropout is priced on.  A new inner case is built only where the parent has none (12 x 64 on the long
    rows, one entry per row), on a seed that follows from its place in the list."""
    out = []
    parent = base.cases()

    def seed():
        return 60000 + 10 * len(out)

    def wrap(name, inner, p=0.5):
        out.append(DropCase(name, parent[inner], p, seed() + 6))
        return out[-1]

    def add(name, row, col, shape, H, F, p=0.5, **kw):
        out.append(DropCase(name, base.Case("", row, col, shape, H, F, seed(), **kw), p, seed() + 6))
        return out[-1]

    # every lane shape, with and without a permutation, v shared and separate
    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            for v in ("shared", "separate"):
                wrap(f"lanes-hub-{H}x{F}-{kind}-{v}", f"lanes-hub-{H}x{F}-{kind}-{v}")
    wrap("lanes-hub-noaxis-graph-separate", "lanes-hub-noaxis-graph-separate")
    for H, F in ((3, 8), (8, 16), (12, 64)):
        wrap(f"lanes-asym-{H}x{F}-indices-shared", f"lanes-asym-{H}x{F}-indices-shared")
        wrap(f"lanes-asym-{H}x{F}-graph-separate", f"lanes-asym-{H}x{F}-graph-separate")
    wrap("lanes-asym-8x16-indices-separate", "lanes-asym-8x16-indices-separate")
    # long rows: scores of std 3, p = 0.5 and 0.9
    ncsr, tcsr = nine_hubs(), three_chunk_hub()
    nrow, ncol, nN = _coo(ncsr)
    trow, tcol, tN = _coo(tcsr)
    for p in (0.5, 0.9):
        wrap(f"long-nine_hubs-8x16-graph-separate-p{p}", "long-nine_hubs-8x16-graph-separate", p)
        wrap(f"long-nine_hubs-3x8-indices-shared-p{p}", "long-nine_hubs-3x8-indices-shared", p)
        wrap(f"long-three_chunk_hub-3x8-graph-separate-p{p}", "long-three_chunk_hub-3x8-graph-separate", p)
        add(f"long-three_chunk_hub-12x64-indices-shared-p{p}", trow, tcol, (tN, tN), 12, 64, p=p, std=3.0)
    wrap("long-three_chunk_hub-8x16-indices-shared-p0.5", "long-three_chunk_hub-8x16-indices-shared")
    add("long-nine_hubs-12x64-graph-separate-p0.9", nrow, ncol, (nN, nN), 12, 64, p=0.9, kind="graph", csr=ncsr, std=3.0, shared=False)
    # rectangular, unsorted, repeats
    wrap("rect-4x16-shared", "rect-4x16-shared")
    wrap("rect-3x8-separate", "rect-3x8-separate")
    wrap("repeats-8x16-shared", "repeats-8x16-shared").pairs = parent["repeats-8x16-shared"].pairs
    wrap("repeats-8x16-separate", "repeats-8x16-separate").pairs = parent["repeats-8x16-separate"].pairs
    # rows whose entries are all dropped: p = 0.9 on the asymmetric pattern, whose rows are short
    wrap("gone-asym-8x16-indices-shared", "lanes-asym-8x16-indices-shared", 0.9)
    wrap("gone-asym-3x8-graph-separate", "lanes-asym-3x8-graph-separate", 0.9)
    # exactly one entry per row
    orow, ocol = one_entry_rows()
    for H, F in ((8, 16), (3, 8), (12, 64)):
        add(f"single-{H}x{F}-separate", orow, ocol, (300, 400), H, F, shared=False)
    add("single-8x16-shared", orow, ocol, (300, 400), 8, 16)
    # p next to 0: everything is kept, by the DROP kernels
    wrap("near0-hub-8x16-indices-shared", "lanes-hub-8x16-indices-shared", P_NEAR_0)
    wrap("near0-hub-12x64-graph-separate", "lanes-hub-12x64-graph-separate", P_NEAR_0)
    wrap("twice-hub-12x64-indices-separate", "twice-hub-12x64-indices-separate")
    wrap("twice-hub-3x8-graph-shared", "twice-hub-3x8-graph-shared")
    wrap("composed-hub-8x16-graph-shared", "composed-hub-8x16-graph-shared")
    wrap("composed-hub-8x16-indices-separate", "composed-hub-8x16-indices-separate")
    wrap("capture-hub-8x16-indices-shared", "lanes-hub-8x16-indices-shared")
    rrow, rcol = _rect_coo()
    out.append(_wrapped(lambda s: DropModuleCase("module-rect-2x8", rrow, rcol, (300, 500), s, 0.5), seed()))
    return out


cases, case_names = seeded(_build_cases)
