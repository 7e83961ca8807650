"""The seeded cases of pygat_amd.additive_attention_dropout (the DROP instantiations of csrc/k20_additive_attention.hip,
pygat_amd/additive_attention.py): additive_attention with seeded dropout on the softmax coefficients.

Patterns, inputs and the ground truth's parts come from additive_attention_case.py by import; a case here wraps one of its `Case`s and
adds p and the seed of the mask.  The mask is philox_ref.flat_mask(seed, STREAM_ATT, E * H, p).reshape(E, H) -- NumPy, no device -- at
the caller's entry index: the mask of dot_attention_dropout.  Ground truth is

    spmm_ref(edge_softmax_ref(leaky_relu((s_dst[row] + s_src[col]) + u)) * mask, v)

through torch autograd on the CPU in fp64: the softmax over ALL entries of a row, the mask after it.  Loss L = <out, G>.  Pricing is
parity.check_autograd, unchanged: out by close_fwd, every gradient by close_grad, i.e. max(1e-5, 4 x the fp32 ground-truth run's own
error).  The LeakyReLU kink is the wrapped case's affair: it asserts, when it is built, that no (entry, head) lies inside the band.  The
wrapped cases are the parent file's own wherever it has the pattern and shape, inputs and seeds as they stand there; the few built here
take the next seed, at most four times, when that assertion fails (nothing here looks at a rehearsal or at a device).
`cases()` lists every case; tests/test_additive_attention_dropout_abi.py rehearses each on the CPU with the fp32 ground-truth run
standing in for the device, tests/test_gpu_additive_attention_dropout.py runs them on the device."""
import torch

import additive_attention_case as base
import philox_ref
from additive_attention_case import SLOPE, logits_z
from dot_attention_case import LANE_SHAPES, edge_softmax_ref, nine_hubs, spmm_ref, three_chunk_hub
from pattern_case import DropoutChecks, OpCase, seeded
from pattern_graphs import _coo, _rect_coo
from dot_attention_dropout_case import P_NEAR_0, one_entry_rows

STREAM_ATT = 3                      # pygat_amd.dropout.STREAM_ATT (asserted by the CPU tests): the stream of the attention mask


def dropout_ref(row, col, n_rows, s_dst, s_src, v, slope, u, mask):
    """mask [E, H] (or [E] without a head axis), pre-scaled, any dtype: cast to the scores'."""
    l = torch.nn.functional.leaky_relu(logits_z(row, col, s_dst, s_src, u), slope)
    return spmm_ref(row, col, n_rows, edge_softmax_ref(row, n_rows, l) * mask.to(l.dtype).reshape(l.shape), v)


class DropCase(DropoutChecks, OpCase):
    """`inner` (an additive_attention_case.Case: entries, s_dst, s_src, v, G, u, slope, kind) under dropout p with the mask of `seed`."""
    op = "additive_attention_dropout"

    def __init__(self, name, inner, p, seed):
        self.name, self.inner, self.p, self.seed = name, inner, p, seed
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "s_dst", "s_src", "v", "G", "u", "slope", "masked", "leaves", "names"):
            setattr(self, attr, getattr(inner, attr))
        E = self.row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))      # float32 [E, H]

    def ref(self, s_dst, s_src, v, u=None):
        return dropout_ref(self.row, self.col, self.shape[0], s_dst, s_src, v, self.slope, u, self.mask).reshape(-1)

    def check_masked(self, du):
        if self.masked is not None:
            assert float(du.detach().cpu()[self.masked].abs().max()) == 0.0, f"{self.name}: du at a masked entry is an exact zero"

    def rehearse(self):
        res = self.stand_in()
        self.check_all_dropped(res[0])
        if self.masked is not None:
            self.check_masked(res[4])
        return self.price(*res)


class DropModuleCase(base.ModuleCase):
    """additive_attention_case's BipartiteGAT with the new op as `attend`: out and the gradients reaching x_src, x_dst, W and a, against
    the module with the ground truth, in fp64."""
    op = "module_dropout"

    def __init__(self, name, row, col, shape, seed, p, kind="indices", csr=None):
        super().__init__(name, row, col, shape, seed, kind=kind, csr=csr)
        self.p, self.mask_seed = p, seed + 11
        E = row.numel()
        self.mask = torch.from_numpy(philox_ref.flat_mask(self.mask_seed, STREAM_ATT, E * self.H, p).reshape(E, self.H))

    def ref_attend(self, s_dst, s_src, v):
        return dropout_ref(self.row, self.col, self.shape[0], s_dst, s_src, v, self.slope, None, self.mask)


def _wrapped(build, seed):
    """build(seed) -> a case that asserts its kink band when it is built; the first of seed, seed + 1, ... that builds."""
    for k in range(5):
        try:
            return build(seed + k)
        except AssertionError as e:
            if "kink band" not in str(e) or k == 4:
                raise


def _build_cases():
    """Wherever additive_attention_case.py has the case -- pattern, lane shape, kind and logit -- it is wrapped as it stands, inputs and
    seed included: what the op without dropout is priced on.  A new inner case is built only where the parent has none (12 x 64 on the
    long rows, one entry per row), on a seed that follows from its place in the list."""
    out = []
    parent = base.cases()

    def seed():
        return 50000 + 10 * len(out)

    def wrap(name, inner, p=0.5):
        out.append(DropCase(name, parent[inner], p, seed() + 6))
        return out[-1]

    def add(name, row, col, shape, H, F, p=0.5, **kw):
        inner = _wrapped(lambda s: base.Case("", row, col, shape, H, F, s, **kw), seed())
        out.append(DropCase(name, inner, p, seed() + 6))
        return out[-1]

    # every lane shape, with and without a permutation, with and without a [E, H] logit
    for H, F in LANE_SHAPES:
        for kind in ("indices", "graph"):
            wrap(f"lanes-hub-{H}x{F}-{kind}-plain", f"lanes-hub-{H}x{F}-{kind}")
            wrap(f"lanes-hub-{H}x{F}-{kind}-logit", f"lanes-hub-{H}x{F}-{kind}-logit")
    wrap("lanes-hub-12x64-indices-shared", "lanes-hub-12x64-indices-shared")
    wrap("lanes-hub-noaxis-graph-logit", "lanes-hub-noaxis-graph-logit")
    for H, F in ((3, 8), (8, 16), (12, 64)):
        wrap(f"lanes-asym-{H}x{F}-indices-plain", f"lanes-asym-{H}x{F}-indices")
        wrap(f"lanes-asym-{H}x{F}-graph-logit", f"lanes-asym-{H}x{F}-graph-logit")
    wrap("lanes-asym-8x16-indices-logit", "lanes-asym-8x16-indices-logit")
    # long rows: scores of std 3, p = 0.5 and 0.9
    ncsr, tcsr = nine_hubs(), three_chunk_hub()
    nrow, ncol, nN = _coo(ncsr)
    trow, tcol, tN = _coo(tcsr)
    for p in (0.5, 0.9):
        wrap(f"long-nine_hubs-8x16-graph-p{p}", "long-nine_hubs-8x16-graph", p)
        wrap(f"long-nine_hubs-3x8-indices-logit-p{p}", "long-nine_hubs-3x8-indices-logit", p)
        wrap(f"long-three_chunk_hub-3x8-graph-p{p}", "long-three_chunk_hub-3x8-graph", p)
        add(f"long-three_chunk_hub-12x64-indices-logit-p{p}", trow, tcol, (tN, tN), 12, 64, p=p, std=3.0, logit="full")
    wrap("long-three_chunk_hub-8x16-graph-shared-p0.5", "long-three_chunk_hub-8x16-graph-shared")
    add("long-nine_hubs-12x64-graph-p0.9", nrow, ncol, (nN, nN), 12, 64, p=0.9, kind="graph", csr=ncsr, std=3.0)
    # rectangular, unsorted, repeats
    wrap("rect-4x16-plain", "rect-4x16")
    wrap("rect-3x8-logit", "rect-3x8-logit")
    wrap("repeats-8x16-plain", "repeats-8x16").pairs = parent["repeats-8x16"].pairs
    wrap("repeats-8x16-logit", "repeats-8x16-logit").pairs = parent["repeats-8x16-logit"].pairs
    # rows whose entries are all dropped: p = 0.9 on the asymmetric pattern, whose rows are short
    wrap("gone-asym-8x16-indices-plain", "lanes-asym-8x16-indices", 0.9)
    wrap("gone-asym-3x8-graph-logit", "lanes-asym-3x8-graph-logit", 0.9)
    # -9e15 on a third of the entries, and dropout on top
    wrap("masked-hub-8x16-indices", "masked-hub-8x16-indices")
    wrap("masked-three_chunk_hub-3x8-graph", "masked-three_chunk_hub-3x8-graph")
    wrap("masked-rect-3x8", "masked-rect-3x8", 0.9)
    # exactly one entry per row
    orow, ocol = one_entry_rows()
    for H, F in ((8, 16), (3, 8), (12, 64)):
        add(f"single-{H}x{F}", orow, ocol, (300, 400), H, F)
    add("single-8x16-logit", orow, ocol, (300, 400), 8, 16, logit="full")
    # p next to 0: everything is kept, by the DROP kernels
    wrap("near0-hub-8x16-indices-plain", "lanes-hub-8x16-indices", P_NEAR_0)
    wrap("near0-hub-12x64-graph-logit", "lanes-hub-12x64-graph-logit", P_NEAR_0)
    # a logit of zeros under dropout: the bits of the DROP kernels without LOGIT
    wrap("zero-hub-12x64-indices", "zero-hub-12x64-indices")
    wrap("zero-three_chunk_hub-8x16-indices", "zero-three_chunk_hub-8x16-indices")
    wrap("twice-nine_hubs-8x16-indices-logit", "twice-nine_hubs-8x16-indices-logit")
    wrap("twice-hub-3x8-graph-plain", "twice-hub-3x8-graph")
    wrap("composed-hub-8x16-graph-plain", "composed-hub-8x16-graph")
    wrap("composed-hub-8x16-indices-logit", "composed-hub-8x16-indices-logit")
    wrap("capture-hub-8x16-indices-logit", "lanes-hub-8x16-indices-logit")
    rrow, rcol = _rect_coo()
    out.append(_wrapped(lambda s: DropModuleCase("module-rect-4x8", rrow, rcol, (300, 500), s, 0.5), seed()))
    return out


cases, case_names = seeded(_build_cases)
