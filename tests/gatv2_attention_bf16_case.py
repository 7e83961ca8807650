"""The seeded cases of pygat_amd.gatv2_attention_bf16 and pygat_amd.gatv2_attention_edge_bf16, the inference forwards on bfloat16 tables
(the BF16 instantiations of the two forward kernels of csrc/k21_gatv2_attention.hip, without and with EDGE;
pygat_amd/gatv2_attention.py).

A case here wraps a case of gatv2_attention_case.py ("plain-...") or of gatv2_attention_edge_case.py ("edge-..."), imported and left as
it is: the same pattern, x_dst, a and slope; the row tables x_src, v (where the case has one of its own) and e are replaced by their
.bfloat16() (torch rounds to nearest even), the tables the device is given.  The contract is bit equality with the float32 op on the
widened tables; beside it the ground truth is the case file's own reference on the widened tables, in fp64 and in fp32, priced by the
one rule of parity.py (out by close_fwd with the fp32 ground-truth run's own error).  There is no backward, and a branch of LeakyReLU
that flips between fp32 and fp64 moves a forward value by no more than the rounding that caused it, so no kink is asserted.

Every case asserts that the rounding matters, so a path that silently read a float32 table could be told apart by value: at least 90 %
of the entries of every N(0, 1) table change when rounded (measured: 0.99998); of a table drawn on the grid of 2^-10 (the grid case) at
least half do (measured: 0.598), and its rounded values stay on the grid -- bfloat16 keeps the leading 8 bits of a multiple of 2^-10,
another multiple -- so that case's sums stay exact in fp32; a table of zeros is exempt.  `cases()` lists every case;
tests/test_gatv2_attention_bf16_abi.py rehearses each on the CPU with the fp32 ground-truth run standing in for the device,
tests/test_gpu_gatv2_attention_bf16.py runs them on the device."""
import torch

import gatv2_attention_case as plain
import gatv2_attention_edge_case as edge
from additive_attention_bf16_case import WIDE_SHAPE, changed
from dot_attention_case import LANE_SHAPES  # noqa: F401
from pattern_case import ForwardCase, seeded
from pattern_graphs import _coo, _hub_graph  # noqa: F401

CHANGED, CHANGED_ON_GRID = 0.9, 0.5


class Bf16Case(ForwardCase):
    """`inner` (a Case of gatv2_attention_case, or an EdgeCase of gatv2_attention_edge_case) with x_src16, v16 (None where v is x_src)
    and e16 (None without edge features) bfloat16 in the place of its x_src, v and e."""

    def __init__(self, name, inner):
        self.name, self.inner = name, inner
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "slope", "shared", "x_dst", "a", "G"):
            setattr(self, attr, getattr(inner, attr))
        self.pairs = getattr(inner, "pairs", None)
        self.edge = hasattr(inner, "e")
        self.op = "gatv2_attention_edge_bf16" if self.edge else "gatv2_attention_bf16"
        self.zero, self.grid = getattr(inner, "zero", False), getattr(inner, "grid", False)
        self.x_src16 = self._rounded("x_src", inner.x_src, self.grid)
        self.v16 = None if inner.shared else self._rounded("v", inner.v, False)
        self.e16 = self._rounded("e", inner.e, self.grid) if self.edge else None
        self._refs = None

    def _rounded(self, what, wide, on_grid):
        narrow = wide.float().bfloat16()
        assert narrow.dtype == torch.bfloat16 and narrow.shape == wide.shape
        if float(wide.abs().max()) == 0.0:                          # (a table of zeros: nothing to round)
            return narrow
        share, least = changed(wide, narrow), CHANGED_ON_GRID if on_grid else CHANGED
        assert share >= least, f"{self.name}: only {share:.3f} of the entries of {what} change when rounded to bfloat16"
        if on_grid:
            steps = narrow.double() / edge.GRID
            assert torch.equal(steps, steps.round()), f"{self.name}: a rounded value of {what} left the grid"
        return narrow

    def widened(self, dtype=torch.float64):
        """(x_src16, v16 | None, e16 | None) as `dtype`: exact."""
        return tuple(None if t is None else t.to(dtype) for t in (self.x_src16, self.v16, self.e16))

    def ref(self, dtype=torch.float64):
        """The ground truth on the widened tables, computed in `dtype`, shaped like the result."""
        x_src, v, e = self.widened(dtype)
        x_dst, a = self.x_dst.to(dtype), self.a.to(dtype)
        v = x_src if v is None else v
        if self.edge:
            out = edge.gatv2_attention_edge_ref(self.row, self.col, self.shape[0], x_dst, x_src, a, v, e, self.slope)
        else:
            out = plain.gatv2_attention_ref(self.row, self.col, self.shape[0], x_dst, x_src, a, v, self.slope)
        return out.reshape(self.G.shape)


def _build_cases():
    out = []

    def take(prefix, source, names):
        for n in names:
            out.append(Bf16Case(f"{prefix}-{n}", source[n]))

    hub = _hub_graph()
    row, col, N = _coo(hub)
    H, F = WIDE_SHAPE
    for prefix, source in (("plain", plain.cases()), ("edge", edge.cases())):
        # every lane shape on the hub pattern (a row of 699 entries: the long-row launch too), from indices and from a graph, v
        # shared and separate
        take(prefix, source, [f"lanes-hub-{h}x{f}-{kind}-{v}" for h, f in LANE_SHAPES for kind in ("indices", "graph")
                              for v in ("shared", "separate")])
        take(prefix, source, [f"lanes-asym-{h}x{f}-{tail}" for h, f in ((3, 8), (8, 16), (12, 64))
                              for tail in ("indices-shared", "graph-separate")])
        take(prefix, source, ["lanes-hub-noaxis-indices-shared", "lanes-asym-noaxis-graph-separate"])
        take(prefix, source, [f"long-{p}-{hf}-{tail}" for p in ("nine_hubs", "three_chunk_hub") for hf in ("8x16", "3x8")
                              for tail in ("indices-shared", "graph-separate")])
        take(prefix, source, ["rect-4x16-shared", "rect-3x8-separate", "repeats-8x16-shared", "repeats-8x16-separate"])
        take(prefix, source, [n for n in source if n.startswith("lonely-")])
        take(prefix, source, ["twice-hub-3x8-graph-shared", "twice-hub-12x64-indices-separate"])
    take("edge", edge.cases(), edge.case_names("zero-"))
    take("edge", edge.cases(), ["grid-hub-8x16-indices-separate", "strided-rect-4x16-shared", "strided-hub-3x8-graph-separate"])
    # the plain cases the zero- cases are built on, where not yet taken: e16 = 0 against the op without the term
    for z in edge.case_names("zero-"):
        name = "plain-" + z[len("zero-"):]
        if name not in {c.name for c in out}:
            out.append(Bf16Case(name, plain.cases()[z[len("zero-"):]]))
    out.append(Bf16Case(f"plain-lanes-hub-{H}x{F}-indices-shared", plain.Case("", row, col, (N, N), H, F, 43000)))
    out.append(Bf16Case(f"plain-lanes-hub-{H}x{F}-graph-separate", plain.Case("", row, col, (N, N), H, F, 43010, kind="graph", csr=hub,
                                                                               shared=False)))
    out.append(Bf16Case(f"edge-lanes-hub-{H}x{F}-indices-separate", edge.EdgeCase("wide-a", row, col, (N, N), H, F, 63000, shared=False)))
    out.append(Bf16Case(f"edge-lanes-hub-{H}x{F}-graph-shared", edge.EdgeCase("wide-b", row, col, (N, N), H, F, 63010, kind="graph",
                                                                              csr=hub)))
    return out


cases, case_names = seeded(_build_cases)
