"""The seeded cases of pygat_amd.additive_attention_bf16, the inference forward on a bfloat16 v table (the BF16 instantiations of the two
forward kernels of csrc/k20_additive_attention.hip, pygat_amd/additive_attention.py).

A case here wraps a case of additive_attention_case.py, imported and left as it is: the same pattern, s_dst, s_src, edge_logit and
slope; v is replaced by v16 = v.bfloat16() (torch rounds to nearest even), the table the device is given.  The contract is bit equality
with the float32 op on the widened table v16.float(); beside it the ground truth is additive_attention_case's own reference on the
widened table, in fp64 and in fp32, priced by the one rule of parity.py (out by close_fwd with the fp32 ground-truth run's own error).
There is no backward, so there is no kink to keep clear of: a branch of LeakyReLU depends on s_dst, s_src and the logit alone, which
are not rounded.  Every case asserts that the rounding matters: at least 90 % of the entries of v change when rounded, so a path that
silently read a float32 table could be told apart by value.  `cases()` lists every case;
tests/test_additive_attention_bf16_abi.py rehearses each on the CPU with the fp32 ground-truth run standing in for the device,
tests/test_gpu_additive_attention_bf16.py runs them on the device."""
import torch

import additive_attention_case as base
from dot_attention_case import LANE_SHAPES  # noqa: F401
from pattern_case import ForwardCase, seeded
from pattern_graphs import _coo, _hub_graph  # noqa: F401

WIDE_SHAPE = (8, 64)      # 128 chunks of 4 per row: two chunks per lane, which no entry of LANE_SHAPES has
CHANGED = 0.9             # the share of the entries of an N(0, 1) table that rounding to bfloat16 changes, at least (measured: 0.99998)


def changed(wide, narrow):
    """The share of the entries of `wide` (fp32 values) that differ from their bfloat16 rounding `narrow`."""
    return float((narrow.double() != wide.double()).double().mean())


class Bf16Case(ForwardCase):
    """`inner` (a Case of additive_attention_case) with v16 [n_cols, (H,) F] bfloat16 in the place of its v."""
    op = "additive_attention_bf16"

    def __init__(self, name, inner):
        self.name, self.inner = name, inner
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "slope", "logit", "masked", "s_dst", "s_src", "u", "G"):
            setattr(self, attr, getattr(inner, attr))
        self.pairs = getattr(inner, "pairs", None)
        self.v16 = inner.v.float().bfloat16()
        assert self.v16.dtype == torch.bfloat16 and self.v16.shape == inner.v.shape
        share = changed(inner.v, self.v16)
        assert share >= CHANGED, f"{name}: only {share:.2f} of the entries of v change when rounded to bfloat16"
        self._refs = None

    def widened(self, dtype=torch.float64):
        """v16 as `dtype`: exact."""
        return self.v16.to(dtype)

    def ref(self, dtype=torch.float64):
        """The ground truth on the widened table, computed in `dtype`, shaped like the result."""
        u = None if self.u is None else self.u.to(dtype)
        out = base.additive_attention_ref(self.row, self.col, self.shape[0], self.s_dst.to(dtype), self.s_src.to(dtype),
                                          self.widened(dtype), self.slope, u)
        return out.reshape(self.G.shape)


def _build_cases():
    src = base.cases()
    out = []

    def take(names):
        for n in names:
            out.append(Bf16Case(n, src[n]))

    # every lane shape on the hub pattern (a row of 699 entries: the long-row launch too), from indices and from a graph, without a
    # logit and with a [E, H] one; a [E] one shared by the heads at every other shape
    take([f"lanes-hub-{H}x{F}-{kind}{tag}" for H, F in LANE_SHAPES for kind in ("indices", "graph") for tag in ("", "-logit")])
    take([n for n in base.case_names("lanes-hub-") if n.endswith("-shared")])
    take([f"lanes-asym-{H}x{F}-indices{tag}" for H, F in ((3, 8), (8, 16), (12, 64)) for tag in ("", "-logit")])
    take([f"lanes-hub-noaxis-{kind}{tag}" for kind in ("indices", "graph") for tag in ("", "-logit")])
    take(base.case_names("long-"))
    take(["rect-4x16", "rect-3x8-logit", "repeats-8x16", "repeats-8x16-logit"])
    take(base.case_names("lonely-"))
    take(base.case_names("zero-"))
    take(base.case_names("masked-"))
    take(base.case_names("twice-"))
    hub = _hub_graph()
    row, col, N = _coo(hub)
    H, F = WIDE_SHAPE
    out.append(Bf16Case(f"lanes-hub-{H}x{F}-indices", base.Case("", row, col, (N, N), H, F, 33000)))
    out.append(Bf16Case(f"lanes-hub-{H}x{F}-graph-logit", base.Case("wide-logit", row, col, (N, N), H, F, 33010, kind="graph", csr=hub,
                                                                      logit="full")))
    return out


cases, case_names = seeded(_build_cases)
