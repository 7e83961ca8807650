"""The seeded cases of pygat_amd.dot_attention on bfloat16 k and v tables, the inference forward (the bf16-table instantiations of the
two forward kernels of csrc/k19_dot_attention.hip, pygat_amd/dot_attention.py).

A case here wraps a case of dot_attention_case.py or dot_attention_bias_case.py, imported and left as it is: the same pattern, q,
bias and scale; k and v are replaced by k16 = k.bfloat16() and v16 = v.bfloat16() (torch rounds to nearest even), the tables the device
is given.  The contract is bit equality with the float32 op on the widened tables k16.float(), v16.float(); beside it the ground truth
is the same fp64 computation as in those files on the widened tables, priced by the one rule of parity.py (out by close_fwd with the
fp32 ground-truth run's own error).  There is no backward.  Every case asserts that the rounding matters: at least 90 % of the entries
of k and of v change when rounded, so a path that silently read float32 tables could be told apart by value.  `cases()` lists every
case; tests/test_dot_attention_bf16_abi.py rehearses each on the CPU with the fp32 ground-truth run standing in for the device,
tests/test_gpu_dot_attention_bf16.py runs them on the device."""
import torch

import dot_attention_bias_case as biased
import dot_attention_case as base
from dot_attention_case import LANE_SHAPES  # noqa: F401
from pattern_case import ForwardCase, seeded
from pattern_graphs import _coo

WIDE_SHAPE = (8, 64)      # 128 chunks of 4 per row: two chunks per lane, which no entry of LANE_SHAPES has; a shape of the measurements


class Bf16Case(ForwardCase):
    """`inner` (a Case or a BiasCase) with k16, v16 [n_cols, (H,) F] bfloat16 in the place of its k and v; bias: inner's, or None."""
    op = "dot_attention_bf16"

    def __init__(self, name, inner):
        self.name, self.inner = name, inner
        for attr in ("row", "col", "shape", "H", "F", "kind", "csr", "q", "scale", "fed_scale"):
            setattr(self, attr, getattr(inner, attr))
        self.bias, self.masked = getattr(inner, "bias", None), getattr(inner, "masked", None)
        self.k16, self.v16 = inner.k.float().bfloat16(), inner.v.float().bfloat16()
        for wide, narrow in ((inner.k, self.k16), (inner.v, self.v16)):
            assert narrow.dtype == torch.bfloat16 and narrow.shape == wide.shape
            changed = float((narrow.double() != wide).double().mean())
            assert changed >= 0.9, f"{name}: only {changed:.2f} of the entries change when rounded to bfloat16"
        self._refs = None

    @property
    def G(self):
        """What the result is shaped like: the wrapped case's G, which has q's shape."""
        return self.inner.G

    def widened(self, dtype=torch.float64):
        """k16 and v16 as `dtype`: exact."""
        return self.k16.to(dtype), self.v16.to(dtype)

    def ref(self, dtype=torch.float64):
        """The ground truth on the widened tables, computed in `dtype`, shaped like q."""
        k, v = self.widened(dtype)
        q = self.q.to(dtype)
        if self.bias is None:
            out = base.dot_attention_ref(self.row, self.col, self.shape[0], q, k, v, self.scale)
        else:
            out = biased.biased_ref(self.row, self.col, self.shape[0], q, k, v, self.scale, self.bias.to(dtype))
        return out.reshape(self.q.shape)


def _build_cases():
    plain, bias = base.cases(), biased.cases()
    out = []

    def take(prefix, source, names):
        for n in names:
            out.append(Bf16Case(f"{prefix}-{n}", source[n]))

    take("plain", plain, [f"lanes-hub-{H}x{F}-{kind}" for H, F in LANE_SHAPES for kind in ("indices", "graph")])
    take("plain", plain, [f"lanes-asym-{H}x{F}-indices" for H, F in ((3, 8), (8, 16), (12, 64))])
    take("plain", plain, ["lanes-hub-noaxis-indices", "lanes-hub-noaxis-graph"])
    take("plain", plain, [f"long-nine_hubs-8x16-{kind}" for kind in ("indices", "graph")])
    take("plain", plain, [f"long-three_chunk_hub-3x8-{kind}" for kind in ("indices", "graph")])
    take("plain", plain, base.case_names("lonely-"))
    take("plain", plain, ["twice-nine_hubs-8x16-indices", "twice-hub-3x8-graph"])
    take("bias", bias, ["rect-3x8", "rect-4x16", "repeats-8x16", "shared-hub-8x16-indices", "shared-hub-3x8-graph",
                        "lanes-hub-noaxis-indices", "lanes-hub-12x64-graph", "lanes-hub-4x256-indices", "long-nine_hubs-8x16-indices",
                        "long-three_chunk_hub-3x8-graph", "lonely-8x16-indices"])
    take("bias", bias, biased.case_names("masked-"))
    take("bias", bias, biased.case_names("zero-"))
    take("bias", bias, ["twice-nine_hubs-8x16-indices"])
    hub = base._hub_graph()
    row, col, N = _coo(hub)
    H, F = WIDE_SHAPE
    out.append(Bf16Case(f"plain-lanes-hub-{H}x{F}-indices", base.Case("", row, col, (N, N), H, F, 31000)))
    inner = base.Case("", row, col, (N, N), H, F, 31010, kind="graph", csr=hub)
    out.append(Bf16Case(f"bias-lanes-hub-{H}x{F}-graph", biased.BiasCase("", inner, biased._bias(row.numel(), H, 31014))))
    return out


cases, case_names = seeded(_build_cases)
