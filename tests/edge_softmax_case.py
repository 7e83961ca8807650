"""Ground truth, inputs and the seeded cases of the tests of pygat_amd.edge_softmax (csrc/k18_edge_softmax.hip).

Ground truth is torch autograd on the CPU through `edge_softmax_ref` (scatter_reduce(amax), exp, index_add, divide: layers.py:145-150,160
as spmm_case.softmax_values spells it), in any dtype.  Loss L = <alpha, G>, G ~ N(0, 1), seeded.  Pricing is parity.check_autograd,
unchanged: alpha by close_fwd, dlogits by close_grad.  The device and both ground-truth runs are fed the same fp32-rounded numbers.
`cases()` lists every seeded case that is priced that way, and `composition_inputs` holds the one case priced through two ops;
tests/test_edge_softmax_abi.py rehearses each of them on the CPU with the fp32 ground-truth run standing in for the device
(`fp32_stand_in`), tests/test_gpu_edge_softmax.py runs them on the device and builds no case of its own."""
import numpy as np
import torch

import parity
from bf16_table_case import hub_graph as lonely_hub_graph
from long_row_cases import nine_hubs, three_chunk_hub
from pattern_case import seeded
from pattern_graphs import COMPOSE_SEED, SLOPE, _asym_graph, _coo, _hub_graph, _params, _rect_coo, _repeat_coo
from spmm_case import coo_of, f32, normal, spmm_ref

HEADS = (1, 2, 3, 6, 8, 64)


def edge_softmax_ref(group, n_groups, logits):
    """logits [E] | [E, H] -> alpha like logits: the softmax over the entries of every group (repeated pairs are separate entries)."""
    l = logits if logits.dim() == 2 else logits[:, None]
    H = l.shape[1]
    m = torch.full((n_groups, H), -float("inf"), dtype=l.dtype).scatter_reduce(0, group[:, None].expand(-1, H), l.detach(), "amax")
    p = torch.exp(l - m[group])
    out = p / torch.zeros(n_groups, H, dtype=l.dtype).index_add(0, group, p)[group]
    return out if logits.dim() == 2 else out[:, 0]


def inputs(E, H, seed, scale=1.0, heads=True):
    """-> (logits [E, H] | [E] ~ N(0, scale^2), G like them), float64 holding fp32-representable numbers."""
    l, G = f32(normal((E, H), seed) * scale), f32(normal((E, H), seed + 1))
    if not heads:
        assert H == 1
        l, G = l[:, 0], G[:, 0]
    return l, G


def fp32_stand_in(group, n_groups):
    """The fp32 ground-truth run in the device's place: the rehearsal that a seed's inputs pass the pricing at all."""
    def run(l, G):
        ll = l.float().requires_grad_(True)
        out = edge_softmax_ref(group, n_groups, ll)
        (dl,) = torch.autograd.grad(out, [ll], G.float())
        return out.detach(), dl
    return run


def price(what, group, n_groups, l, G, alpha, dl):
    """alpha and dlogits of one run against the ground truth -> (report, alpha in fp64)."""
    assert alpha.shape == l.shape and dl.shape == l.shape, what
    rep, (y64, _) = parity.check_autograd(alpha.reshape(-1), [dl], lambda l_: edge_softmax_ref(group, n_groups, l_).reshape(-1), [l],
                                          G.reshape(-1), ["dlogits"], what)
    print(what, {k: f"{e:.2e}" for k, e in rep.items()})
    return rep, y64.reshape(l.shape)


class Case:
    """One seeded case: the entries (row, col) of a `shape` pattern, logits and G; `kind` = how the device's pattern is built
    ("indices": EdgePattern.from_indices, entries as given; "graph": CSRGraph.edge_pattern() of the CSR the entries came from).
    `fed` is what the run under test is given: the logits themselves, except where a case feeds an equivalent of them."""

    def __init__(self, name, row, col, shape, H, seed, by="row", kind="indices", scale=1.0, heads=True, csr=None):
        self.name, self.row, self.col, self.shape, self.H, self.by, self.kind, self.csr = name, row, col, shape, H, by, kind, csr
        self.group, self.n_groups = (row, shape[0]) if by == "row" else (col, shape[1])
        self.logits, self.G = inputs(row.numel(), H, seed, scale, heads)
        self.fed = self.logits

    def price(self, alpha, dl):
        return price(self.name, self.group, self.n_groups, self.logits, self.G, alpha, dl)

    def rehearse(self):
        return self.price(*fp32_stand_in(self.group, self.n_groups)(self.fed, self.G))


def _build_cases():
    out = []
    for pname, builder in (("hub", _hub_graph), ("asym", _asym_graph)):
        csr = builder()
        row, col, N = _coo(csr)
        for H in HEADS:
            for kind in ("indices", "graph"):
                out.append(Case(f"heads-{pname}-H{H}-{kind}", row, col, (N, N), H, 2000 + 10 * H + len(out), kind=kind, csr=csr))
        out.append(Case(f"heads-{pname}-noaxis-indices", row, col, (N, N), 1, 2900 + len(out), heads=False))
        out.append(Case(f"heads-{pname}-noaxis-graph", row, col, (N, N), 1, 2950 + len(out), kind="graph", heads=False, csr=csr))
    for pname, builder in (("nine_hubs", nine_hubs), ("three_chunk_hub", three_chunk_hub)):
        csr = builder()
        row, col, N = _coo(csr)
        for H in (1, 8):
            for kind in ("indices", "graph"):
                out.append(Case(f"long-{pname}-H{H}-{kind}", row, col, (N, N), H, 3000 + 10 * H + len(out), kind=kind, scale=3.0, csr=csr))
    csr = _asym_graph()
    row, col, N = _coo(csr)
    out.append(Case("col-asym-H8-indices", row, col, (N, N), 8, 4000, by="col"))
    out.append(Case("col-asym-H3-indices", row, col, (N, N), 3, 4010, by="col"))
    out.append(Case("col-asym-H8-graph", row, col, (N, N), 8, 4020, by="col", kind="graph", csr=csr))
    csr = _hub_graph()
    hrow, hcol, hN = _coo(csr)
    out.append(Case("col-hub-H8-graph", hrow, hcol, (hN, hN), 8, 4030, by="col", kind="graph", csr=csr))
    rrow, rcol = _rect_coo()
    for by in ("row", "col"):
        out.append(Case(f"rect-H4-{by}", rrow, rcol, (300, 500), 4, 5000 + len(out), by=by))
        out.append(Case(f"rect-H3-{by}", rrow, rcol, (300, 500), 3, 5100 + len(out), by=by))
    prow, pcol, N, pairs = _repeat_coo()
    for by in ("row", "col"):
        out.append(Case(f"repeats-H8-{by}", prow, pcol, (N, N), 8, 6000 + len(out), by=by))
        out[-1].pairs = pairs                                    # [(k, k')] positions of the repeated (row, col) pairs
    return out + _exact_cases() + _twice_cases()


def _exact_cases():
    """Rows of one entry; the reference's mask value among N(0, 1) logits; rows of equal huge logits; a constant per group."""
    out = []
    csr = lonely_hub_graph()
    row, col, N = _coo(csr)
    for H in (3, 8):
        for kind in ("indices", "graph"):
            out.append(Case(f"lonely-H{H}-{kind}", row, col, (N, N), H, 7000 + H, kind=kind, csr=csr))
    csr = _hub_graph()
    row, col, N = _coo(csr)
    deg = torch.bincount(row, minlength=N)
    masked = (torch.rand(row.numel(), generator=torch.Generator().manual_seed(7101)) < 0.3) & (deg[row] >= 3)
    masked[torch.as_tensor(np.asarray(csr[0][:-1], dtype=np.int64))] = False       # a row's first entry stays: no row is masked whole
    assert int(masked.sum()) > 500 and bool(masked[row == 5].any())                 # (row 5: the hub row of 699 entries)
    rows = torch.zeros(N, dtype=torch.bool)
    rows[::3] = True
    rows[5] = True
    shift = torch.randint(-8, 9, (N, 8), generator=torch.Generator().manual_seed(7301)).double()
    for kind in ("indices", "graph"):
        c = Case(f"masked-{kind}", row, col, (N, N), 8, 7100, kind=kind, csr=csr)
        c.logits[masked] = -9e15                                                     # layers.py:40
        c.masked = masked
        out.append(c)
        c = Case(f"huge-{kind}", row, col, (N, N), 8, 7200, kind=kind, csr=csr)
        c.huge, c.deg = rows[row], deg
        c.logits[c.huge] = 9e15
        out.append(c)
        # logits on a 2^-10 grid inside [-7, 7], whole-number shifts inside [-8, 8]: every shifted logit is exact in fp32, so the exact
        # softmax of `fed` is that of `logits` and one ground truth prices both runs
        for name, moved in ((f"grid-{kind}", False), (f"shifted-{kind}", True)):
            c = Case(name, row, col, (N, N), 8, 7300, kind=kind, csr=csr)
            c.logits = c.fed = torch.round(c.logits.clamp(-7, 7) * 1024) / 1024
            if moved:
                c.fed = c.logits + shift[row]
                assert torch.equal(c.fed.float().double(), c.fed)
            out.append(c)
    return out


def _twice_cases():
    csr = nine_hubs()
    row, col, N = _coo(csr)
    return [Case(f"twice-H{H}-{kind}-{by}", row, col, (N, N), H, 7400 + H, by=by, kind=kind, scale=3.0, csr=csr)
            for H, kind, by in ((8, "indices", "row"), (8, "graph", "row"), (3, "indices", "col"), (1, "graph", "col"))]


def composition_inputs():
    """The reference's sparse layer from parts (layers.py:141-160): Wh, s, t in fp32 on the CPU, logits = LeakyReLU(s_i + t_j).
    -> (rowptr, col, x, W, a, logits [E, H], Wh [N, H, Fo], G [N, H, Fo]); logits, Wh, G float64 holding fp32 numbers."""
    H, Fo = 8, 16
    rowptr, col = _hub_graph()
    N = len(rowptr) - 1
    r, c = coo_of(rowptr, col)
    x, W, a, _ = _params(N, 48, H, Fo, seed=COMPOSE_SEED)
    Wh = torch.stack([x @ W[h] for h in range(H)], 1)                               # [N, H, Fo], fp32
    s, t = torch.einsum("nhf,hf->nh", Wh, a[:, :Fo]), torch.einsum("nhf,hf->nh", Wh, a[:, Fo:])
    logits = torch.nn.functional.leaky_relu(s[r] + t[c], SLOPE)
    return rowptr, col, x, W, a, logits.double(), Wh.double(), f32(normal((N, H, Fo), 7500))


def composition_ref(r, c, N):
    """(logits, Wh) -> y = spmm(edge_softmax(logits), Wh) flattened: the torch spelling of the composition, in the leaves' dtype."""
    def fn(l_, Wh_):
        return spmm_ref(r, c, N, edge_softmax_ref(r, N, l_), Wh_).reshape(-1)
    return fn


def price_composition(y, grads, rowptr, col, logits, Wh, G):
    r, c = coo_of(rowptr, col)
    rep, _ = parity.check_autograd(y.reshape(-1), list(grads), composition_ref(r, c, len(rowptr) - 1), [logits, Wh], G.reshape(-1),
                                   ["dlogits", "dWh"], "edge_softmax + spmm")
    print("edge_softmax + spmm", {k: f"{v:.2e}" for k, v in rep.items()})
    return rep


cases, case_names = seeded(_build_cases)
