"""The one measuring harness of the pattern-attention bench tools (dot_attention_bench.py, additive_attention_bench.py,
gatv2_attention_bench.py; edge_softmax_bench.py takes `run_in_child` alone).  What a tool keeps is its byte models, its contenders and
its own record fields; how it measures is written here, once.

The workload is config 5's: the R-MAT graph of bench.py (pygat_amd.rmat, seed 1), its edge pattern with the transpose built, tensors
drawn from a device generator of seed 2, and 1024 rows picked with seed 3, the row of most entries added, on which outputs are checked.

The measuring step runs in a child process under `timeout -k 10 <--limit seconds>` (`run_in_child`); the process that was started
never opens the GPU.  All contenders run in that one child, alternated round by round (`alternate`): after every contender's warm-up
calls a round times `steps` calls of one contender, each between two HIP events, then the same of the next, in dict order.  Reported
per contender: the median over all rounds x steps timed calls and the spread of the rounds' medians (largest minus smallest).  A
difference below that spread is not a difference.

Before timing, the contenders' outputs are priced on the same seeded inputs by the rule of tests/parity.py against an fp64 computation
on the CPU over the checked rows (`pricer`): the whole [E, H, F] product does not fit an fp64 CPU run.  That computation walks the rows
256 at a time (`sampled_rows`), so that no [entries, H, F] tensor grows beyond them, and is the same for every family but for the score
and the values (`softmax_aggregate`).  `*_roof_ms` is a byte model's time at 8 TB/s and `*_roof_fraction` that over the measured time:
the whole op's share of the HBM roof on the byte model, not a kernel's.  Recorded, not gated.  One JSON object per record, appended."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLE_ROWS = 1024
HBM_BYTES_PER_S = 8e12
SECTOR = 32          # bytes: the granularity at which a row of H floats is counted


def sectors(nbytes):
    return -(-nbytes // SECTOR) * SECTOR


def timed_round(fn, steps):
    """-> the ms of `steps` calls, each between two events."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def alternate(contenders, rounds, steps, warmup):
    """{name: fn} -> {name: (median ms of all timed calls, spread of the rounds' medians)}."""
    for fn in contenders.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed_round(fn, steps))
    out = {}
    for name, per_round in times.items():
        medians = [statistics.median(r) for r in per_round]
        out[name] = (statistics.median([t for r in per_round for t in r]), max(medians) - min(medians))
    return out


class Workload:
    """What every tool measures on, built once per run from args: graph, pattern (transpose built), N, E, the CSR arrays on the CPU
    (rp_t, col_t, deg), the checked rows, perm (whether the pattern carries a permutation), dev and the imported parity; row_d, col_d:
    the row and the column of every entry as int64 on the device, E 8 bytes each, for the tool whose composition gathers by them."""

    def __init__(self, args, tool, row_d=False, col_d=False):
        import torch
        if not torch.cuda.is_available():
            sys.exit(f"{tool}: needs a GPU (a time taken anywhere else says nothing)")
        import pygat_amd as pg
        from pygat_amd.rmat import rmat_csr_numpy
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import parity                                                     # the one tolerance rule (tests/parity.py)
        self.parity, self.dev = parity, torch.device("cuda", 0)
        rp, col = rmat_csr_numpy(args.scale, args.draws, seed=1)
        self.graph = pg.CSRGraph(torch.from_numpy(rp).to(self.dev), torch.from_numpy(col).to(self.dev))
        self.pattern = self.graph.edge_pattern()
        self.pattern.transposed()
        self.N, self.E, self.perm = self.graph.n, self.graph.nnz, self.pattern.perm is not None
        self.row_d = self.pattern.edge_rc[:, 0].long() if row_d else None
        self.col_d = self.pattern.edge_rc[:, 1].long() if col_d else None
        self.rp_t, self.col_t = torch.from_numpy(rp).long(), torch.from_numpy(col).long()
        self.deg = self.rp_t[1:] - self.rp_t[:-1]
        picked = torch.randperm(self.N, generator=torch.Generator().manual_seed(3))[:SAMPLE_ROWS]
        self.rows = torch.unique(torch.cat([picked, torch.argmax(self.deg)[None]]))

    def generator(self):
        """A fresh device generator of the tensor seed: every shape draws the same stream."""
        import torch
        return torch.Generator(device=self.dev).manual_seed(2)


def shapes(args):
    """--shapes -> (shape, H, F) one after the other, the device cache emptied behind each: the caller's tensors of one shape are
    gone by then if they lived in the call it made."""
    import torch
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        yield shape, H, F
        torch.cuda.empty_cache()


def forward_of(fn, leaves):
    import torch

    def run():
        with torch.no_grad():
            return fn(*leaves)
    return run


def both_of(fn, leaves, G, clone=True):
    """Forward + backward with every leaf's gradient asked for, on leaves of its own (clone=False: fresh leaves on the same memory)."""
    import torch
    leaves = [(t.detach().clone() if clone else t.detach()).requires_grad_(True) for t in leaves]

    def run():
        return torch.autograd.grad(fn(*leaves), leaves, G)
    return run


def run_legs(args, contenders, G, clone=True):
    """{name: (fn, leaves)} -> [(what, {name: (median, spread)})]: the forward leg and, unless --forward-only, the forward + backward
    leg, whose leaves are made only once the forward leg has run."""
    def leg(of):
        return alternate({name: of(fn, leaves) for name, (fn, leaves) in contenders.items()}, args.rounds, args.steps, args.warmup)
    legs = [("forward", leg(forward_of))]
    if not args.forward_only:
        legs.append(("forward_backward", leg(lambda fn, leaves: both_of(fn, leaves, G, clone))))
    return legs


def sampled_rows(workload, rows_chunk=256):
    """The checked rows `rows_chunk` at a time -> (part, idx, sub, cols, inv): the rows, their entries' CSR positions (a row's entries
    together and in order), each entry's row within part, the distinct columns and each entry's place among them."""
    import torch
    rp, col = workload.rp_t, workload.col_t
    for part in torch.split(workload.rows, rows_chunk):
        idx = torch.cat([torch.arange(int(rp[r]), int(rp[r + 1])) for r in part.tolist()])
        sub = torch.repeat_interleave(torch.arange(part.numel()), rp[part + 1] - rp[part])
        cols, inv = torch.unique(col[idx], return_inverse=True)
        yield part, idx, sub, cols, inv


def taken(t, index, dtype):
    """t[index] on the CPU in dtype (None stays None); t may live on the device."""
    return None if t is None else t[index.to(t.device)].cpu().to(dtype)


def softmax_aggregate(scores, sub, n_rows, values_at_entries, mask=None):
    """scores [entries, H], values_at_entries [entries, H, F], sub the row of each entry -> out [n_rows, H, F]: the softmax over each
    row's entries, times mask [entries, H] (pre-scaled, after the softmax) where given, times the values, summed per row."""
    import torch
    m = torch.full((n_rows, scores.shape[1]), -float("inf"), dtype=scores.dtype)
    m = m.scatter_reduce(0, sub[:, None].expand(-1, scores.shape[1]), scores, "amax")
    p = torch.exp(scores - m[sub])
    alpha = p / torch.zeros_like(m).index_add(0, sub, p)[sub]
    if mask is not None:
        alpha = alpha * mask
    out = torch.zeros(n_rows, *values_at_entries.shape[1:], dtype=scores.dtype)
    return out.index_add(0, sub, alpha[:, :, None] * values_at_entries)


def sampled_reference(workload, dtype, entry_terms, mask=None, rows_chunk=256):
    """out of the checked rows by torch on the CPU in dtype.  entry_terms(dtype, part, idx, sub, cols, inv) -> (scores [entries, H],
    values at the entries [entries, H, F]) is the tool's part; mask: [E, H] at the CSR position, as softmax_aggregate takes it."""
    import torch
    outs = []
    for part, idx, sub, cols, inv in sampled_rows(workload, rows_chunk):
        scores, values = entry_terms(dtype, part, idx, sub, cols, inv)
        outs.append(softmax_aggregate(scores, sub, part.numel(), values, taken(mask, idx, dtype)))
    return torch.cat(outs)


def pricer(workload, entry_terms, mask=None):
    """-> (err_of, the fp32 reference's own error against the fp64 one); err_of(out, what) prices a contender's whole out on the
    checked rows against sampled_reference by parity.close_fwd and returns its error."""
    import torch
    ref64, ref32 = (sampled_reference(workload, dtype, entry_terms, mask) for dtype in (torch.float64, torch.float32))

    def err_of(out, what):
        return workload.parity.close_fwd(out[workload.rows.to(workload.dev)], ref64, what, ref32)
    return err_of, workload.parity.err(ref32, ref64)


HEAD = ("bench", "values", "device", "p", "graph", "N", "E", "H", "F", "scale", "negative_slope", "rounds", "steps_per_round", "warmup",
        "checked_rows", "longest_checked_row")


def base_record(bench, args, workload, H, F, **extra):
    """The head of a record, in HEAD's order; extra: those of HEAD's fields that only some records have.  bench=None: no such key."""
    import torch
    assert set(extra) <= set(HEAD), extra
    w = workload
    fields = {"bench": bench, "device": torch.cuda.get_device_name(0), "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1",
              "N": w.N, "E": w.E, "H": H, "F": F, "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup,
              "checked_rows": int(w.rows.numel()), "longest_checked_row": int(w.deg[w.rows].max()), **extra}
    return {key: fields[key] for key in HEAD if fields.get(key) is not None}


def roof_fields(res, what, name="fused"):
    """`{name}_{what}_roof_ms` and `_roof_fraction` from the record's own `{name}_forward_bytes` (+ `_backward_bytes`)."""
    model = res[f"{name}_forward_bytes"] + (res[f"{name}_backward_bytes"] if what == "forward_backward" else 0)
    res[f"{name}_{what}_roof_ms"] = 1e3 * model / HBM_BYTES_PER_S
    res[f"{name}_{what}_roof_fraction"] = res[f"{name}_{what}_roof_ms"] / res[f"{name}_{what}_ms"]


def add_legs(res, legs, speedup=None, each=None, roof=None):
    """Per leg, in this order: every contender's `{name}_{what}_ms` and `_spread_ms`; `{what}_speedup` = speedup[0]'s time over
    speedup[1]'s; each(what), the tool's own fields of a leg; roof_fields of the contender `roof`."""
    for what, r in legs:
        for name in r:
            res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
        if speedup is not None:
            res[f"{what}_speedup"] = res[f"{speedup[0]}_{what}_ms"] / res[f"{speedup[1]}_{what}_ms"]
        if each is not None:
            each(what)
        if roof is not None:
            roof_fields(res, what, roof)


def add_bf16_ratio(res):
    """The close of a float32-against-bfloat16 forward record."""
    res["measured_ratio"] = res["fused_bf16_forward_ms"] / res["fused_fp32_forward_ms"]
    res["faster_by_more_than_the_spread"] = (res["fused_fp32_forward_ms"] - res["fused_bf16_forward_ms"]
                                             > max(res["fused_fp32_forward_spread_ms"], res["fused_bf16_forward_spread_ms"]))


def write(record, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a") as f:
        f.write(json.dumps(record) + "\n")
    print(json.dumps(record), flush=True)


def common_arguments(parser, limit, out_help, shapes=("8x16,8x64", None), forward_only_help="skip the forward + backward leg"):
    """The flags every tool has; limit: the default of --limit, shapes: (default, help) of --shapes."""
    parser.add_argument("--shapes", default=shapes[0], help=shapes[1])
    parser.add_argument("--rounds", type=int, default=5)
    parser.add_argument("--steps", type=int, default=10, help="timed calls per round and contender")
    parser.add_argument("--warmup", type=int, default=10)
    parser.add_argument("--forward-only", action="store_true", help=forward_only_help)
    parser.add_argument("--scale", type=int, default=20)
    parser.add_argument("--draws", type=int, default=5_000_000)
    parser.add_argument("--limit", type=int, default=limit, help="seconds the measuring child may take")
    parser.add_argument("--out", default=None, help=out_help)
    parser.add_argument("--child", action="store_true", help=argparse.SUPPRESS)


def run_in_child(file, limit):
    """Start `file --child` with this process's own arguments under the time limit and exit with its status: a fresh child process,
    this one never opens the GPU."""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(file), "--child"] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))
