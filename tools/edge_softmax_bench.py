#!/usr/bin/env python3
"""What pygat_amd.edge_softmax costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py), H heads
(default 8), N(0, 1) logits, forward and backward:

    python tools/edge_softmax_bench.py [--heads 8] [--perm] [--by row] [--reps 50] [--warmup 10] [--out profiles/edge_softmax_bench.jsonl]

The measuring step runs in a child process under `timeout -k 10 <--limit seconds>`; this process never opens the GPU.  Times are HIP
events around `reps` calls after `warmup` calls of the same shape.  --perm takes the pattern from EdgePattern.from_indices (a
permutation entry per walked entry) instead of the graph's own (none).  Algorithmic bytes:
  forward   E H 4 x 3 + E 8 (+ E 4 with a permutation): the logits read by the group pass and again by the entry pass, alpha
            written, the (row, col) pair of every entry;
  backward  E H 4 x 5 + E 8 (+ E 4): alpha and G read by both passes, dlogits written.
The fraction of the 8 TB/s HBM roof is those bytes over the measured time.  Recorded, not gated.  One JSON object per run, appended."""
import argparse
import json
import os
import sys

from pattern_bench import run_in_child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8.0e12     # bytes / s, MI355X HBM3E


def forward_bytes(E, H, perm):
    return E * H * 4 * 3 + E * 8 + (E * 4 if perm else 0)


def backward_bytes(E, H, perm):
    return E * H * 4 * 5 + E * 8 + (E * 4 if perm else 0)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("edge_softmax_bench: needs a GPU (a time taken anywhere else says nothing)")
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(args.scale, args.draws, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    pattern = pg.EdgePattern.from_indices(graph.edge_index(), (graph.n, graph.n)) if args.perm else graph.edge_pattern()
    E, H = graph.nnz, args.heads
    g = torch.Generator(device=dev).manual_seed(2)
    logits = torch.randn(E, H, generator=g, device=dev).requires_grad_(True)
    G = torch.randn(E, H, generator=g, device=dev)
    has_perm = (pattern.perm if args.by == "row" else pattern.transposed()[2]) is not None

    def fwd():
        with torch.no_grad():
            return pg.edge_softmax(pattern, logits, args.by)

    alpha = pg.edge_softmax(pattern, logits, args.by)

    def bwd():
        return torch.autograd.grad(alpha, [logits], G, retain_graph=True)

    res = {"device": torch.cuda.get_device_name(0), "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": graph.n, "E": E,
           "H": H, "by": args.by, "perm": has_perm, "reps": args.reps, "warmup": args.warmup,
           "forward_bytes": forward_bytes(E, H, has_perm), "backward_bytes": backward_bytes(E, H, has_perm), "roof_bytes_per_s": ROOF}
    res["forward_ms"] = timed(fwd, args.reps, args.warmup)
    res["backward_ms"] = timed(bwd, args.reps, args.warmup)
    res["forward_fraction_of_roof"] = res["forward_bytes"] / ROOF / (res["forward_ms"] * 1e-3)
    res["backward_fraction_of_roof"] = res["backward_bytes"] / ROOF / (res["backward_ms"] * 1e-3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))


def parse(argv=None):
    """-> (the parser, the arguments with --out and what else depends on the mode filled in)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--by", choices=("row", "col"), default="row")
    ap.add_argument("--perm", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--draws", type=int, default=5_000_000)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_softmax_bench.jsonl"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    return ap, args


def main():
    args = parse()[1]
    if args.child:
        return measure(args)
    run_in_child(__file__, args.limit)


if __name__ == "__main__":
    main()
