#!/usr/bin/env python3
"""What a bf16 feature table buys the inference forward at config 5 (R-MAT 2^20 nodes, 10 760 610 edges, Fin 128, 8 heads x 16;
pygat_amd.rmat, the graph of bench.py).  One process, torch.no_grad(), alternating rounds:

  (a) gat_level(...)                              the fp32 inference forward (the yardstick)
  (b) gat_level(..., table_dtype=torch.bfloat16)  projection (fp32, unchanged) + pack + the bf16-table forward

each timed with device events over `--reps` calls per round, `--rounds` rounds a, b, a, b, ... after `--warmup` calls of each;
then the kernel spans of both (ops.KernelTimer: events around the launches, a run of their own) and the byte model of
DESIGN.md section 4: gathers of 8 + 4 R bytes per edge against 8 + 2 R, the pack pass 6 R bytes per node on top.
Also: the largest deviation of (b) from (a) on these N(0, 1) inputs.  Prints one JSON line; --out writes it to a file."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--fout", type=int, default=16)
    ap.add_argument("--fin", type=int, default=128)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--edges", type=int, default=5_000_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import pygat_amd as pg
    from pygat_amd import ops
    from pygat_amd.rmat import rmat_csr_numpy
    if not torch.cuda.is_available():
        sys.exit("bf16_forward_bench: no GPU; nothing is measured")
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(args.scale, args.edges, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    H, Fo, Fin = args.heads, args.fout, args.fin
    g = torch.Generator(device=dev).manual_seed(2)
    X = torch.randn(graph.n, Fin, generator=g, device=dev)
    Ws = list(torch.randn(H, Fin, Fo, generator=g, device=dev) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5))
    As = list(torch.randn(H, 2 * Fo, generator=g, device=dev) * 0.3)
    kinds = {"fp32": {}, "bf16": {"table_dtype": torch.bfloat16}}

    def level(kind):
        return pg.gat_level(X, graph, Ws, As, None, 0.2, True, **kinds[kind])

    def timed(kind):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            r = level(kind)
        b.record()
        b.synchronize()
        del r
        return a.elapsed_time(b) / args.reps

    with torch.no_grad():
        outs = {}
        for kind in kinds:
            for _ in range(args.warmup):
                outs[kind] = level(kind)
        torch.cuda.synchronize()
        dev_max = float((outs["bf16"] - outs["fp32"]).abs().max())
        ref_max = float(outs["fp32"].abs().max())
        outs.clear()
        ms = {k: [] for k in kinds}
        for _ in range(args.rounds):
            for kind in kinds:
                ms[kind].append(timed(kind))
        spans = {}
        for kind in kinds:
            ops.TIMER = ops.KernelTimer()
            for _ in range(args.reps):
                level(kind)
            torch.cuda.synchronize()
            spans[kind] = {k: round(statistics.median(v) * 1e3, 1) for k, v in ops.TIMER.times_ms().items()}
            ops.TIMER = None
    Fp = 1 << max(2, (Fo - 1).bit_length())
    R, E, N = H * Fp, graph.nnz, graph.n
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {
        "tool": "bf16_forward_bench", "device": torch.cuda.get_device_name(0), "n": N, "nnz": E, "fin": Fin, "heads": H, "fout": Fo,
        "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
        "fp32_forward_ms": {"median": round(med["fp32"], 4), "min": round(min(ms["fp32"]), 4), "max": round(max(ms["fp32"]), 4)},
        "bf16_forward_ms": {"median": round(med["bf16"], 4), "min": round(min(ms["bf16"]), 4), "max": round(max(ms["bf16"]), 4)},
        "fp32_over_bf16": round(med["fp32"] / med["bf16"], 4),
        "spans_us": spans,
        "byte_model": {"gather_bytes_per_edge": {"fp32": 8 + 4 * R, "bf16": 8 + 2 * R}, "pack_bytes_per_node": 6 * R,
                       "gather_MB": {"fp32": round(E * (8 + 4 * R) / 1e6, 1), "bf16": round(E * (8 + 2 * R) / 1e6, 1)},
                       "pack_MB": round(N * 6 * R / 1e6, 1)},
        "max_abs_deviation_from_fp32": dev_max, "max_abs_fp32_output": ref_max,
    }
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
