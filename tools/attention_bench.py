#!/usr/bin/env python3
"""What return_attention costs at config 5 (R-MAT 2^20 nodes, 10 760 610 edges, Fin 128, 8 heads x 16; pygat_amd.rmat, the graph
bench.py times): the no-grad forward of the v1 level and of the GATv2 level with and without the attention table, device events,
alternating pairs (one pair = one forward without, one with; each timed over --reps calls).  Prints one JSON line per level kind.

    python tools/attention_bench.py [--pairs 7] [--reps 10] [--kinds v1,v2]
    python tools/attention_bench.py --grad-legs [--iters 50] [--warmup 10] [--out FILE]
        (training step of the v1 level, forward + backward, with return_attention False / True / "grad" -- the last with a loss on
        both outputs -- interleaved iteration by iteration, one device-event pair per step, medians; then the HIP-event spans of
        the K14 launches and of K4 from the same process, K14 against its byte model, and the new kernels' register / scratch
        footprint.  One JSON object.)
    rocprofv3 --kernel-trace --stats -d DIR -o att -- python tools/attention_bench.py --profile
        (--profile: a few forwards with the attention, no timing -- the kernel table gives the k13 launches' time; the byte model
        below turns it into a fraction of the 8 TB/s roof: python tools/attention_bench.py --roof DIR)

Byte model of the attention pass (csrc/k13_attention.hip; what an edge must move at least, caches assumed to absorb the
row-local reads -- s, m, Z, the rowptr pair, GATv2's Whi row -- and nothing else):
  v1: per edge (row, col) 8 B + two map entries 8 B + the t_j gather 4H + the coefficients 4H;  the t stream: every row before the
      self-loop-only tail reads its Wh row (4R) and writes t (4H).
  v2: per edge 8 + 8 + the Whj_j gather 4R + the coefficients 4H;  Whi rows 4R once per row.
Byte model of the alpha-gradient passes (csrc/k14_alpha_grad.hip), N' = rows of more than one edge:
  rows: per edge (row, col) 8 + A 4H + the t_j gather 4H;  per row of N' its (s, m, Z) 12H in, the record 16H and ds' 4H out, less
        the 8H the issue's model leaves to caches = 24H;  cols: per edge 8 + A through perm_t 4H + the record gather 16H; dt' 4H per
        node;  the long-row scan of each pass reads every (row, col) pair once more, 8 B per edge, and the rowptr pair of each row."""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8.0e12     # bytes / s, MI355X HBM3E


def byte_model(kind, n, E, H, R, t_rows):
    if kind == "v1":
        return E * (8 + 8 + 4 * H + 4 * H) + t_rows * (4 * R + 4 * H)
    return E * (8 + 8 + 4 * R + 4 * H) + n * 4 * R


def setup(args):
    import torch
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(20, 5_000_000, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    H, Fo, Fin = args.heads, args.fout, args.fin
    g = torch.Generator(device=dev).manual_seed(2)
    X = torch.randn(graph.n, Fin, generator=g, device=dev)
    W1 = torch.randn(H, Fin, Fo, generator=g, device=dev) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)
    a1 = torch.randn(H, 2 * Fo, generator=g, device=dev) * 0.3
    W2 = torch.randn(H, 2 * Fin, Fo, generator=g, device=dev) * (1.414 * (2.0 / (2 * Fin + Fo)) ** 0.5)
    a2 = torch.randn(H, Fo, generator=g, device=dev) * 0.3
    return graph, X, (list(W1), list(a1)), (list(W2), list(a2))


def level(kind, graph, X, P, ra):
    import pygat_amd as pg
    from pygat_amd.gatv2 import gatv2_level
    if kind == "v1":
        return pg.gat_level(X, graph, P[0], P[1], None, 0.2, True, return_attention=ra)
    return gatv2_level(X, graph, P[0], P[1], None, 0.2, True, return_attention=ra)


def timed(kind, graph, X, P, ra, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        r = level(kind, graph, X, P, ra)
    b.record()
    b.synchronize()
    del r
    return a.elapsed_time(b) / reps


def roof(d, args):
    """k13 kernels of a --profile run's stats against the byte model."""
    import csv
    import numpy as np
    from pygat_amd.rmat import rmat_csr_numpy
    rp, col = rmat_csr_numpy(20, 5_000_000, seed=1)
    n, E = len(rp) - 1, len(col)
    deg = np.diff(rp)
    # the level runs in the internal degree order: the rows before the self-loop-only tail (rows of degree > 1 in a symmetric
    # pattern with self loops) carry t
    t_rows = int((deg > 1).sum())
    H = args.heads
    R = H * max(4, 1 << (args.fout - 1).bit_length())
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    calls = args.profile_calls
    out = {"calls_per_kind": calls, "kernels": {}}
    for r in rows:
        nm = r["Name"]
        if "att_" not in nm:
            continue
        key = "t" if "att_t_kernel" in nm else ("v1_edges" if "att_v1_kernel" in nm else ("v2_edges" if "att_v2_kernel" in nm else nm))
        out["kernels"][key] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3}
    for r in rows:
        nm = r["Name"]
        if "gat_fwd_kernel<" in nm:          # template <LPR, VEC, V2, AUX, FAST, ...>: the main launch of K2 / its V2 variant
            targs = [t.strip() for t in nm.split("gat_fwd_kernel<")[1].split(">")[0].split(",")]
            key = "v2_forward_main" if targs[2] == "true" else "k2_main"
            prev = out["kernels"].get(key)
            if prev is None or float(r["AverageNs"]) / 1e3 > prev["avg_us"]:
                out["kernels"][key] = {"calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3, "name": nm[:120]}
    k = out["kernels"]
    if "t" in k and "v1_edges" in k:
        us = k["t"]["avg_us"] + k["v1_edges"]["avg_us"]
        b = byte_model("v1", n, E, H, R, t_rows)
        out["v1"] = {"us": round(us, 1), "model_bytes": b, "roof_us": round(b / ROOF * 1e6, 1), "roof_fraction": round(b / ROOF * 1e6 / us, 3)}
    if "v2_edges" in k:
        us = k["v2_edges"]["avg_us"]
        b = byte_model("v2", n, E, H, R, t_rows)
        out["v2"] = {"us": round(us, 1), "model_bytes": b, "roof_us": round(b / ROOF * 1e6, 1), "roof_fraction": round(b / ROOF * 1e6 / us, 3)}
    print(json.dumps(out))


def alpha_grad_model(n, E, H, n_multi):
    rows = E * (8 + 4 * H + 4 * H) + n_multi * (16 * H + 8 * H)
    cols = E * (8 + 4 * H + 16 * H) + n * 4 * H
    scan = E * 8 + n * 8
    return {"rows": rows + scan, "cols": cols + scan}


def grad_legs(args):
    """fwd + bwd of the v1 level at config 5 with return_attention False (a) / True (b) / "grad" and a loss on both outputs (c)."""
    import ctypes as C
    import torch
    import pygat_amd as pg
    from pygat_amd import ops
    from pygat_amd._lib import lib
    graph, X, P1, _ = setup(args)
    Ws = [w.clone().requires_grad_(True) for w in P1[0]]
    As = [v.clone().requires_grad_(True) for v in P1[1]]
    H = args.heads
    gen = torch.Generator(device=X.device).manual_seed(3)
    G = torch.randn(graph.n, H * args.fout, generator=gen, device=X.device)
    A = torch.randn(graph.nnz, H, generator=gen, device=X.device)

    def step(mode):
        for p in Ws + As:
            p.grad = None
        r = pg.gat_level(X, graph, Ws, As, None, 0.2, True, return_attention=mode)
        if mode == "grad":
            torch.autograd.backward([r[0], r[1]], [G, A])
        else:
            (r[0] if mode else r).backward(G)

    legs = {"a_false": False, "b_true": True, "c_grad": "grad"}
    for _ in range(max(10, args.warmup)):
        for m in legs.values():
            step(m)
    torch.cuda.synchronize()
    iters = max(50, args.iters)
    ev = {k: [] for k in legs}
    for _ in range(iters):
        for k, m in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); step(m); b.record()
            ev[k].append((a, b))
    torch.cuda.synchronize()
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = {"graph": {"n": graph.n, "E": graph.nnz}, "heads": H, "fout": args.fout, "fin": args.fin, "iters": iters,
           "warmup": max(10, args.warmup), "step_ms_median": {k: round(med([a.elapsed_time(b) for a, b in v]), 4) for k, v in ev.items()}}
    sm = out["step_ms_median"]
    out["true_minus_false_ms"] = round(sm["b_true"] - sm["a_false"], 4)
    out["grad_minus_true_ms"] = round(sm["c_grad"] - sm["b_true"], 4)
    # kernel spans of leg (c), same process: HIP events around the launches (ops.KernelTimer)
    ops.TIMER = ops.KernelTimer()
    for _ in range(iters):
        step("grad")
    torch.cuda.synchronize()
    spans = {k: round(med(v) * 1e3, 1) for k, v in ops.TIMER.times_ms().items()}
    ops.TIMER = None
    out["span_us_median"] = spans
    import numpy as np
    deg = np.diff(graph.fwd.rowptr.cpu().numpy())
    model = alpha_grad_model(graph.n, graph.nnz, H, int((deg > 1).sum()))
    out["k14"] = {}
    for key, span in (("rows", "k14_alpha_rows"), ("cols", "k14_alpha_cols")):
        us = spans.get(span)
        out["k14"][key] = {"us": us, "model_bytes": model[key], "roof_us": round(model[key] / ROOF * 1e6, 1),
                           "roof_fraction": None if not us else round(model[key] / ROOF * 1e6 / us, 3)}
    out["k14"]["apply_and_da_us"] = spans.get("k14_alpha_apply")
    out["k4_backward_col_us"] = spans.get("k4_backward_col")
    out["footprint"] = {}
    for name in ("k14_rows_long", "k14_cols_long", "k14_rows_wave", "k14_cols_wave", "k14_apply"):
        regs, scratch = C.c_int(-1), C.c_int(-1)
        rc = lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch))
        out["footprint"][name] = {"regs": regs.value, "scratch_bytes": scratch.value} if rc == 0 else lib.pygat_last_error().decode()
    txt = json.dumps(out, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kinds", default="v1,v2")
    ap.add_argument("--fin", type=int, default=128)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--fout", type=int, default=16)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-calls", type=int, default=5)
    ap.add_argument("--roof", metavar="DIR")
    ap.add_argument("--grad-legs", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", metavar="FILE")
    args = ap.parse_args()
    if args.roof:
        return roof(args.roof, args)
    if args.grad_legs:
        return grad_legs(args)
    import torch
    graph, X, P1, P2 = setup(args)
    with torch.no_grad():
        for kind in args.kinds.split(","):
            P = P1 if kind == "v1" else P2
            for _ in range(args.warmup):
                level(kind, graph, X, P, False); level(kind, graph, X, P, True)
            torch.cuda.synchronize()
            if args.profile:
                for _ in range(args.profile_calls):
                    level(kind, graph, X, P, True)
                torch.cuda.synchronize()
                continue
            off, on = [], []
            for _ in range(args.pairs):
                off.append(timed(kind, graph, X, P, False, args.reps))
                on.append(timed(kind, graph, X, P, True, args.reps))
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            print(json.dumps({"kind": kind, "n": graph.n, "E": graph.nnz, "heads": args.heads, "fout": args.fout, "fin": args.fin,
                              "forward_ms": [round(v, 4) for v in off], "forward_with_attention_ms": [round(v, 4) for v in on],
                              "median_ms": round(med(off), 4), "median_with_attention_ms": round(med(on), 4),
                              "delta_ms": round(med(on) - med(off), 4)}), flush=True)


if __name__ == "__main__":
    main()
