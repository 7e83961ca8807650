#!/usr/bin/env python3
"""What pygat_amd.sample_blocks costs on the headline R-MAT graph (pygat_amd.rmat.rmat_csr, 2^20 nodes, drawn on the device) against
the same kind of block from a torch composition on the same device:

    python tools/sample_bench.py [--seeds 1024,16384] [--fanouts 10/10,25/5,10,15] [--rounds 5] [--steps 5] [--warmup 3]
                                 [--out profiles/sample_bench.jsonl]
    python tools/sample_bench.py --footprints profiles/sample_footprints.txt      # pygat_kernel_footprint of the K22 kernels, nothing timed
    python tools/sample_bench.py --weighted [--out profiles/sample_weighted_bench.jsonl]      # what sampling weighted by edge adds

The composition (the baseline; it runs without K22): random keys per candidate entry (every entry of every dst row), one sort by
(row, key), the first `fanout` of each row, torch.unique for the sources, a node table for the local ids, EdgePattern.from_indices.
It draws a uniform sample without replacement per row like the sampler, but not the same one, and it is not seeded per position.

Both contenders run in this one process and are alternated hop by hop, round by round: a round times `steps` calls of the sampler on
hop t, then `steps` calls of the composition on the same dst, each call between two host clock reads with a device synchronise before
the first (a call ends in its own host read, so the clock sees the whole call).  Reported per hop: the median over all rounds x steps
calls and the spread (lowest and highest) of the rounds' medians, the ratio of the medians, the candidate entries the hop examined
(the sum of the dst degrees; the sampler's Philox calls are at least a quarter of that per pass over the keys), the kept entries and
kept entries per second.  Per configuration besides: sample_blocks end to end, host reads included.  Recorded, not gated.  One JSON
object per (seeds, fanouts), appended.

--weighted: the same graph, seeds and fanouts, but the contenders are sample_neighbors_weighted (uniform random weights in [0.05, 1),
one tensor for all hops) and sample_neighbors on the same dst -- the dst of the UNWEIGHTED blocks, so both examine the same candidate
entries -- alternated in the same way, and sample_blocks_weighted against sample_blocks end to end, alternated round by round.  What
the weighted call adds per candidate: one 4-byte weight per pass over the keys, a log and a division; per hop: two more launches (the
long rows' count, the entry count).  Nothing is compared but the time: the two draw different samples."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_hop(pg, torch, graph, dst, fanout):
    """The block of `dst` from torch ops: -> (EdgePattern, src_nodes, candidates)."""
    dev = dst.device
    rp, col = graph.fwd.rowptr.long(), graph.fwd.col.long()
    n_dst = dst.numel()
    b = rp[dst]
    deg = rp[dst + 1] - b
    offs = torch.cumsum(deg, 0) - deg
    row = torch.repeat_interleave(torch.arange(n_dst, device=dev), deg)          # (a host read: the number of candidates)
    total = row.numel()
    within = torch.arange(total, device=dev) - offs[row]
    pos = b[row] + within
    key = torch.rand(total, device=dev, dtype=torch.float64)
    order = torch.argsort(row.double() + key)                                     # by (row, key): a row's candidates stay together
    keep = torch.sort(order[within < fanout]).values if fanout is not None else torch.arange(total, device=dev)
    r, j = row[keep], col[pos[keep]]
    local = torch.full((graph.n,), -1, dtype=torch.int64, device=dev)
    local[dst] = torch.arange(n_dst, device=dev)
    others = torch.unique(j)
    others = others[local[others] < 0]
    local[others] = n_dst + torch.arange(others.numel(), device=dev)
    src = torch.cat([dst, others])
    pattern = pg.EdgePattern.from_indices(torch.stack([r, local[j]]), (n_dst, src.numel()))
    return pattern, src, total


def timed(torch, fn, steps):
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(rounds):
    flat = [x for r in rounds for x in r]
    meds = [statistics.median(r) for r in rounds]
    return dict(median_ms=round(statistics.median(flat), 4), round_medians_ms=[round(min(meds), 4), round(max(meds), 4)], calls=len(flat))


K22_KERNELS = ("k22_count", "k22_verify", "k22_list", "k22_select_wave", "k22_select_block", "k22_clear_dst", "k22_sources", "k22_relabel",
               "k22_count_weighted", "k22_list_weighted", "k22_count_long_weighted", "k22_entries_weighted", "k22_select_wave_weighted",
               "k22_select_block_weighted")


def alternate(torch, args, ours, theirs):
    """Warm both up, then `rounds` rounds of `steps` calls of the one and `steps` calls of the other -> their two summaries."""
    for _ in range(args.warmup):
        ours(), theirs()
    a, b = [], []
    for _ in range(args.rounds):
        a.append(timed(torch, ours, args.steps))
        b.append(timed(torch, theirs, args.steps))
    return summary(a), summary(b)


def footprints(torch, path, family, names):
    """pygat_kernel_footprint of the kernels `names` of `family` (K22, K23, K24) -> the text file at `path`; nothing is timed."""
    import ctypes as C
    from pygat_amd import _lib
    torch.cuda.init()
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    width = max(16, max(len(name) for name in names) + 1)
    with open(path, "w") as f:
        f.write(f"# pygat_kernel_footprint of the {family} kernels on {torch.cuda.get_device_name(0)}: VGPRs per lane, scratch bytes per lane\n")
        for name in names:
            regs, scratch = C.c_int(0), C.c_int(0)
            _lib.check(_lib.lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)), name)
            f.write(f"{name:{width}s} regs={regs.value:3d} scratch={scratch.value}\n")


def weighted_leg(args, torch, pg, graph, deg, seed):
    dev = graph.device
    w = torch.rand(graph.nnz, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) * 0.95 + 0.05
    for n_seeds in (int(s) for s in args.seeds.split(",")):
        seeds = torch.randperm(graph.n, device=dev, generator=torch.Generator(device=dev).manual_seed(n_seeds))[:n_seeds]
        for fan in args.fanouts.split("/"):
            fanouts = [int(f) for f in fan.split(",")]
            blocks = pg.sample_blocks(graph, seeds, fanouts, seed=seed)[::-1]                # hop order: the dst of both contenders
            hops = []
            for t, blk in enumerate(blocks):
                dst, fanout = blk.dst_nodes, fanouts[-1 - t]
                plain = lambda: pg.sample_neighbors(graph, dst, fanout, seed=seed, hop=t)                    # noqa: E731
                weighted = lambda: pg.sample_neighbors_weighted(graph, dst, fanout, w, seed=seed, hop=t)    # noqa: E731
                wb = weighted()
                assert wb.nnz == blk.nnz, "every weight is positive: both keep min(degree, fanout) entries per row"
                sa, sb = alternate(torch, args, weighted, plain)
                cand = int(deg[dst].sum())
                hops.append(dict(hop=t, n_dst=blk.n_dst, fanout=fanout, candidates=cand, kept=wb.nnz, n_src=wb.n_src, unweighted_n_src=blk.n_src,
                                 long_rows=int((deg[dst] > 256).sum()), longest_row=int(deg[dst].max()), weighted=sa, unweighted=sb,
                                 weighted_over_unweighted=round(sa["median_ms"] / sb["median_ms"], 3),
                                 extra_us=round((sa["median_ms"] - sb["median_ms"]) * 1e3, 1)))
                print(json.dumps(hops[-1]), flush=True)
            a, b = [], []                                                       # (both are warm from the hops)
            for _ in range(args.rounds):
                a.append(timed(torch, lambda: pg.sample_blocks_weighted(graph, seeds, fanouts, w, seed=seed), args.steps))
                b.append(timed(torch, lambda: pg.sample_blocks(graph, seeds, fanouts, seed=seed), args.steps))
            line = dict(tool="sample_bench --weighted", device=torch.cuda.get_device_name(0), graph=f"rmat scale {args.scale}", N=graph.n,
                        E=graph.nnz, seeds=n_seeds, fanouts=fanouts, rounds=args.rounds, steps=args.steps, weights="uniform [0.05, 1)",
                        sample_blocks_weighted=summary(a), sample_blocks=summary(b), hops=hops)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            print(f"seeds={n_seeds} fanouts={fanouts}: sample_blocks_weighted {line['sample_blocks_weighted']['median_ms']} ms, sample_blocks "
                  f"{line['sample_blocks']['median_ms']} ms", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--footprints", default=None)
    ap.add_argument("--weighted", action="store_true")
    ap.add_argument("--seeds", default="1024,16384")
    ap.add_argument("--fanouts", default="10/10,25/5,10,15")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "sample_weighted_bench.jsonl" if args.weighted else "sample_bench.jsonl")
    import torch
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench: needs a GPU (there is nothing to time without one)")
    if args.footprints:
        return footprints(torch, args.footprints, "K22", K22_KERNELS)
    dev = "cuda"
    rowptr, col = rmat_csr(scale=args.scale, device=dev)
    graph = pg.CSRGraph(rowptr, col)
    deg = (graph.fwd.rowptr[1:] - graph.fwd.rowptr[:-1]).long()
    print(f"graph: N={graph.n} E={graph.nnz} max degree={int(deg.max())}", flush=True)
    seed = torch.tensor([20], dtype=torch.int64, device=dev)
    if args.weighted:
        return weighted_leg(args, torch, pg, graph, deg, seed)
    for n_seeds in (int(s) for s in args.seeds.split(",")):
        seeds = torch.randperm(graph.n, device=dev, generator=torch.Generator(device=dev).manual_seed(n_seeds))[:n_seeds]
        for fan in args.fanouts.split("/"):
            fanouts = [int(f) for f in fan.split(",")]
            blocks = pg.sample_blocks(graph, seeds, fanouts, seed=seed)[::-1]                # hop order
            hops = []
            for t, blk in enumerate(blocks):
                dst, fanout = blk.dst_nodes, fanouts[-1 - t]
                ours = lambda: pg.sample_neighbors(graph, dst, fanout, seed=seed, hop=t)    # noqa: E731
                theirs = lambda: torch_hop(pg, torch, graph, dst, fanout)                    # noqa: E731
                pattern, src, cand = theirs()
                assert pattern.nnz == blk.nnz and int(deg[dst].sum()) == cand, "both keep min(degree, fanout) entries per row"
                sa, sb = alternate(torch, args, ours, theirs)
                hops.append(dict(hop=t, n_dst=blk.n_dst, fanout=fanout, candidates=cand, philox_calls_per_pass=-(-cand // 4), kept=blk.nnz,
                                 n_src=blk.n_src, baseline_n_src=int(src.numel()), long_rows=int((deg[dst] > 256).sum()),
                                 longest_row=int(deg[dst].max()), sampler=sa, composition=sb,
                                 composition_over_sampler=round(sb["median_ms"] / sa["median_ms"], 3),
                                 kept_per_s=round(blk.nnz / (sa["median_ms"] * 1e-3)), candidates_per_s=round(cand / (sa["median_ms"] * 1e-3))))
                print(json.dumps(hops[-1]), flush=True)
            whole = summary([timed(torch, lambda: pg.sample_blocks(graph, seeds, fanouts, seed=seed), args.steps) for _ in range(args.rounds)])
            line = dict(tool="sample_bench", device=torch.cuda.get_device_name(0), graph=f"rmat scale {args.scale}", N=graph.n, E=graph.nnz,
                        seeds=n_seeds, fanouts=fanouts, rounds=args.rounds, steps=args.steps, sample_blocks=whole,
                        sum_of_hops_sampler_ms=round(sum(h["sampler"]["median_ms"] for h in hops), 4),
                        sum_of_hops_composition_ms=round(sum(h["composition"]["median_ms"] for h in hops), 4), hops=hops)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            print(f"seeds={n_seeds} fanouts={fanouts}: sample_blocks {whole['median_ms']} ms, composition "
                  f"{line['sum_of_hops_composition_ms']} ms", flush=True)


if __name__ == "__main__":
    main()
