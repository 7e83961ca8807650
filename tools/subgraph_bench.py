#!/usr/bin/env python3
"""What pygat_amd.induced_subgraph and pygat_amd.random_walk cost on the headline R-MAT graph (pygat_amd.rmat.rmat_csr, 2^20 nodes,
drawn on the device) against torch compositions on the same device:

    python tools/subgraph_bench.py [--sets 16384,131072] [--roots 4096,32768] [--length 4] [--rounds 5] [--steps 5] [--warmup 3]
                                   [--out profiles/subgraph_bench.jsonl]
    python tools/subgraph_bench.py --footprints profiles/subgraph_footprints.txt     # pygat_kernel_footprint of the K23 kernels, nothing timed

Node sets: `--sets` ids drawn uniformly without repeats, and the flattened walks of `--roots` roots x `--length` steps (repeats and
all).  Three measurements per set, each alternated with its counterpart round by round in this one process (the conventions of
tools/sample_bench.py, whose timed() and summary() are used: every call between two host clock reads with a device synchronise before
the first and after the call; the median over all rounds x steps calls and the spread of the rounds' medians):

  subgraph      induced_subgraph up to rowptr / col / edge_ids, against the composition: a mark table, nonzero of the kept entries
                (mark[row] & mark[col] over ALL entries of the graph; the row of every entry is the graph's own edge_rc), a relabel
                through a rank table (cumsum of the marks), bincount + cumsum for rowptr.  Both results are compared, integer for
                integer, before anything is timed.
  graph         the time to the first use of sub.graph: CSRGraph(rowptr, col, validate=False) on the sub-pattern -- the existing
                construction (edge pairs, mirror permutation or transpose, slot structures), not K23's; here so that the reader sees
                it beside the call that feeds it.  It has no counterpart.
  walk          random_walk, against a torch loop of `length` gather steps (torch.randint keys, the same high-word pick).  The two
                draw different walks; only the time is compared.

Recorded, not gated.  One JSON object per node set, appended."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sample_bench import alternate, footprints, summary, timed    # noqa: E402  (the shared timing conventions and footprint writer)

K23_KERNELS = ("k23_mark", "k23_nodes", "k23_count_rows", "k23_list", "k23_count_long", "k23_empties", "k23_info", "k23_fill_rows",
               "k23_fill_long", "k23_walk")


def torch_subgraph(torch, graph, row64, col64, nodes):
    """The sub-pattern on `nodes` from torch ops -> (rowptr int32, col int32, edge_ids int64)."""
    mark = torch.zeros(graph.n, dtype=torch.bool, device=nodes.device)
    mark[nodes] = True
    pos = torch.nonzero(mark[row64] & mark[col64]).flatten()                       # (a host read: the number of kept entries)
    rank = torch.cumsum(mark, 0) - 1
    n = int(rank[-1]) + 1                                                          # (a host read: the number of nodes)
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=nodes.device)
    rowptr[1:] = torch.cumsum(torch.bincount(rank[row64[pos]], minlength=n), 0)
    return rowptr.to(torch.int32), rank[col64[pos]].to(torch.int32), pos


def torch_walk(torch, rp64, col64, start, length):
    cur, out = start, [start]
    for _ in range(length):
        b = rp64[cur]
        d = rp64[cur + 1] - b
        k = torch.randint(0, 2 ** 32, cur.shape, dtype=torch.int64, device=cur.device)
        cur = torch.where(d > 0, col64[torch.clamp(b + ((k * d) >> 32), max=col64.numel() - 1)], cur)
        out.append(cur)
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--footprints", default=None)
    ap.add_argument("--sets", default="16384,131072")
    ap.add_argument("--roots", default="4096,32768")
    ap.add_argument("--length", type=int, default=4)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgraph_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr
    if not torch.cuda.is_available():
        raise SystemExit("subgraph_bench: needs a GPU (there is nothing to time without one)")
    if args.footprints:
        return footprints(torch, args.footprints, "K23", K23_KERNELS)
    dev = "cuda"
    rowptr, col = rmat_csr(scale=args.scale, device=dev)
    graph = pg.CSRGraph(rowptr, col)
    rp64, col64, row64 = graph.fwd.rowptr.long(), graph.fwd.col.long(), graph.fwd.edge_rc[:, 0].long()
    deg = rp64[1:] - rp64[:-1]
    print(f"graph: N={graph.n} E={graph.nnz} max degree={int(deg.max())}", flush=True)
    seed = torch.tensor([23], dtype=torch.int64, device=dev)
    sets = []
    for k in (int(s) for s in args.sets.split(",")):
        sets.append((f"uniform {k}", torch.randperm(graph.n, device=dev, generator=torch.Generator(device=dev).manual_seed(k))[:k], None))
    for k in (int(s) for s in args.roots.split(",")):
        roots = torch.randperm(graph.n, device=dev, generator=torch.Generator(device=dev).manual_seed(k + 1))[:k]
        sets.append((f"walks of {k} roots x {args.length}", pg.random_walk(graph, roots, args.length, seed=seed).flatten(), roots))
    for what, nodes, roots in sets:
        sub = pg.induced_subgraph(graph, nodes)
        t_rowptr, t_col, t_ids = torch_subgraph(torch, graph, row64, col64, nodes)
        assert torch.equal(sub.rowptr, t_rowptr) and torch.equal(sub.col, t_col) and torch.equal(sub.edge_ids, t_ids), what
        ours, theirs = alternate(torch, args, lambda: pg.induced_subgraph(graph, nodes),
                                 lambda: torch_subgraph(torch, graph, row64, col64, nodes))
        build = lambda: pg.CSRGraph(sub.rowptr, sub.col, validate=False)    # noqa: E731
        for _ in range(args.warmup):
            build()
        first_use = summary([timed(torch, build, args.steps) for _ in range(args.rounds)]) if sub.n_empty_rows == 0 else None
        line = dict(tool="subgraph_bench", device=torch.cuda.get_device_name(0), graph=f"rmat scale {args.scale}", N=graph.n, E=graph.nnz,
                    nodes=what, n_in=int(nodes.numel()), n=sub.n, nnz=sub.nnz, n_empty_rows=sub.n_empty_rows,
                    long_rows=int((deg[sub.nodes] > 256).sum()), longest_row=int(deg[sub.nodes].max()),
                    row_entries_examined=int(deg[sub.nodes].sum()), rounds=args.rounds, steps=args.steps,
                    induced_subgraph=ours, composition=theirs, composition_over_induced_subgraph=round(theirs["median_ms"] / ours["median_ms"], 3),
                    csrgraph_first_use=first_use)
        if roots is not None:
            start = roots
            w_ours, w_theirs = alternate(torch, args, lambda: pg.random_walk(graph, start, args.length, seed=seed),
                                         lambda: torch_walk(torch, rp64, col64, start, args.length))
            line.update(n_walk=int(start.numel()), length=args.length, random_walk=w_ours, torch_walk=w_theirs,
                        torch_walk_over_random_walk=round(w_theirs["median_ms"] / w_ours["median_ms"], 3))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
