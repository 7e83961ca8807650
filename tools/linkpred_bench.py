#!/usr/bin/env python3
"""What pygat_amd.find_edges, negative_edges and link_batch cost on the headline R-MAT graph (pygat_amd.rmat.rmat_csr, 2^20 nodes, drawn
on the device) against torch compositions on the same device:

    python tools/linkpred_bench.py [--pairs 1024,65536,1048576] [--src 1024,65536] [--negs 1,5] [--batch 1024] [--num-neg 5] [--fanouts 10,25]
                                   [--rounds 5] [--steps 5] [--warmup 3] [--out profiles/linkpred_bench.jsonl]
    python tools/linkpred_bench.py --footprints profiles/linkpred_footprints.txt     # pygat_kernel_footprint of the K24 kernels, nothing timed

Each measurement is alternated with its counterpart round by round in this one process (the conventions of tools/sample_bench.py, whose
timed() and summary() are used: every call between two host clock reads with a device synchronise before the first and after the
call; the median over all rounds x steps calls and the spread of the rounds' medians):

  find      find_edges on n pairs -- half of them entries of the graph at random positions, half random pairs -- against
            torch.searchsorted over the int64 keys row * N + col of all entries (sorted as the CSR stands).  The key table is built
            once per graph; its build time is reported apart (key_table_build).  Results are compared, integer for integer, first.
  negatives negative_edges for n_src sources (the rows of random entries: link prediction's sources) x num_neg, against the torch
            rejection loop: randint, the same searchsorted membership test (and the source itself), redrawn until none is left -- one
            host read per trip.  The two draw different ids; only the time is compared (and that no draw of either is an entry).
  batch     link_batch, and its parts run by hand one after the other: the endpoints' gather, negative_edges, torch.unique, the
            weights (zeroing and restoring the excluded positions), sample_blocks_weighted, the pair pattern.

Recorded, not gated.  One JSON object per configuration, appended."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sample_bench import alternate, footprints, summary, timed    # noqa: E402  (the shared timing conventions and footprint writer)

K24_KERNELS = ("k24_find", "k24_draw")


def torch_find(torch, keys, N, row, col):
    q = row * N + col
    idx = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
    return torch.where(keys[idx] == q, idx, torch.full_like(idx, -1))


def torch_negatives(torch, keys, N, src, num_neg):
    """-> (neg [n_src, num_neg], trips of the loop)"""
    u = src.repeat_interleave(num_neg)
    out = torch.randint(0, N, u.shape, dtype=torch.int64, device=u.device)
    todo = torch.arange(u.numel(), device=u.device)
    trips = 0
    while True:
        trips += 1
        uu, vv = u[todo], out[todo]
        q = uu * N + vv
        idx = torch.searchsorted(keys, q).clamp_(max=keys.numel() - 1)
        todo = todo[(keys[idx] == q) | (uu == vv)]                     # (a host read: the number of draws to repeat)
        if todo.numel() == 0:
            return out.view(-1, num_neg), trips
        out[todo] = torch.randint(0, N, todo.shape, dtype=torch.int64, device=u.device)


def alone(torch, args, fn):
    for _ in range(args.warmup):
        fn()
    return summary([timed(torch, fn, args.steps) for _ in range(args.rounds)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--footprints", default=None)
    ap.add_argument("--pairs", default="1024,65536,1048576")
    ap.add_argument("--src", default="1024,65536")
    ap.add_argument("--negs", default="1,5")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--num-neg", type=int, default=5)
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linkpred_bench.jsonl"))
    args = ap.parse_args()
    import torch
    import pygat_amd as pg
    from pygat_amd import linkpred
    from pygat_amd.rmat import rmat_csr
    if not torch.cuda.is_available():
        raise SystemExit("linkpred_bench: needs a GPU (there is nothing to time without one)")
    if args.footprints:
        return footprints(torch, args.footprints, "K24", K24_KERNELS)
    dev = "cuda"
    rowptr, col = rmat_csr(scale=args.scale, device=dev)
    graph = pg.CSRGraph(rowptr, col)
    N, E = graph.n, graph.nnz
    col64, row64 = graph.fwd.col.long(), graph.fwd.edge_rc[:, 0].long()
    deg = graph.fwd.rowptr[1:].long() - graph.fwd.rowptr[:-1].long()
    print(f"graph: N={N} E={E} max degree={int(deg.max())} symmetric={graph.symmetric}", flush=True)
    head = dict(tool="linkpred_bench", device=torch.cuda.get_device_name(0), graph=f"rmat scale {args.scale}", N=N, E=E,
                rounds=args.rounds, steps=args.steps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def record(line):
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        print(json.dumps(line), flush=True)

    keys = row64 * N + col64
    key_build = alone(torch, args, lambda: graph.fwd.edge_rc[:, 0].long() * N + graph.fwd.col.long())
    gen = torch.Generator(device=dev).manual_seed(24)
    seed = torch.tensor([24], dtype=torch.int64, device=dev)

    for n in (int(s) for s in args.pairs.split(",")):
        at = torch.randint(0, E, (n // 2,), device=dev, generator=gen)
        row = torch.cat([row64[at], torch.randint(0, N, (n - n // 2,), device=dev, generator=gen)])
        colq = torch.cat([col64[at], torch.randint(0, N, (n - n // 2,), device=dev, generator=gen)])
        pos = pg.find_edges(graph, row, colq)
        assert torch.equal(pos, torch_find(torch, keys, N, row, colq)) and torch.equal(pos[:n // 2], at), n
        ours, theirs = alternate(torch, args, lambda: pg.find_edges(graph, row, colq), lambda: torch_find(torch, keys, N, row, colq))
        record(dict(head, what="find", n_pairs=n, found=int((pos >= 0).sum()), find_edges=ours, searchsorted=theirs,
                    searchsorted_over_find_edges=round(theirs["median_ms"] / ours["median_ms"], 3), key_table_build=key_build))

    for n_src in (int(s) for s in args.src.split(",")):
        src = row64[torch.randint(0, E, (n_src,), device=dev, generator=gen)]
        for num_neg in (int(s) for s in args.negs.split(",")):
            neg = pg.negative_edges(graph, src, num_neg, seed=seed)
            t_neg, trips = torch_negatives(torch, keys, N, src, num_neg)
            u = src.repeat_interleave(num_neg)
            for drawn in (neg, t_neg):
                assert bool((pg.find_edges(graph, u, drawn.flatten()) == -1).all()) and bool((drawn.flatten() != u).all())
            ours, theirs = alternate(torch, args, lambda: pg.negative_edges(graph, src, num_neg, seed=seed),
                                     lambda: torch_negatives(torch, keys, N, src, num_neg))
            record(dict(head, what="negatives", n_src=n_src, num_neg=num_neg, mean_degree_of_src=round(float(deg[src].float().mean()), 1),
                        largest_degree_of_src=int(deg[src].max()), rejection_trips=trips, negative_edges=ours, rejection_loop=theirs,
                        rejection_loop_over_negative_edges=round(theirs["median_ms"] / ours["median_ms"], 3)))

    B, K, fanouts = args.batch, args.num_neg, [int(s) for s in args.fanouts.split(",")]
    off = torch.nonzero(row64 != col64).flatten()
    edge_ids = off[torch.randint(0, off.numel(), (B,), device=dev, generator=gen)]
    rev_first = timed(torch, graph.reverse_edge_ids, 1)[0]             # (once per graph: perm_f on a symmetric pattern)
    batch = pg.link_batch(graph, edge_ids, K, fanouts, seed=seed)
    u, v = graph.fwd.edge_rc[edge_ids, 0].long(), col64[edge_ids]
    neg = pg.negative_edges(graph, u, K, seed=seed)
    seeds, inv = torch.unique(torch.cat([u, v, neg.flatten()]), sorted=True, return_inverse=True)
    excluded = linkpred._excluded(graph, edge_ids, "reverse")
    w = graph._link_w
    rows = torch.cat([inv[:B], inv[:B].repeat_interleave(K)])

    def weights():
        w[excluded] = 0.0
        w[excluded] = 1.0
    parts = dict(
        endpoints=alone(torch, args, lambda: (graph.fwd.edge_rc[edge_ids, 0].long(), graph.fwd.col[edge_ids].long())),
        negative_edges=alone(torch, args, lambda: pg.negative_edges(graph, u, K, seed=seed)),
        unique=alone(torch, args, lambda: torch.unique(torch.cat([u, v, neg.flatten()]), sorted=True, return_inverse=True)),
        weights=alone(torch, args, weights),
        sample_blocks_weighted=alone(torch, args, lambda: pg.sample_blocks_weighted(graph, seeds, fanouts, w, seed=seed)),
        pairs=alone(torch, args, lambda: pg.EdgePattern.from_indices(torch.stack([rows, inv[B:]]), (seeds.numel(), seeds.numel()))))
    whole = alone(torch, args, lambda: pg.link_batch(graph, edge_ids, K, fanouts, seed=seed))
    record(dict(head, what="batch", B=B, num_neg=K, fanouts=fanouts, n_seeds=int(seeds.numel()),
                block_entries=[blk.nnz for blk in batch.blocks], block_sources=[blk.n_src for blk in batch.blocks],
                reverse_edge_ids_first_ms=round(rev_first, 4), link_batch=whole, parts=parts,
                parts_sum_ms=round(sum(p["median_ms"] for p in parts.values()), 4)))


if __name__ == "__main__":
    main()
