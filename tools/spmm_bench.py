#!/usr/bin/env python3
"""What pygat_amd.spmm costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py), H heads of
F columns (default 8 x 16), row-softmax values, against the same product through torch.sparse, one head at a time, in the same
process on the same GPU:

    python tools/spmm_bench.py [--heads 8] [--fout 16] [--reps 20] [--warmup 5] [--out profiles/spmm_bench.json]

Times are HIP events around `reps` calls after `warmup` calls of the same shape, forward alone and forward + backward (both
gradients).  Algorithmic bytes of the forward: E (4 H + 8) + (E + N) 4 H F -- the values, the column index and the permutation
entry of every entry, one gathered row per entry and one written row per node; the fraction of the 8 TB/s HBM roof is those bytes
over the measured time (a gathered row that hits a cache costs less than its bytes, so the figure is not a bandwidth).  Recorded,
not gated.  One JSON object."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROOF = 8.0e12     # bytes / s, MI355X HBM3E


def forward_bytes(N, E, H, F):
    return E * (4 * H + 8) + (E + N) * 4 * H * F


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--fout", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--draws", type=int, default=5_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spmm_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("spmm_bench: needs a GPU (a time taken anywhere else says nothing)")
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(args.scale, args.draws, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    pattern = graph.edge_pattern()
    N, E, H, F = graph.n, graph.nnz, args.heads, args.fout
    g = torch.Generator(device=dev).manual_seed(2)
    index = graph.edge_index()
    logits = torch.randn(E, H, generator=g, device=dev)
    m = torch.full((N, H), -float("inf"), device=dev).scatter_reduce(0, index[0][:, None].expand(-1, H), logits, "amax")
    p = torch.exp(logits - m[index[0]])
    values = (p / torch.zeros(N, H, device=dev).index_add(0, index[0], p)[index[0]]).requires_grad_(True)
    b = torch.randn(N, H, F, generator=g, device=dev).requires_grad_(True)
    G = torch.randn(N, H, F, generator=g, device=dev)
    del logits, m, p

    def ours_fwd():
        with torch.no_grad():
            return pg.spmm(pattern, values, b)

    def ours_fwd_bwd():
        return torch.autograd.grad(pg.spmm(pattern, values, b), [values, b], G)

    def sparse_out():
        return torch.stack([torch.sparse.mm(torch.sparse_coo_tensor(index, values[:, h], (N, N)), b[:, h]) for h in range(H)], 1)

    def sparse_fwd():
        with torch.no_grad():
            return sparse_out()

    def sparse_fwd_bwd():
        return torch.autograd.grad(sparse_out(), [values, b], G)

    with torch.no_grad():
        diff = float((ours_fwd() - sparse_fwd()).abs().max())
    res = {"device": torch.cuda.get_device_name(0), "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E,
           "H": H, "F": F, "reps": args.reps, "warmup": args.warmup, "max_abs_diff_vs_torch_sparse": diff,
           "forward_bytes": forward_bytes(N, E, H, F), "roof_bytes_per_s": ROOF}
    for name, fn in (("spmm_forward_ms", ours_fwd), ("spmm_forward_backward_ms", ours_fwd_bwd),
                     ("torch_sparse_forward_ms", sparse_fwd), ("torch_sparse_forward_backward_ms", sparse_fwd_bwd)):
        try:
            res[name] = timed(fn, args.reps, args.warmup)
        except RuntimeError as e:        # (torch.sparse's side only: ours raises ValueError or fails the run)
            if name.startswith("spmm"):
                raise
            res[name] = f"failed: {str(e).splitlines()[0]}"
    res["spmm_forward_fraction_of_roof"] = res["forward_bytes"] / ROOF / (res["spmm_forward_ms"] * 1e-3)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
