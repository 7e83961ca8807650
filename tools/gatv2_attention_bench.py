#!/usr/bin/env python3
"""What pygat_amd.gatv2_attention costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py)
against the same result from the parts it fuses -- two torch gathers and their sum, leaky_relu, the product with a and its sum over the
features, edge_softmax (K18) and spmm (pygat_spmm_forward) -- at H x F = 8x16 and 8x64, N(0, 1) tensors, slope 0.2, with v shared
(v=None: v is x_src) and with a v table of its own, the forward alone and forward + backward:

    python tools/gatv2_attention_bench.py [--shapes 8x16,8x64] [--values shared,separate] [--rounds 5] [--steps 10] [--warmup 10]
                                          [--dropout | --edge] [--out profiles/gatv2_attention_bench.jsonl]
    python tools/gatv2_attention_bench.py --tables-bf16 [--edge] [...]      # gatv2_attention_bf16 (gatv2_attention_edge_bf16): the fp32
                                          # fused forward against the bf16 one -> profiles/gatv2_attention_bf16_bench.jsonl (..._edge_bf16_...)

The measuring step runs in a child process under `timeout -k 10 <--limit seconds>`; this process never opens the GPU.  Both contenders
run in that one process, alternated round by round, timed as tools/dot_attention_bench.py times its own (`alternate`, imported): a
round times `steps` calls of one contender, each between two HIP events, then the same of the other.  Reported per contender: the
median over all rounds x steps timed calls (at least 50) and the spread of the rounds' medians: a difference below that spread is
not a difference.  The composition is the baseline: it runs kernels and torch ops that exist without K21, on the same build.

Before timing, both contenders' outputs are priced on the same seeded inputs by the rule of tests/parity.py against an fp64
computation on the CPU, on a sample of rows (the row of most entries among them).  Algorithmic bytes are computed from the shapes (E
entries, N rows, M columns, H heads, R = H F floats per row), `*_bytes` below; `*_roof_ms` is their time at 8 TB/s, and
`*_roof_fraction` that over the measured time: the whole op's share of the HBM roof on the byte model, not a kernel's.  Recorded, not
gated.  One JSON object per (shape, value table), appended.

--edge measures pygat_amd.gatv2_attention_edge, e [E, H, F] ~ N(0, 1) inside the score, against the same composition with e added
before leaky_relu, at 8x16 and 8x32 by default (an [E, R] tensor is 5.5 and 11 GB there; at 8x64 it is 22 GB, and the composition,
which keeps some ten of them for autograd, runs only where the device has the room: otherwise the fused op is recorded alone and the
line says so), into profiles/gatv2_attention_edge_bench.jsonl.

--tables-bf16 measures the inference forwards on bfloat16 tables (forward only), as tools/dot_attention_bench.py --kv-bf16 does for
K19: in the one child process it alternates the fused forward on float32 tables with the fused forward on bfloat16 tables -- x_src,
the separate v and, with --edge, e.  Both are fed the same values -- N(0, 1) draws rounded to bfloat16, and those widened to float32
-- so the two outputs are compared with torch.equal here (asserted); the bfloat16 one is priced on the sampled rows as above.
Recorded per (shape, value table): both medians with their spreads, their ratio, and the byte model's ratio beside it.  The yardstick
is the float32 forward of the same run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SAMPLE_ROWS = 1024
HBM_BYTES_PER_S = 8e12
SECTOR = 32          # bytes: the granularity at which the H floats of S[c] are counted


def sectors(nbytes):
    return -(-nbytes // SECTOR) * SECTOR


def fused_forward_bytes(E, N, M, H, F, shared):
    """Per entry: the column index and the x_src row (shared: that is the value row too; separate: the v row besides).  Per row:
    x_dst read, out, m and Z written, the row pointer."""
    R = H * F
    return E * (4 + (1 if shared else 2) * 4 * R) + N * (2 * 4 * R + 2 * 4 * H + 4)


def bf16_forward_bytes(E, N, M, H, F, shared, edge=False, perm=False):
    """bfloat16 x_src, v and e tables (inference): their rows at 2 bytes a value; x_dst read and out written in float32; m and Z are
    not written; with e the entry index where the pattern carries a permutation."""
    R = H * F
    return E * (4 + ((1 if shared else 2) + (1 if edge else 0)) * 2 * R + (4 if edge and perm else 0)) + N * (2 * 4 * R + 4)


def fused_backward_bytes(E, N, M, H, F, shared, perm=False):
    """Row pass: the forward's reads per entry (and the entry index where the pattern carries a permutation), P and S written; x_dst,
    G, out, m, Z read and dx_dst written per row.  Column pass on the transposed pattern: the row index, the entry index, the x_dst
    row and S at sector granularity per entry; x_src read and dx_src written per column (the da records are a few MB).  dv, K17 on
    the transposed pattern: P with the two indices and the G row per entry, dv per column; shared: the sum of dx_src's two parts."""
    R = H * F
    rows = E * (4 + (1 if shared else 2) * 4 * R + 2 * 4 * H + (4 if perm else 0)) + N * (4 * 4 * R + 2 * 4 * H + 4)
    cols = E * (8 + 4 * R + sectors(4 * H)) + M * (2 * 4 * R + 4)
    dv = E * (4 * H + 8 + 4 * R) + M * (4 * R + 4) + (M * 3 * 4 * R if shared else 0)
    return rows + cols + dv


def composed_forward_bytes(E, N, M, H, F):
    """The two gathers (an int64 index and a row read, [E, R] written, each), their sum (two reads and a write), leaky_relu and the
    product with a (a read and a write each), the sum over the features ([E, R] read, [E, H] written).  K18: the scores read by the
    row pass and again by the entry pass with the (row, col) pair, alpha written; m and Z per row.  SpMM: alpha, the column index and
    the v row per entry, out per row."""
    R = H * F
    score = 2 * E * (8 + 2 * 4 * R) + E * 3 * 4 * R + 2 * E * 2 * 4 * R + E * (4 * R + 4 * H)
    softmax = E * (3 * 4 * H + 8) + N * (2 * 2 * 4 * H + 4)
    spmm = E * (4 * H + 4 + 4 * R) + N * (4 * R + 4)
    return score + softmax + spmm


def composed_backward_bytes(E, N, M, H, F):
    """SpMM's backward: an SDDMM over G and v (dalpha written) and the transposed SpMM of alpha and G (dv).  K18's backward: alpha and
    dalpha read by both passes, dscores written, c per row.  The sum's backward broadcasts ([E, H] read, [E, R] written); the
    product's gives da ([E, R] read twice, reduced) and the gradient of leaky_relu's output (two reads and a write); leaky_relu's
    backward (two reads and a write); the two gathers' backwards: [E, R] and an int64 index read and added into [N, R] and [M, R]
    tables that were zeroed first."""
    R = H * F
    spmm_b = E * (2 * 4 * R + 8 + 4 * H) + E * (4 * H + 8 + 4 * R) + M * (4 * R + 4)
    softmax_b = E * (5 * 4 * H + 8) + N * (2 * 4 * H + 4)
    score_b = E * (4 * H + 4 * R) + E * 2 * 4 * R + 2 * E * 3 * 4 * R + 2 * E * (8 + 3 * 4 * R) + (N + M) * 4 * R
    return spmm_b + softmax_b + score_b


def sampled_reference(rp, col, rows, x_dst, x_src, a, v, slope, dtype, mask=None, e=None):
    """out of `rows` by torch on the CPU in `dtype`: the softmax over each row's entries of a . leaky_relu(x_dst_i + x_src_j), times
    mask (the dropout's, [E, H] at the CSR position, after the softmax), times v_j; the rows a few hundred at a time, so that no
    [entries, H, F] tensor grows beyond them.  e: the edge rows of --edge, [E, H, F] at the CSR position, added behind x_dst_i + x_src_j."""
    import torch
    ad = a.cpu().to(dtype)
    outs = []
    for part in torch.split(rows, 256):
        deg = rp[part + 1] - rp[part]
        idx = torch.cat([torch.arange(int(rp[r]), int(rp[r + 1])) for r in part.tolist()])
        sub = torch.repeat_interleave(torch.arange(part.numel()), deg)
        cols, inv = torch.unique(col[idx], return_inverse=True)
        xd, xs, vs = x_dst[part].cpu().to(dtype), x_src[cols].cpu().to(dtype), v[cols].cpu().to(dtype)
        t = xd[sub] + xs[inv]
        if e is not None:
            t = t + e[idx.to(e.device)].cpu().to(dtype)
        s = (ad * torch.nn.functional.leaky_relu(t, slope)).sum(-1)
        m = torch.full((part.numel(), s.shape[1]), -float("inf"), dtype=dtype).scatter_reduce(0, sub[:, None].expand(-1, s.shape[1]), s, "amax")
        p = torch.exp(s - m[sub])
        alpha = p / torch.zeros_like(m).index_add(0, sub, p)[sub]
        if mask is not None:
            alpha = alpha * mask[idx.to(mask.device)].cpu().to(dtype)
        outs.append(torch.zeros(part.numel(), v.shape[1], v.shape[2], dtype=dtype).index_add(0, sub, alpha[:, :, None] * vs[inv]))
    return torch.cat(outs)


def measure(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("gatv2_attention_bench: needs a GPU (a time taken anywhere else says nothing)")
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    from dot_attention_bench import alternate                        # the one timing routine of these tools
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity                                                     # the one tolerance rule (tests/parity.py)
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(args.scale, args.draws, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    pattern = graph.edge_pattern()
    pattern.transposed()
    N, E = graph.n, graph.nnz
    row_d, col_d = pattern.edge_rc[:, 0].long(), pattern.edge_rc[:, 1].long()
    rp_t, col_t = torch.from_numpy(rp).long(), torch.from_numpy(col).long()
    deg = rp_t[1:] - rp_t[:-1]
    picked = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:SAMPLE_ROWS]
    rows = torch.unique(torch.cat([picked, torch.argmax(deg)[None]]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    slope, perm = 0.2, pattern.perm is not None
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        for values in args.values.split(","):
            shared = values == "shared"
            g = torch.Generator(device=dev).manual_seed(2)
            x_dst, x_src = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(2))
            a = torch.randn(H, F, generator=g, device=dev)
            G = torch.randn(N, H, F, generator=g, device=dev)
            leaves = (x_dst, x_src, a) + (() if shared else (torch.randn(N, H, F, generator=g, device=dev),))

            def fused(xd, xs, a_, v_=None):
                return pg.gatv2_attention(pattern, xd, xs, a_, v_, slope)

            def composed(xd, xs, a_, v_=None):
                e = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d], slope)).sum(-1)
                return pg.spmm(pattern, pg.edge_softmax(pattern, e), xs if v_ is None else v_)

            def forward_of(fn):
                def run():
                    with torch.no_grad():
                        return fn(*leaves)
                return run

            def both_of(fn):
                mine = [t.detach().clone().requires_grad_(True) for t in leaves]

                def run():
                    return torch.autograd.grad(fn(*mine), mine, G)
                return run

            v = leaves[-1] if not shared else x_src
            if args.tables_bf16:
                measure_bf16(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, rp_t, col_t, deg, rows,
                             perm)
                del x_dst, x_src, a, G, leaves, v
                torch.cuda.empty_cache()
                continue
            if args.edge:
                measure_edge(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, v, G, row_d, col_d, rp_t,
                             col_t, deg, rows, perm)
                del x_dst, x_src, a, G, leaves, v
                torch.cuda.empty_cache()
                continue
            if args.dropout:
                measure_dropout(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, v, row_d, col_d, rp_t,
                                col_t, deg, rows, perm, forward_of, both_of, fused)
                del x_dst, x_src, a, G, leaves, v
                torch.cuda.empty_cache()
                continue
            # the same seeded inputs, both contenders priced on the sampled rows
            out_f, out_c = forward_of(fused)(), forward_of(composed)()
            ref64 = sampled_reference(rp_t, col_t, rows, x_dst, x_src, a, v, slope, torch.float64)
            ref32 = sampled_reference(rp_t, col_t, rows, x_dst, x_src, a, v, slope, torch.float32)
            err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} {values} fused out", ref32)
            err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} {values} composed out", ref32)
            res = {"bench": "gatv2_attention", "values": values, "device": torch.cuda.get_device_name(0),
                   "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
                   "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
                   "longest_checked_row": int(deg[rows].max()), "out_err_fused": err_f, "out_err_composed": err_c,
                   "out_err_fp32_reference": parity.err(ref32, ref64), "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
                   "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, shared),
                   "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F),
                   "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F, shared, perm),
                   "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F)}
            del out_f, out_c
            legs = [("forward", alternate({"fused": forward_of(fused), "composed": forward_of(composed)}, args.rounds, args.steps,
                                          args.warmup))]
            if not args.forward_only:
                legs.append(("forward_backward", alternate({"fused": both_of(fused), "composed": both_of(composed)}, args.rounds,
                                                           args.steps, args.warmup)))
            for what, r in legs:
                for name in ("fused", "composed"):
                    res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
                res[f"{what}_speedup"] = res[f"composed_{what}_ms"] / res[f"fused_{what}_ms"]
                model = res["fused_forward_bytes"] + (res["fused_backward_bytes"] if what == "forward_backward" else 0)
                res[f"fused_{what}_roof_ms"] = 1e3 * model / HBM_BYTES_PER_S
                res[f"fused_{what}_roof_fraction"] = res[f"fused_{what}_roof_ms"] / res[f"fused_{what}_ms"]
            res["peak_device_bytes"] = torch.cuda.max_memory_allocated(dev)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
            print(json.dumps(res), flush=True)
            del x_dst, x_src, a, G, leaves, v
            torch.cuda.empty_cache()


def measure_bf16(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, rp_t, col_t, deg, rows, perm):
    """--tables-bf16, one shape and one kind of v: the fused forward on float32 tables against gatv2_attention_bf16 on the bfloat16
    tables of the same values; with --edge gatv2_attention_edge against gatv2_attention_edge_bf16, e [E, H, F] among the tables; one
    JSON object."""
    N, E, shared = pattern.n_rows, pattern.nnz, values == "shared"
    x_dst, a = leaves[0], leaves[2]
    x16 = leaves[1].bfloat16()
    v16 = None if shared else leaves[3].bfloat16()
    e16 = torch.randn(E, H, F, generator=torch.Generator(device=dev).manual_seed(5), device=dev).bfloat16() if args.edge else None
    xw, vw, ew = (None if t is None else t.float() for t in (x16, v16, e16))      # the same values, widened: the float32 contender's

    def run_fp32():
        with torch.no_grad():
            if args.edge:
                return pg.gatv2_attention_edge(pattern, x_dst, xw, a, ew, vw, slope)
            return pg.gatv2_attention(pattern, x_dst, xw, a, vw, slope)

    def run_bf16():
        with torch.no_grad():
            if args.edge:
                return pg.gatv2_attention_edge_bf16(pattern, x_dst, x16, a, e16, v16, slope)
            return pg.gatv2_attention_bf16(pattern, x_dst, x16, a, v16, slope)

    out_w, out_h = run_fp32(), run_bf16()
    equal = bool(torch.equal(out_w, out_h))
    assert equal, f"{shape} {values}: the bf16 forward differs from the float32 forward on the widened tables"
    ref64 = sampled_reference(rp_t, col_t, rows, x_dst, xw, a, xw if shared else vw, slope, torch.float64, e=ew)
    ref32 = sampled_reference(rp_t, col_t, rows, x_dst, xw, a, xw if shared else vw, slope, torch.float32, e=ew)
    err_h = parity.close_fwd(out_h[rows.to(dev)], ref64, f"{shape} {values} fused, bf16 tables: out", ref32)
    fp32_bytes = fused_forward_bytes(E, N, N, H, F, shared) + (edge_bytes(E, H, F, perm)["fused_forward"] if args.edge else 0)
    res = {"bench": "gatv2_attention --tables-bf16" + (" --edge" if args.edge else ""), "values": values,
           "device": torch.cuda.get_device_name(0), "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H,
           "F": F, "negative_slope": slope, "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup,
           "checked_rows": int(rows.numel()), "longest_checked_row": int(deg[rows].max()),
           "out_bf16_equals_out_fp32_on_widened_tables": equal, "out_err_fused_bf16": err_h,
           "out_err_fp32_reference": parity.err(ref32, ref64), "fused_forward_bytes": fp32_bytes,
           "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F, shared, args.edge, perm)}
    res["byte_model_ratio"] = res["fused_bf16_forward_bytes"] / res["fused_forward_bytes"]
    del out_w, out_h
    r = alternate({"fused_fp32": run_fp32, "fused_bf16": run_bf16}, args.rounds, args.steps, args.warmup)
    for name in ("fused_fp32", "fused_bf16"):
        res[f"{name}_forward_ms"], res[f"{name}_forward_spread_ms"] = r[name]
        res[f"{name}_forward_roof_fraction"] = (1e3 * res["fused_bf16_forward_bytes" if name == "fused_bf16" else "fused_forward_bytes"]
                                                / HBM_BYTES_PER_S / res[f"{name}_forward_ms"])
    res["measured_ratio"] = res["fused_bf16_forward_ms"] / res["fused_fp32_forward_ms"]
    res["faster_by_more_than_the_spread"] = (res["fused_fp32_forward_ms"] - res["fused_bf16_forward_ms"]
                                             > max(res["fused_fp32_forward_spread_ms"], res["fused_bf16_forward_spread_ms"]))
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(dev)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)
    print(f"{shape} {values}: bf16 tables take {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
          f"{res['byte_model_ratio']:.3f}; outputs bit-equal", flush=True)


def measure_dropout(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, v, row_d, col_d, rp_t, col_t, deg,
                    rows, perm, forward_of, both_of, fused):
    """--dropout, one shape and one kind of v: fused with dropout, fused without, the composition with the mask as a tensor; one JSON
    object.  The fused op's algorithmic bytes are those without dropout -- the mask is drawn in registers -- but for the permutation
    entry the forward now reads where the pattern carries one (4 bytes an entry; this graph's pattern carries none)."""
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=dev)
    N, E, shared = pattern.n_rows, pattern.nnz, values == "shared"

    def fused_dropout(xd, xs, a_, v_=None):
        return pg.gatv2_attention_dropout(pattern, xd, xs, a_, p, v_, slope, seed=seed)

    def composed_dropout(xd, xs, a_, v_=None):
        e = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d], slope)).sum(-1)
        return pg.spmm(pattern, pg.edge_softmax(pattern, e) * pg.attention_dropout_mask(pattern, H, p, seed), xs if v_ is None else v_)

    contenders = {"fused_dropout": fused_dropout, "composed_dropout": composed_dropout, "fused": fused}
    out_f, out_c = forward_of(fused_dropout)(), forward_of(composed_dropout)()
    mask = pg.attention_dropout_mask(pattern, H, p, seed)
    ref64 = sampled_reference(rp_t, col_t, rows, *leaves[:3], v, slope, torch.float64, mask=mask)
    ref32 = sampled_reference(rp_t, col_t, rows, *leaves[:3], v, slope, torch.float32, mask=mask)
    err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} {values} fused, dropout: out", ref32)
    err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} {values} composed, dropout: out", ref32)
    res = {"bench": "gatv2_attention --dropout", "values": values, "device": torch.cuda.get_device_name(0), "p": p,
           "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
           "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
           "longest_checked_row": int(deg[rows].max()), "kept_fraction": float((mask != 0).float().mean()),
           "out_err_fused_dropout": err_f, "out_err_composed_dropout": err_c, "out_err_fp32_reference": parity.err(ref32, ref64),
           "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, shared),
           "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F, shared, perm),
           "fused_dropout_extra_forward_bytes": 4 * E if perm else 0, "mask_tensor_bytes": E * H * 4}
    del out_f, out_c, mask
    legs = [("forward", alternate({k: forward_of(fn) for k, fn in contenders.items()}, args.rounds, args.steps, args.warmup))]
    if not args.forward_only:
        legs.append(("forward_backward", alternate({k: both_of(fn) for k, fn in contenders.items()}, args.rounds, args.steps, args.warmup)))
    for what, r in legs:
        for name in contenders:
            res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
        res[f"{what}_speedup"] = res[f"composed_dropout_{what}_ms"] / res[f"fused_dropout_{what}_ms"]
        res[f"dropout_{what}_measured_increment"] = res[f"fused_dropout_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(dev)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)
    print(f"{shape} {values}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged "
          f"bytes; the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)


def edge_bytes(E, H, F, perm=False):
    """What e adds to the byte models, R = H F: the fused op reads the entry's e row once in each of its three passes (and the entry
    index in the forward where the pattern carries a permutation) and writes de once; the composition has one more elementwise add in
    its forward (two [E, R] reads and a write) and none in its backward: the add hands its incoming gradient on as de."""
    R = H * F
    return {"fused_forward": E * 4 * R + (4 * E if perm else 0), "fused_backward": 3 * E * 4 * R, "composed_forward": 3 * E * 4 * R,
            "composed_backward": 0}


def measure_edge(args, torch, pg, parity, alternate, dev, pattern, shape, values, H, F, slope, leaves, v, G, row_d, col_d, rp_t, col_t, deg,
                 rows, perm):
    """--edge, one shape and one kind of v: gatv2_attention_edge against the composition with e inside leaky_relu; one JSON object.
    Every gradient is asked for, de among them."""
    N, E, shared = pattern.n_rows, pattern.nnz, values == "shared"
    R = H * F
    e = torch.randn(E, H, F, generator=torch.Generator(device=dev).manual_seed(5), device=dev)
    leaves = leaves + (e,)

    def fused(xd, xs, a_, *rest):
        return pg.gatv2_attention_edge(pattern, xd, xs, a_, rest[-1], None if shared else rest[0], slope)

    def composed(xd, xs, a_, *rest):
        s = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d] + rest[-1], slope)).sum(-1)
        return pg.spmm(pattern, pg.edge_softmax(pattern, s), xs if shared else rest[0])

    def forward_of(fn):
        def run():
            with torch.no_grad():
                return fn(*leaves)
        return run

    def both_of(fn):
        mine = [t.detach().clone().requires_grad_(True) for t in leaves]

        def run():
            return torch.autograd.grad(fn(*mine), mine, G)
        return run

    # the composition keeps the two gathers, their sum, the sum with e, leaky_relu's output and the product for autograd, and its
    # backward holds as many gradients at its peak: some fourteen [E, R] tensors with the two copies of e
    free, _ = torch.cuda.mem_get_info(dev)
    need = 14 * E * 4 * R
    with_composed = need <= free
    extra = edge_bytes(E, H, F, perm)
    out_f = forward_of(fused)()
    ref64 = sampled_reference(rp_t, col_t, rows, *leaves[:3], v, slope, torch.float64, e=e)
    ref32 = sampled_reference(rp_t, col_t, rows, *leaves[:3], v, slope, torch.float32, e=e)
    res = {"bench": "gatv2_attention --edge", "values": values, "device": torch.cuda.get_device_name(0),
           "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
           "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
           "longest_checked_row": int(deg[rows].max()), "e_tensor_bytes": E * 4 * R,
           "out_err_fused": parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} {values} fused, edge: out", ref32),
           "out_err_fp32_reference": parity.err(ref32, ref64),
           "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, shared) + extra["fused_forward"],
           "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F, shared, perm) + extra["fused_backward"],
           "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F) + extra["composed_forward"],
           "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F) + extra["composed_backward"]}
    contenders = {"fused": fused}
    if with_composed:
        out_c = forward_of(composed)()
        res["out_err_composed"] = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} {values} composed, edge: out", ref32)
        res["out_max_abs_fused_minus_composed"] = float((out_f - out_c).abs().max())
        contenders["composed"] = composed
        del out_c
    else:
        res["composed"] = (f"not run: some {need / 2 ** 30:.0f} GiB for its [E, R] tensors against {free / 2 ** 30:.0f} GiB free; "
                           f"the fused op is recorded alone")
    del out_f
    legs = [("forward", alternate({k: forward_of(fn) for k, fn in contenders.items()}, args.rounds, args.steps, args.warmup))]
    if not args.forward_only:
        legs.append(("forward_backward", alternate({k: both_of(fn) for k, fn in contenders.items()}, args.rounds, args.steps, args.warmup)))
    for what, r in legs:
        for name in contenders:
            res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
        model = res["fused_forward_bytes"] + (res["fused_backward_bytes"] if what == "forward_backward" else 0)
        other = res["composed_forward_bytes"] + (res["composed_backward_bytes"] if what == "forward_backward" else 0)
        res[f"{what}_bytes_ratio_model"] = other / model
        res[f"fused_{what}_roof_ms"] = 1e3 * model / HBM_BYTES_PER_S
        res[f"fused_{what}_roof_fraction"] = res[f"fused_{what}_roof_ms"] / res[f"fused_{what}_ms"]
        if with_composed:
            res[f"{what}_speedup"] = res[f"composed_{what}_ms"] / res[f"fused_{what}_ms"]
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(dev)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=None, help="8x16,8x64; under --edge 8x16,8x32")
    ap.add_argument("--values", default="shared,separate", help="shared: v=None, v is x_src; separate: a v table of its own")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed calls per round and contender")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true", help="skip the forward + backward leg")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--draws", type=int, default=5_000_000)
    ap.add_argument("--limit", type=int, default=540, help="seconds the measuring child may take")
    ap.add_argument("--dropout", action="store_true", help="gatv2_attention_dropout at p = 0.5 against the op without dropout and the "
                    "composition with the mask as a tensor")
    ap.add_argument("--edge", action="store_true", help="gatv2_attention_edge, e [E, H, F] inside the score, against the composition "
                    "with e added before leaky_relu")
    ap.add_argument("--tables-bf16", action="store_true", help="gatv2_attention_bf16 (with --edge: gatv2_attention_edge_bf16): the fused "
                    "forward on float32 tables against the fused forward on the bfloat16 tables of the same values (forward only)")
    ap.add_argument("--out", default=None, help="profiles/gatv2_attention_bench.jsonl, or ..._dropout_bench.jsonl under --dropout, "
                    "..._edge_bench.jsonl under --edge, ..._bf16_bench.jsonl and ..._edge_bf16_bench.jsonl under --tables-bf16")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.edge and args.dropout:
        ap.error("--edge and --dropout are two measurements: there is no op with both")
    if args.shapes is None:
        args.shapes = "8x16,8x32" if args.edge else "8x16,8x64"
    if args.tables_bf16 and args.dropout:
        ap.error("--tables-bf16 and --dropout are two measurements: there is no op with both")
    if args.out is None and args.tables_bf16:
        args.out = os.path.join(ROOT, "profiles", "gatv2_attention_edge_bf16_bench.jsonl" if args.edge else "gatv2_attention_bf16_bench.jsonl")
    if args.out is None:
        name = "gatv2_attention_edge_bench.jsonl" if args.edge else "gatv2_attention_dropout_bench.jsonl" if args.dropout else \
            "gatv2_attention_bench.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
