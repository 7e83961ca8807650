#!/usr/bin/env python3
"""What pygat_amd.additive_attention costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py)
against the same result from the parts it fuses -- two torch gathers and their sum, leaky_relu, edge_softmax (K18) and spmm
(pygat_spmm_forward) -- at H x F = 8x16 and 8x64, N(0, 1) tensors, slope 0.2, the forward alone and forward + backward:

    python tools/additive_attention_bench.py [--shapes 8x16,8x64] [--rounds 5] [--steps 10] [--warmup 10] [--out profiles/additive_attention_bench.jsonl]
    python tools/additive_attention_bench.py --logit [...]      # with an N(0, 1) [E, H] edge_logit that requires a gradient, on both sides
    python tools/additive_attention_bench.py --dropout [...]    # additive_attention_dropout at p = 0.5: three contenders alternated --
                                                                # fused with dropout, fused without, the composition with the mask as a
                                                                # tensor -> profiles/additive_attention_dropout_bench.jsonl
    python tools/additive_attention_bench.py --tables-bf16 [--logit] [...]    # additive_attention_bf16: the fp32 fused forward against
                                                                # the bf16 one -> profiles/additive_attention_bf16_bench.jsonl

The measuring step runs in a child process under `timeout -k 10 <--limit seconds>`; this process never opens the GPU.  Both contenders
run in that one process, alternated round by round, timed as tools/dot_attention_bench.py times its own (`alternate`, imported): a
round times `steps` calls of one contender, each between two HIP events, then the same of the other.  Reported per contender: the
median over all rounds x steps timed calls (at least 50) and the spread of the rounds' medians: a difference below that spread is
not a difference.  The composition is the baseline: it runs kernels and torch ops that exist without K20, on the same build.

Before timing, both contenders' outputs are priced on the same seeded inputs by the rule of tests/parity.py against an fp64
computation on the CPU, on a sample of rows (the row of most entries among them).  Algorithmic bytes are computed from the shapes (E
entries, N rows, M columns, H heads, R = H F floats per row), `*_bytes` below; `*_roof_ms` is their time at 8 TB/s, and
`*_roof_fraction` that over the measured time: the whole op's share of the HBM roof on the byte model, not a kernel's.  Recorded, not
gated.  One JSON object per shape, appended.

--tables-bf16 measures the inference forward on a bfloat16 v table (forward only), as tools/dot_attention_bench.py --kv-bf16 does for
K19: in the one child process it alternates the fused forward on a float32 table with the fused forward on a bfloat16 table.  Both are
fed the same values -- N(0, 1) draws rounded to bfloat16, and those widened to float32 -- so the two outputs are compared with
torch.equal here (asserted); the bfloat16 one is priced on the sampled rows as above.  Recorded per shape: both medians with their
spreads, their ratio, and the byte model's ratio beside it.  The yardstick is the float32 forward of the same run."""
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
SECTOR = 32          # bytes: the granularity at which the H floats of s_src[j] are counted


def sectors(nbytes):
    return -(-nbytes // SECTOR) * SECTOR


def fused_forward_bytes(E, N, M, H, F, logit=False, perm=False):
    """Per entry: the column index, the H floats of s_src[j] at sector granularity and the v row; with a logit its H floats and, where
    the pattern carries a permutation, the entry index.  Per row: s_dst read, out, m and Z written, the row pointer."""
    R = H * F
    entry = 4 + sectors(4 * H) + 4 * R + ((4 * H + (4 if perm else 0)) if logit else 0)
    return E * entry + N * (4 * H + 4 * R + 2 * 4 * H + 4)


def fused_backward_bytes(E, N, M, H, F, logit=False, perm=False):
    """Row pass: the forward's reads per entry, P and S written; s_dst, G, out, m, Z read and ds_dst written per row.  Column side, two
    SpMMs on the transposed pattern: P with the row index, the permutation entry and the G row per entry, dv per column; S with the
    same two indices and the H ones of a row at sector granularity per entry, ds_src per column."""
    R = H * F
    entry = 4 + sectors(4 * H) + 4 * R + 2 * 4 * H + ((4 * H + (4 if perm else 0)) if logit else 0)
    rows = E * entry + N * (4 * H + 2 * 4 * R + 2 * 4 * H + 4 * H + 4)
    cols = E * (4 * H + 8 + 4 * R) + M * (4 * R + 4) + E * (4 * H + 8 + sectors(4 * H)) + M * (4 * H + 4)
    return rows + cols


def bf16_forward_bytes(E, N, M, H, F, logit=False, perm=False):
    """A bfloat16 v table (inference): the v row at 2 bytes a value; m and Z are not written; everything else as fused_forward_bytes."""
    R = H * F
    entry = 4 + sectors(4 * H) + 2 * R + ((4 * H + (4 if perm else 0)) if logit else 0)
    return E * entry + N * (4 * H + 4 * R + 4)


def composed_forward_bytes(E, N, M, H, F, logit=False):
    """The two gathers (an index and H floats at sector granularity read, [E, H] written, each), their sum and leaky_relu (two reads and
    a write, one read and a write; with a logit one more sum).  K18: the logits read by the row pass and again by the entry pass with
    the (row, col) pair, alpha written; m and Z per row.  SpMM: alpha, the column index and the v row per entry, out per row."""
    R = H * F
    gathers = 2 * E * (8 + sectors(4 * H) + 4 * H) + E * (3 * 4 * H) + E * (2 * 4 * H) + (E * (3 * 4 * H) if logit else 0)
    softmax = E * (3 * 4 * H + 8) + N * (2 * 2 * 4 * H + 4)
    spmm = E * (4 * H + 4 + 4 * R) + N * (4 * R + 4)
    return gathers + softmax + spmm


def composed_backward_bytes(E, N, M, H, F, logit=False):
    """SpMM's backward: an SDDMM over G and v (dalpha written) and the transposed SpMM of alpha and G (dv).  K18's backward: alpha and
    dalpha read by both passes, dlogits written, c per row.  leaky_relu's backward (two reads and a write), and the two gathers'
    backwards: [E, H] and an index read and added into [N, H] and [M, H] tables that were zeroed first."""
    R = H * F
    spmm_b = E * (2 * 4 * R + 8 + 4 * H) + E * (4 * H + 8 + 4 * R) + M * (4 * R + 4)
    softmax_b = E * (5 * 4 * H + 8) + N * (2 * 4 * H + 4)
    rest = E * (3 * 4 * H) + 2 * E * (4 * H + 8 + 2 * sectors(4 * H)) + (N + M) * 4 * H
    return spmm_b + softmax_b + rest


def sampled_reference(rp, col, rows, s_dst, s_src, v, slope, dtype, u=None, mask=None):
    """out of `rows` by torch on the CPU in `dtype`: the softmax over each row's entries of leaky_relu((s_dst_i + s_src_j) + u) (u [E, H],
    at the CSR position), times mask (the dropout's, [E, H] at the CSR position, after the softmax), times v_j."""
    import torch
    deg = rp[rows + 1] - rp[rows]
    idx = torch.cat([torch.arange(int(rp[r]), int(rp[r + 1])) for r in rows.tolist()])
    sub = torch.repeat_interleave(torch.arange(rows.numel()), deg)
    cols, inv = torch.unique(col[idx], return_inverse=True)
    sd, ss, vs = s_dst[rows].cpu().to(dtype), s_src[cols].cpu().to(dtype), v[cols].cpu().to(dtype)
    z = sd[sub] + ss[inv]
    if u is not None:
        z = z + u[idx.to(u.device)].cpu().to(dtype)
    l = torch.nn.functional.leaky_relu(z, slope)
    m = torch.full(sd.shape, -float("inf"), dtype=dtype).scatter_reduce(0, sub[:, None].expand(-1, l.shape[1]), l, "amax")
    p = torch.exp(l - m[sub])
    alpha = p / torch.zeros_like(m).index_add(0, sub, p)[sub]
    if mask is not None:
        alpha = alpha * mask[idx.to(mask.device)].cpu().to(dtype)
    return torch.zeros(rows.numel(), v.shape[1], v.shape[2], dtype=dtype).index_add(0, sub, alpha[:, :, None] * vs[inv])


def measure(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("additive_attention_bench: needs a GPU (a time taken anywhere else says nothing)")
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
        g = torch.Generator(device=dev).manual_seed(2)
        s_dst, s_src = (torch.randn(N, H, generator=g, device=dev) for _ in range(2))
        v, G = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(2))
        leaves = (s_dst, s_src, v) + ((torch.randn(E, H, generator=g, device=dev),) if args.logit else ())

        def fused(sd, ss, v_, u=None):
            return pg.additive_attention(pattern, sd, ss, v_, slope, u)

        def composed(sd, ss, v_, u=None):
            z = sd[row_d] + ss[col_d]
            if u is not None:
                z = z + u
            return pg.spmm(pattern, pg.edge_softmax(pattern, torch.nn.functional.leaky_relu(z, slope)), v_)

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

        if args.tables_bf16:
            measure_bf16(args, torch, pg, parity, alternate, dev, pattern, shape, H, F, slope, leaves, rp_t, col_t, deg, rows, perm)
            del s_dst, s_src, v, G, leaves
            torch.cuda.empty_cache()
            continue
        if args.dropout:
            measure_dropout(args, torch, pg, parity, alternate, dev, pattern, shape, H, F, slope, leaves, G, row_d, col_d, rp_t, col_t, deg,
                            rows, perm, forward_of, both_of, fused)
            del s_dst, s_src, v, G, leaves
            torch.cuda.empty_cache()
            continue
        # the same seeded inputs, both contenders priced on the sampled rows
        out_f, out_c = forward_of(fused)(), forward_of(composed)()
        ref64 = sampled_reference(rp_t, col_t, rows, *leaves[:3], slope, torch.float64, *leaves[3:])
        ref32 = sampled_reference(rp_t, col_t, rows, *leaves[:3], slope, torch.float32, *leaves[3:])
        err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} fused out", ref32)
        err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} composed out", ref32)
        res = {"bench": "additive_attention" + (" --logit" if args.logit else ""), "device": torch.cuda.get_device_name(0),
               "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
               "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
               "longest_checked_row": int(deg[rows].max()), "out_err_fused": err_f, "out_err_composed": err_c,
               "out_err_fp32_reference": parity.err(ref32, ref64), "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
               "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, args.logit, perm),
               "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F, args.logit),
               "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F, args.logit, perm),
               "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F, args.logit)}
        del out_f, out_c
        legs = [("forward", alternate({"fused": forward_of(fused), "composed": forward_of(composed)}, args.rounds, args.steps, args.warmup))]
        if not args.forward_only:
            legs.append(("forward_backward", alternate({"fused": both_of(fused), "composed": both_of(composed)}, args.rounds, args.steps,
                                                       args.warmup)))
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
        del s_dst, s_src, v, G, leaves
        torch.cuda.empty_cache()


def measure_bf16(args, torch, pg, parity, alternate, dev, pattern, shape, H, F, slope, leaves, rp_t, col_t, deg, rows, perm):
    """--tables-bf16, one shape: the fused forward on a float32 v table against additive_attention_bf16 on the bfloat16 table of the
    same values (with --logit: both with the [E, H] edge_logit); one JSON object."""
    N, E, R = pattern.n_rows, pattern.nnz, H * F
    s_dst, s_src, v = leaves[:3]
    u = leaves[3] if args.logit else None
    v16 = v.bfloat16()
    vw = v16.float()                                                # the same values, widened: what the float32 contender is fed

    def run_fp32():
        with torch.no_grad():
            return pg.additive_attention(pattern, s_dst, s_src, vw, slope, u)

    def run_bf16():
        with torch.no_grad():
            return pg.additive_attention_bf16(pattern, s_dst, s_src, v16, slope, u)

    out_w, out_h = run_fp32(), run_bf16()
    equal = bool(torch.equal(out_w, out_h))
    assert equal, f"{shape}: the bf16 forward differs from the float32 forward on the widened table"
    ref64 = sampled_reference(rp_t, col_t, rows, s_dst, s_src, vw, slope, torch.float64, u)
    ref32 = sampled_reference(rp_t, col_t, rows, s_dst, s_src, vw, slope, torch.float32, u)
    err_h = parity.close_fwd(out_h[rows.to(dev)], ref64, f"{shape} fused, bf16 table: out", ref32)
    res = {"bench": "additive_attention --tables-bf16" + (" --logit" if args.logit else ""), "device": torch.cuda.get_device_name(0),
           "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
           "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
           "longest_checked_row": int(deg[rows].max()), "out_bf16_equals_out_fp32_on_widened_tables": equal,
           "out_err_fused_bf16": err_h, "out_err_fp32_reference": parity.err(ref32, ref64),
           "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, args.logit, perm),
           "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F, args.logit, perm)}
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
    print(f"{shape}: the bf16 table takes {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
          f"{res['byte_model_ratio']:.3f}; outputs bit-equal", flush=True)


def measure_dropout(args, torch, pg, parity, alternate, dev, pattern, shape, H, F, slope, leaves, G, row_d, col_d, rp_t, col_t, deg, rows,
                    perm, forward_of, both_of, fused):
    """--dropout, one shape: fused with dropout, fused without, the composition with the mask as a tensor; one JSON object.  The fused
    op's algorithmic bytes are those without dropout -- the mask is drawn in registers -- but for the permutation entry the forward now
    reads where the pattern carries one (4 bytes an entry; this graph's pattern carries none)."""
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=dev)
    N, E = pattern.n_rows, pattern.nnz

    def fused_dropout(sd, ss, v_, u=None):
        return pg.additive_attention_dropout(pattern, sd, ss, v_, p, slope, u, seed=seed)

    def composed_dropout(sd, ss, v_, u=None):
        z = sd[row_d] + ss[col_d]
        if u is not None:
            z = z + u
        alpha = pg.edge_softmax(pattern, torch.nn.functional.leaky_relu(z, slope))
        return pg.spmm(pattern, alpha * pg.attention_dropout_mask(pattern, H, p, seed), v_)

    contenders = {"fused_dropout": fused_dropout, "composed_dropout": composed_dropout, "fused": fused}
    out_f, out_c = forward_of(fused_dropout)(), forward_of(composed_dropout)()
    mask = pg.attention_dropout_mask(pattern, H, p, seed)
    ref64 = sampled_reference(rp_t, col_t, rows, *leaves[:3], slope, torch.float64, *leaves[3:4], mask=mask)
    ref32 = sampled_reference(rp_t, col_t, rows, *leaves[:3], slope, torch.float32, *leaves[3:4], mask=mask)
    err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} fused, dropout: out", ref32)
    err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} composed, dropout: out", ref32)
    res = {"bench": "additive_attention --dropout" + (" --logit" if args.logit else ""), "device": torch.cuda.get_device_name(0), "p": p,
           "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "negative_slope": slope,
           "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
           "longest_checked_row": int(deg[rows].max()), "kept_fraction": float((mask != 0).float().mean()),
           "out_err_fused_dropout": err_f, "out_err_composed_dropout": err_c, "out_err_fp32_reference": parity.err(ref32, ref64),
           "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F, args.logit, perm),
           "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F, args.logit, perm),
           "fused_dropout_extra_forward_bytes": 0 if args.logit or not perm else 4 * E, "mask_tensor_bytes": E * H * 4}
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
    print(f"{shape}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged bytes; "
          f"the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x16,8x64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed calls per round and contender")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true", help="skip the forward + backward leg")
    ap.add_argument("--logit", action="store_true", help="both contenders with an [E, H] edge_logit that requires a gradient")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--draws", type=int, default=5_000_000)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--dropout", action="store_true", help="additive_attention_dropout at p = 0.5 against the op without dropout and "
                    "the composition with the mask as a tensor")
    ap.add_argument("--tables-bf16", action="store_true", help="additive_attention_bf16: the fused forward on a float32 v table against "
                    "the fused forward on the bfloat16 table of the same values (forward only; goes with --logit)")
    ap.add_argument("--out", default=None, help="profiles/additive_attention_bench.jsonl, or ..._dropout_bench.jsonl under --dropout, "
                    "..._bf16_bench.jsonl under --tables-bf16")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.tables_bf16 and args.dropout:
        ap.error("--tables-bf16 and --dropout are two measurements: there is no op with both")
    if args.out is None:
        name = "additive_attention_bf16_bench.jsonl" if args.tables_bf16 else "additive_attention_dropout_bench.jsonl" if args.dropout else \
            "additive_attention_bench.jsonl"
        args.out = os.path.join(ROOT, "profiles", name)
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
