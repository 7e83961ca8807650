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

How it measures is tools/pattern_bench.py's and described there: the child process under `timeout -k 10 <--limit seconds>`, the
contenders alternated round by round in that one process (at least 50 timed calls each), the median and the spread, the pricing of
the outputs on a sample of rows, the roof fields.  The composition is the baseline: it runs kernels and torch ops that exist without
K20, on the same build.  Algorithmic bytes are computed from the shapes (E entries, N rows, M columns, H heads, R = H F floats per
row), `*_bytes` below.  Recorded, not gated.  One JSON object per shape, appended.

--tables-bf16 measures the inference forward on a bfloat16 v table (forward only), as tools/dot_attention_bench.py --kv-bf16 does for
K19: in the one child process it alternates the fused forward on a float32 table with the fused forward on a bfloat16 table.  Both are
fed the same values -- N(0, 1) draws rounded to bfloat16, and those widened to float32 -- so the two outputs are compared with
torch.equal here (asserted); the bfloat16 one is priced on the sampled rows as above.  Recorded per shape: both medians with their
spreads, their ratio, and the byte model's ratio beside it.  The yardstick is the float32 forward of the same run."""
import argparse
import os

import pattern_bench as pb
from pattern_bench import sectors          # the H floats of s_src[j] are counted at 32-byte granularity

SLOPE = 0.2


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


def record_bytes(mode, E, N, H, F, logit=False, perm=False):
    """The byte-model fields of a record of `mode` (None, "dropout" or "tables_bf16"), in the record's order; the bench's pattern is
    square, M = N.  Under dropout the fused op's bytes are those without it -- the mask is drawn in registers -- but for the
    permutation entry the forward now reads where the pattern carries one and no logit made it read it already."""
    fused_f = fused_forward_bytes(E, N, N, H, F, logit, perm)
    if mode == "tables_bf16":
        return {"fused_forward_bytes": fused_f, "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F, logit, perm)}
    fused_b = fused_backward_bytes(E, N, N, H, F, logit, perm)
    if mode == "dropout":
        return {"fused_forward_bytes": fused_f, "fused_backward_bytes": fused_b,
                "fused_dropout_extra_forward_bytes": 0 if logit or not perm else 4 * E, "mask_tensor_bytes": E * H * 4}
    return {"fused_forward_bytes": fused_f, "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F, logit),
            "fused_backward_bytes": fused_b, "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F, logit)}


def entry_terms(s_dst, s_src, v, u=None):
    """The family's part of pattern_bench.sampled_reference: the score leaky_relu((s_dst_i + s_src_j) + u) (u [E, H], at the CSR
    position) and the values v_j."""
    import torch

    def terms(dtype, part, idx, sub, cols, inv):
        z = pb.taken(s_dst, part, dtype)[sub] + pb.taken(s_src, cols, dtype)[inv]
        if u is not None:
            z = z + pb.taken(u, idx, dtype)
        return torch.nn.functional.leaky_relu(z, SLOPE), pb.taken(v, cols, dtype)[inv]
    return terms


def inputs(args, w, H, F):
    """One shape's seeded tensors and the two plain contenders -> (leaves, G, fused, composed); leaves: s_dst, s_src, v and, under
    --logit, the [E, H] edge_logit."""
    import torch
    import pygat_amd as pg
    g = w.generator()
    s_dst, s_src = (torch.randn(w.N, H, generator=g, device=w.dev) for _ in range(2))
    v, G = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(2))
    leaves = (s_dst, s_src, v) + ((torch.randn(w.E, H, generator=g, device=w.dev),) if args.logit else ())
    row_d, col_d = w.row_d, w.col_d

    def fused(sd, ss, v_, u=None):
        return pg.additive_attention(w.pattern, sd, ss, v_, SLOPE, u)

    def composed(sd, ss, v_, u=None):
        z = sd[row_d] + ss[col_d]
        if u is not None:
            z = z + u
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, torch.nn.functional.leaky_relu(z, SLOPE)), v_)

    return leaves, G, fused, composed


def measure_plain(args, w, shape, H, F):
    """No mode flag: the fused op against the composition (under --logit both with the edge_logit); one JSON object."""
    import torch
    leaves, G, fused, composed = inputs(args, w, H, F)
    # the same seeded inputs, both contenders priced on the sampled rows
    out_f, out_c = pb.forward_of(fused, leaves)(), pb.forward_of(composed, leaves)()
    err_of, ref_err = pb.pricer(w, entry_terms(*leaves))
    res = pb.base_record("additive_attention" + (" --logit" if args.logit else ""), args, w, H, F, negative_slope=SLOPE)
    res.update({"out_err_fused": err_of(out_f, f"{shape} fused out"), "out_err_composed": err_of(out_c, f"{shape} composed out"),
                "out_err_fp32_reference": ref_err, "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
                **record_bytes(None, w.E, w.N, H, F, args.logit, w.perm)})
    del out_f, out_c
    legs = pb.run_legs(args, {"fused": (fused, leaves), "composed": (composed, leaves)}, G)
    pb.add_legs(res, legs, speedup=("composed", "fused"), roof="fused")
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)


def measure_bf16(args, w, shape, H, F):
    """--tables-bf16: the fused forward on a float32 v table against additive_attention_bf16 on the bfloat16 table of the same values
    (with --logit: both with the [E, H] edge_logit); one JSON object."""
    import torch
    import pygat_amd as pg
    leaves, G = inputs(args, w, H, F)[:2]      # (G is drawn and held though nothing reads it: peak_device_bytes has always counted it)
    s_dst, s_src, v = leaves[:3]
    u = leaves[3] if args.logit else None
    v16 = v.bfloat16()
    vw = v16.float()                                                # the same values, widened: what the float32 contender is fed

    def run_fp32():
        with torch.no_grad():
            return pg.additive_attention(w.pattern, s_dst, s_src, vw, SLOPE, u)

    def run_bf16():
        with torch.no_grad():
            return pg.additive_attention_bf16(w.pattern, s_dst, s_src, v16, SLOPE, u)

    out_w, out_h = run_fp32(), run_bf16()
    equal = bool(torch.equal(out_w, out_h))
    assert equal, f"{shape}: the bf16 forward differs from the float32 forward on the widened table"
    err_of, ref_err = pb.pricer(w, entry_terms(s_dst, s_src, vw, u))
    res = pb.base_record("additive_attention --tables-bf16" + (" --logit" if args.logit else ""), args, w, H, F, negative_slope=SLOPE)
    res.update({"out_bf16_equals_out_fp32_on_widened_tables": equal, "out_err_fused_bf16": err_of(out_h, f"{shape} fused, bf16 table: out"),
                "out_err_fp32_reference": ref_err, **record_bytes("tables_bf16", w.E, w.N, H, F, args.logit, w.perm)})
    res["byte_model_ratio"] = res["fused_bf16_forward_bytes"] / res["fused_forward_bytes"]
    del out_w, out_h
    r = pb.alternate({"fused_fp32": run_fp32, "fused_bf16": run_bf16}, args.rounds, args.steps, args.warmup)
    for name, model in (("fused_fp32", "fused_forward_bytes"), ("fused_bf16", "fused_bf16_forward_bytes")):
        res[f"{name}_forward_ms"], res[f"{name}_forward_spread_ms"] = r[name]
        res[f"{name}_forward_roof_fraction"] = 1e3 * res[model] / pb.HBM_BYTES_PER_S / res[f"{name}_forward_ms"]
    pb.add_bf16_ratio(res)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)
    print(f"{shape}: the bf16 table takes {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
          f"{res['byte_model_ratio']:.3f}; outputs bit-equal", flush=True)


def measure_dropout(args, w, shape, H, F):
    """--dropout: fused with dropout, fused without, the composition with the mask as a tensor; one JSON object."""
    import torch
    import pygat_amd as pg
    leaves, G, fused, _ = inputs(args, w, H, F)
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=w.dev)
    row_d, col_d = w.row_d, w.col_d

    def fused_dropout(sd, ss, v_, u=None):
        return pg.additive_attention_dropout(w.pattern, sd, ss, v_, p, SLOPE, u, seed=seed)

    def composed_dropout(sd, ss, v_, u=None):
        z = sd[row_d] + ss[col_d]
        if u is not None:
            z = z + u
        alpha = pg.edge_softmax(w.pattern, torch.nn.functional.leaky_relu(z, SLOPE))
        return pg.spmm(w.pattern, alpha * pg.attention_dropout_mask(w.pattern, H, p, seed), v_)

    out_f, out_c = pb.forward_of(fused_dropout, leaves)(), pb.forward_of(composed_dropout, leaves)()
    mask = pg.attention_dropout_mask(w.pattern, H, p, seed)
    err_of, ref_err = pb.pricer(w, entry_terms(*leaves), mask)
    res = pb.base_record("additive_attention --dropout" + (" --logit" if args.logit else ""), args, w, H, F, p=p, negative_slope=SLOPE)
    res.update({"kept_fraction": float((mask != 0).float().mean()), "out_err_fused_dropout": err_of(out_f, f"{shape} fused, dropout: out"),
                "out_err_composed_dropout": err_of(out_c, f"{shape} composed, dropout: out"), "out_err_fp32_reference": ref_err,
                **record_bytes("dropout", w.E, w.N, H, F, args.logit, w.perm)})
    del out_f, out_c, mask

    def increment(what):
        res[f"dropout_{what}_measured_increment"] = res[f"fused_dropout_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
    legs = pb.run_legs(args, {"fused_dropout": (fused_dropout, leaves), "composed_dropout": (composed_dropout, leaves),
                              "fused": (fused, leaves)}, G)
    pb.add_legs(res, legs, speedup=("composed_dropout", "fused_dropout"), each=increment)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)
    print(f"{shape}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged bytes; "
          f"the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)


def measure(args):
    w = pb.Workload(args, "additive_attention_bench", row_d=True, col_d=True)
    one_shape = measure_bf16 if args.tables_bf16 else measure_dropout if args.dropout else measure_plain
    for shape, H, F in pb.shapes(args):
        one_shape(args, w, shape, H, F)


def parse(argv=None):
    """-> (the parser, the arguments with --out and what else depends on the mode filled in)."""
    ap = argparse.ArgumentParser()
    pb.common_arguments(ap, 420, "profiles/additive_attention_bench.jsonl, or ..._dropout_bench.jsonl under --dropout, "
                        "..._bf16_bench.jsonl under --tables-bf16")
    ap.add_argument("--logit", action="store_true", help="both contenders with an [E, H] edge_logit that requires a gradient")
    ap.add_argument("--dropout", action="store_true", help="additive_attention_dropout at p = 0.5 against the op without dropout and "
                    "the composition with the mask as a tensor")
    ap.add_argument("--tables-bf16", action="store_true", help="additive_attention_bf16: the fused forward on a float32 v table against "
                    "the fused forward on the bfloat16 table of the same values (forward only; goes with --logit)")
    args = ap.parse_args(argv)
    if args.tables_bf16 and args.dropout:
        ap.error("--tables-bf16 and --dropout are two measurements: there is no op with both")
    if args.out is None:
        name = "additive_attention_bf16_bench.jsonl" if args.tables_bf16 else "additive_attention_dropout_bench.jsonl" if args.dropout else \
            "additive_attention_bench.jsonl"
        args.out = os.path.join(pb.ROOT, "profiles", name)
    return ap, args


def main():
    args = parse()[1]
    if args.child:
        return measure(args)
    pb.run_in_child(__file__, args.limit)


if __name__ == "__main__":
    main()
