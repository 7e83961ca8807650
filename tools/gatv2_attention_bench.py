#!/usr/bin/env python3
"""What pygat_amd.gatv2_attention costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py)
against the same result from the parts it fuses -- two torch gathers and their sum, leaky_relu, the product with a and its sum over the
features, edge_softmax (K18) and spmm (pygat_spmm_forward) -- at H x F = 8x16 and 8x64, N(0, 1) tensors, slope 0.2, with v shared
(v=None: v is x_src) and with a v table of its own, the forward alone and forward + backward:

    python tools/gatv2_attention_bench.py [--shapes 8x16,8x64] [--values shared,separate] [--rounds 5] [--steps 10] [--warmup 10]
                                          [--dropout | --edge] [--out profiles/gatv2_attention_bench.jsonl]
    python tools/gatv2_attention_bench.py --tables-bf16 [--edge] [...]      # gatv2_attention_bf16 (gatv2_attention_edge_bf16): the fp32
                                          # fused forward against the bf16 one -> profiles/gatv2_attention_bf16_bench.jsonl (..._edge_bf16_...)

How it measures is tools/pattern_bench.py's and described there: the child process under `timeout -k 10 <--limit seconds>`, the
contenders alternated round by round in that one process (at least 50 timed calls each), the median and the spread, the pricing of
the outputs on a sample of rows, the roof fields.  The composition is the baseline: it runs kernels and torch ops that exist without
K21, on the same build.  Algorithmic bytes are computed from the shapes (E entries, N rows, M columns, H heads, R = H F floats per
row), `*_bytes` below.  Recorded, not gated.  One JSON object per (shape, value table), appended.

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
import os

import pattern_bench as pb
from pattern_bench import sectors          # the H floats of S[c] are counted at 32-byte granularity

SLOPE = 0.2


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


def edge_bytes(E, H, F, perm=False):
    """What e adds to the byte models, R = H F: the fused op reads the entry's e row once in each of its three passes (and the entry
    index in the forward where the pattern carries a permutation) and writes de once; the composition has one more elementwise add in
    its forward (two [E, R] reads and a write) and none in its backward: the add hands its incoming gradient on as de."""
    R = H * F
    return {"fused_forward": E * 4 * R + (4 * E if perm else 0), "fused_backward": 3 * E * 4 * R, "composed_forward": 3 * E * 4 * R,
            "composed_backward": 0}


def record_bytes(mode, E, N, H, F, shared, edge=False, perm=False):
    """The byte-model fields of a record of `mode` (None, "dropout" or "tables_bf16"; edge: with --edge), in the record's order; the
    bench's pattern is square, M = N.  Under dropout the fused op's bytes are those without it -- the mask is drawn in registers --
    but for the permutation entry the forward now reads where the pattern carries one."""
    extra = edge_bytes(E, H, F, perm) if edge else dict.fromkeys(("fused_forward", "fused_backward", "composed_forward", "composed_backward"), 0)
    fused_f = fused_forward_bytes(E, N, N, H, F, shared) + extra["fused_forward"]
    if mode == "tables_bf16":
        return {"fused_forward_bytes": fused_f, "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F, shared, edge, perm)}
    fused_b = fused_backward_bytes(E, N, N, H, F, shared, perm) + extra["fused_backward"]
    if mode == "dropout":
        return {"fused_forward_bytes": fused_f, "fused_backward_bytes": fused_b, "fused_dropout_extra_forward_bytes": 4 * E if perm else 0,
                "mask_tensor_bytes": E * H * 4}
    composed_f = composed_forward_bytes(E, N, N, H, F) + extra["composed_forward"]
    composed_b = composed_backward_bytes(E, N, N, H, F) + extra["composed_backward"]
    if edge:
        return {"e_tensor_bytes": E * 4 * H * F, "fused_forward_bytes": fused_f, "fused_backward_bytes": fused_b,
                "composed_forward_bytes": composed_f, "composed_backward_bytes": composed_b}
    return {"fused_forward_bytes": fused_f, "composed_forward_bytes": composed_f, "fused_backward_bytes": fused_b,
            "composed_backward_bytes": composed_b}


def entry_terms(x_dst, x_src, a, v, e=None):
    """The family's part of pattern_bench.sampled_reference: the score a . leaky_relu(x_dst_i + x_src_j) and the values v_j; e: the
    edge rows of --edge, [E, H, F] at the CSR position, added behind x_dst_i + x_src_j."""
    import torch

    def terms(dtype, part, idx, sub, cols, inv):
        t = pb.taken(x_dst, part, dtype)[sub] + pb.taken(x_src, cols, dtype)[inv]
        if e is not None:
            t = t + pb.taken(e, idx, dtype)
        return (a.cpu().to(dtype) * torch.nn.functional.leaky_relu(t, SLOPE)).sum(-1), pb.taken(v, cols, dtype)[inv]
    return terms


def inputs(w, H, F, shared):
    """One shape's seeded tensors for one kind of v and the two plain contenders -> (leaves, G, fused, composed); leaves: x_dst,
    x_src, a and, where v is not shared, v."""
    import torch
    import pygat_amd as pg
    g = w.generator()
    x_dst, x_src = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(2))
    a = torch.randn(H, F, generator=g, device=w.dev)
    G = torch.randn(w.N, H, F, generator=g, device=w.dev)
    leaves = (x_dst, x_src, a) + (() if shared else (torch.randn(w.N, H, F, generator=g, device=w.dev),))
    row_d, col_d = w.row_d, w.col_d

    def fused(xd, xs, a_, v_=None):
        return pg.gatv2_attention(w.pattern, xd, xs, a_, v_, SLOPE)

    def composed(xd, xs, a_, v_=None):
        e = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d], SLOPE)).sum(-1)
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, e), xs if v_ is None else v_)

    return leaves, G, fused, composed


def measure_plain(args, w, shape, values, H, F):
    """No mode flag, one shape and one kind of v: the fused op against the composition; one JSON object."""
    import torch
    shared = values == "shared"
    leaves, G, fused, composed = inputs(w, H, F, shared)
    # the same seeded inputs, both contenders priced on the sampled rows
    out_f, out_c = pb.forward_of(fused, leaves)(), pb.forward_of(composed, leaves)()
    err_of, ref_err = pb.pricer(w, entry_terms(*leaves[:3], leaves[1] if shared else leaves[3]))
    res = pb.base_record("gatv2_attention", args, w, H, F, values=values, negative_slope=SLOPE)
    res.update({"out_err_fused": err_of(out_f, f"{shape} {values} fused out"), "out_err_composed": err_of(out_c, f"{shape} {values} composed out"),
                "out_err_fp32_reference": ref_err, "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
                **record_bytes(None, w.E, w.N, H, F, shared, perm=w.perm)})
    del out_f, out_c
    legs = pb.run_legs(args, {"fused": (fused, leaves), "composed": (composed, leaves)}, G)
    pb.add_legs(res, legs, speedup=("composed", "fused"), roof="fused")
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)


def measure_bf16(args, w, shape, values, H, F):
    """--tables-bf16, one shape and one kind of v: the fused forward on float32 tables against gatv2_attention_bf16 on the bfloat16
    tables of the same values; with --edge gatv2_attention_edge against gatv2_attention_edge_bf16, e [E, H, F] among the tables; one
    JSON object."""
    import torch
    import pygat_amd as pg
    shared = values == "shared"
    leaves, G = inputs(w, H, F, shared)[:2]      # (G is drawn and held though nothing reads it: peak_device_bytes has always counted it)
    x_dst, a = leaves[0], leaves[2]
    x16 = leaves[1].bfloat16()
    v16 = None if shared else leaves[3].bfloat16()
    e16 = torch.randn(w.E, H, F, generator=torch.Generator(device=w.dev).manual_seed(5), device=w.dev).bfloat16() if args.edge else None
    xw, vw, ew = (None if t is None else t.float() for t in (x16, v16, e16))      # the same values, widened: the float32 contender's

    def run_fp32():
        with torch.no_grad():
            if args.edge:
                return pg.gatv2_attention_edge(w.pattern, x_dst, xw, a, ew, vw, SLOPE)
            return pg.gatv2_attention(w.pattern, x_dst, xw, a, vw, SLOPE)

    def run_bf16():
        with torch.no_grad():
            if args.edge:
                return pg.gatv2_attention_edge_bf16(w.pattern, x_dst, x16, a, e16, v16, SLOPE)
            return pg.gatv2_attention_bf16(w.pattern, x_dst, x16, a, v16, SLOPE)

    out_w, out_h = run_fp32(), run_bf16()
    equal = bool(torch.equal(out_w, out_h))
    assert equal, f"{shape} {values}: the bf16 forward differs from the float32 forward on the widened tables"
    err_of, ref_err = pb.pricer(w, entry_terms(x_dst, xw, a, xw if shared else vw, ew))
    res = pb.base_record("gatv2_attention --tables-bf16" + (" --edge" if args.edge else ""), args, w, H, F, values=values, negative_slope=SLOPE)
    res.update({"out_bf16_equals_out_fp32_on_widened_tables": equal,
                "out_err_fused_bf16": err_of(out_h, f"{shape} {values} fused, bf16 tables: out"), "out_err_fp32_reference": ref_err,
                **record_bytes("tables_bf16", w.E, w.N, H, F, shared, args.edge, w.perm)})
    res["byte_model_ratio"] = res["fused_bf16_forward_bytes"] / res["fused_forward_bytes"]
    del out_w, out_h
    r = pb.alternate({"fused_fp32": run_fp32, "fused_bf16": run_bf16}, args.rounds, args.steps, args.warmup)
    for name, model in (("fused_fp32", "fused_forward_bytes"), ("fused_bf16", "fused_bf16_forward_bytes")):
        res[f"{name}_forward_ms"], res[f"{name}_forward_spread_ms"] = r[name]
        res[f"{name}_forward_roof_fraction"] = 1e3 * res[model] / pb.HBM_BYTES_PER_S / res[f"{name}_forward_ms"]
    pb.add_bf16_ratio(res)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)
    print(f"{shape} {values}: bf16 tables take {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
          f"{res['byte_model_ratio']:.3f}; outputs bit-equal", flush=True)


def measure_dropout(args, w, shape, values, H, F):
    """--dropout, one shape and one kind of v: fused with dropout, fused without, the composition with the mask as a tensor; one JSON
    object."""
    import torch
    import pygat_amd as pg
    shared = values == "shared"
    leaves, G, fused, _ = inputs(w, H, F, shared)
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=w.dev)
    row_d, col_d = w.row_d, w.col_d

    def fused_dropout(xd, xs, a_, v_=None):
        return pg.gatv2_attention_dropout(w.pattern, xd, xs, a_, p, v_, SLOPE, seed=seed)

    def composed_dropout(xd, xs, a_, v_=None):
        e = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d], SLOPE)).sum(-1)
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, e) * pg.attention_dropout_mask(w.pattern, H, p, seed), xs if v_ is None else v_)

    out_f, out_c = pb.forward_of(fused_dropout, leaves)(), pb.forward_of(composed_dropout, leaves)()
    mask = pg.attention_dropout_mask(w.pattern, H, p, seed)
    err_of, ref_err = pb.pricer(w, entry_terms(*leaves[:3], leaves[1] if shared else leaves[3]), mask)
    res = pb.base_record("gatv2_attention --dropout", args, w, H, F, values=values, p=p, negative_slope=SLOPE)
    res.update({"kept_fraction": float((mask != 0).float().mean()),
                "out_err_fused_dropout": err_of(out_f, f"{shape} {values} fused, dropout: out"),
                "out_err_composed_dropout": err_of(out_c, f"{shape} {values} composed, dropout: out"), "out_err_fp32_reference": ref_err,
                **record_bytes("dropout", w.E, w.N, H, F, shared, perm=w.perm)})
    del out_f, out_c, mask

    def increment(what):
        res[f"dropout_{what}_measured_increment"] = res[f"fused_dropout_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
    legs = pb.run_legs(args, {"fused_dropout": (fused_dropout, leaves), "composed_dropout": (composed_dropout, leaves),
                              "fused": (fused, leaves)}, G)
    pb.add_legs(res, legs, speedup=("composed_dropout", "fused_dropout"), each=increment)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)
    print(f"{shape} {values}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged "
          f"bytes; the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)


def measure_edge(args, w, shape, values, H, F):
    """--edge, one shape and one kind of v: gatv2_attention_edge against the composition with e inside leaky_relu; one JSON object.
    Every gradient is asked for, de among them."""
    import torch
    import pygat_amd as pg
    shared = values == "shared"
    leaves, G = inputs(w, H, F, shared)[:2]
    v = leaves[1] if shared else leaves[3]
    e = torch.randn(w.E, H, F, generator=torch.Generator(device=w.dev).manual_seed(5), device=w.dev)
    leaves = leaves + (e,)
    row_d, col_d = w.row_d, w.col_d

    def fused(xd, xs, a_, *rest):
        return pg.gatv2_attention_edge(w.pattern, xd, xs, a_, rest[-1], None if shared else rest[0], SLOPE)

    def composed(xd, xs, a_, *rest):
        s = (a_ * torch.nn.functional.leaky_relu(xd[row_d] + xs[col_d] + rest[-1], SLOPE)).sum(-1)
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, s), xs if shared else rest[0])

    # the composition keeps the two gathers, their sum, the sum with e, leaky_relu's output and the product for autograd, and its
    # backward holds as many gradients at its peak: some fourteen [E, R] tensors with the two copies of e
    free, _ = torch.cuda.mem_get_info(w.dev)
    need = 14 * w.E * 4 * H * F
    model = record_bytes(None, w.E, w.N, H, F, shared, True, w.perm)
    out_f = pb.forward_of(fused, leaves)()
    err_of, ref_err = pb.pricer(w, entry_terms(*leaves[:3], v, e))
    res = pb.base_record("gatv2_attention --edge", args, w, H, F, values=values, negative_slope=SLOPE)
    res.update({"e_tensor_bytes": model.pop("e_tensor_bytes"), "out_err_fused": err_of(out_f, f"{shape} {values} fused, edge: out"),
                "out_err_fp32_reference": ref_err, **model})
    contenders = {"fused": (fused, leaves)}
    if need <= free:
        out_c = pb.forward_of(composed, leaves)()
        res["out_err_composed"] = err_of(out_c, f"{shape} {values} composed, edge: out")
        res["out_max_abs_fused_minus_composed"] = float((out_f - out_c).abs().max())
        contenders["composed"] = (composed, leaves)
        del out_c
    else:
        res["composed"] = (f"not run: some {need / 2 ** 30:.0f} GiB for its [E, R] tensors against {free / 2 ** 30:.0f} GiB free; "
                           f"the fused op is recorded alone")
    del out_f

    def own(what):
        sides = ("forward", "backward") if what == "forward_backward" else ("forward",)
        res[f"{what}_bytes_ratio_model"] = sum(res[f"composed_{s}_bytes"] for s in sides) / sum(res[f"fused_{s}_bytes"] for s in sides)
        pb.roof_fields(res, what)
        if "composed" in contenders:
            res[f"{what}_speedup"] = res[f"composed_{what}_ms"] / res[f"fused_{what}_ms"]
    pb.add_legs(res, pb.run_legs(args, contenders, G), each=own)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)


def measure(args):
    import torch
    w = pb.Workload(args, "gatv2_attention_bench", row_d=True, col_d=True)
    one_case = measure_bf16 if args.tables_bf16 else measure_edge if args.edge else measure_dropout if args.dropout else measure_plain
    for shape, H, F in pb.shapes(args):
        for values in args.values.split(","):
            one_case(args, w, shape, values, H, F)
            torch.cuda.empty_cache()


def parse(argv=None):
    """-> (the parser, the arguments with --out and what else depends on the mode filled in)."""
    ap = argparse.ArgumentParser()
    pb.common_arguments(ap, 540, "profiles/gatv2_attention_bench.jsonl, or ..._dropout_bench.jsonl under --dropout, "
                        "..._edge_bench.jsonl under --edge, ..._bf16_bench.jsonl and ..._edge_bf16_bench.jsonl under --tables-bf16",
                        shapes=(None, "8x16,8x64; under --edge 8x16,8x32"))
    ap.add_argument("--values", default="shared,separate", help="shared: v=None, v is x_src; separate: a v table of its own")
    ap.add_argument("--dropout", action="store_true", help="gatv2_attention_dropout at p = 0.5 against the op without dropout and the "
                    "composition with the mask as a tensor")
    ap.add_argument("--edge", action="store_true", help="gatv2_attention_edge, e [E, H, F] inside the score, against the composition "
                    "with e added before leaky_relu")
    ap.add_argument("--tables-bf16", action="store_true", help="gatv2_attention_bf16 (with --edge: gatv2_attention_edge_bf16): the fused "
                    "forward on float32 tables against the fused forward on the bfloat16 tables of the same values (forward only)")
    args = ap.parse_args(argv)
    if args.edge and args.dropout:
        ap.error("--edge and --dropout are two measurements: there is no op with both")
    if args.shapes is None:
        args.shapes = "8x16,8x32" if args.edge else "8x16,8x64"
    if args.tables_bf16 and args.dropout:
        ap.error("--tables-bf16 and --dropout are two measurements: there is no op with both")
    if args.out is None:
        name = ("gatv2_attention_edge_bf16_bench.jsonl" if args.tables_bf16 and args.edge else "gatv2_attention_bf16_bench.jsonl" if
                args.tables_bf16 else "gatv2_attention_edge_bench.jsonl" if args.edge else "gatv2_attention_dropout_bench.jsonl" if
                args.dropout else "gatv2_attention_bench.jsonl")
        args.out = os.path.join(pb.ROOT, "profiles", name)
    return ap, args


def main():
    args = parse()[1]
    if args.child:
        return measure(args)
    pb.run_in_child(__file__, args.limit)


if __name__ == "__main__":
    main()
