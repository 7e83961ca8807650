#!/usr/bin/env python3
"""What pygat_amd.dot_attention costs at config 5 (R-MAT 2^20 nodes, 10 760 610 entries; pygat_amd.rmat, the graph of bench.py) against
the same result from the three ops it fuses -- edge_dot (pygat_spmm_grad_values), edge_softmax (K18) and spmm (pygat_spmm_forward) --
at H x F = 8x16 and 8x64, N(0, 1) tensors, scale 1 / sqrt(F), the forward alone and forward + backward:

    python tools/dot_attention_bench.py [--shapes 8x16,8x64] [--rounds 5] [--steps 10] [--warmup 10] [--out profiles/dot_attention_bench.jsonl]
    rocprofv3 --kernel-trace --stats -d DIR -o da -- python tools/dot_attention_bench.py --child --forward-only --shapes 8x64 --out DIR/run.jsonl
    python tools/dot_attention_bench.py --bias [...]       # the per-entry bias: three contenders -> profiles/dot_attention_bias_bench.jsonl
    python tools/dot_attention_bench.py --kv-bf16 [...]    # bf16 k and v tables: fp32 against bf16 forward -> profiles/dot_attention_bf16_bench.jsonl
    python tools/dot_attention_bench.py --dropout [...]    # seeded attention dropout: three contenders -> profiles/dot_attention_dropout_bench.jsonl
    python tools/dot_attention_bench.py --edge [...]       # per-entry key and value features: fused against the chain of parts -> profiles/dot_attention_edge_bench.jsonl

How it measures is tools/pattern_bench.py's and described there: the child process under `timeout -k 10 <--limit seconds>`, the
contenders alternated round by round in that one process (at least 50 timed calls each), the median and the spread, the pricing of
the outputs on a sample of rows.  The composition is given q already multiplied by the scale, so it runs the parent's kernels and
nothing else.  Algorithmic bytes are computed from the shapes (E entries, N rows, M columns, R = H F floats per row), `*_bytes` below.
Recorded, not gated.  One JSON object per shape, appended.

--bias measures dot_attention's per-entry bias instead: in the one child process it alternates the fused op with an N(0, 1) [E, H] bias
that requires a gradient, the composition spmm(edge_softmax(edge_dot(q, k) + bias), v) with the same bias, and the fused op without
a bias, prices the first two on the sampled rows against the fp64 computation with the bias on the scores, and prints the byte
model's expectation of what the bias adds to the fused forward (4 H bytes per entry, 4 more where the pattern carries a
permutation; the bench's pattern carries none) beside the measured increment.

--kv-bf16 measures the inference forward on bfloat16 k and v tables (forward only): in the one child process it alternates the fused
forward on float32 tables with the fused forward on bfloat16 tables.  Both are fed the same values -- N(0, 1) draws rounded to
bfloat16, and those widened to float32 -- so the two outputs are compared with torch.equal here; the bfloat16 one is priced on the
sampled rows as above.  Recorded per shape: both medians with their spreads, their ratio, and the byte model's ratio beside it
((4 R + 4) / (8 R + 4) per entry, and with the per-row traffic) -> profiles/dot_attention_bf16_bench.jsonl.

--dropout measures dot_attention_dropout at p = 0.5: in the one child process it alternates the fused op with dropout, the fused op
without it (dot_attention), and the composition spmm(edge_softmax(edge_dot(q, k)) * attention_dropout_mask(pattern, H, p, seed), v)
with the same seed, which writes and reads the mask as a [E, H] tensor.  The first and the last are priced on the sampled rows against
the fp64 computation under the mask attention_dropout_mask writes (that it is the mask of tests/philox_ref.py is the tests' business).
The fused op's bytes are those without dropout -- the decisions are drawn in registers -- so what the measured increment over the
fused op without dropout shows is arithmetic: ten Philox rounds per (entry, head chunk) and lane.

--edge measures dot_attention_edge: in the one child process it alternates the fused op, with an N(0, 1) e [E, H, F] that requires a
gradient, and the chain of parts a user writes without it -- edge_dot(q, k, scale) + scale * (q[row] * e).sum(-1), edge_softmax,
spmm(alpha, v) + zeros.index_add(0, row, alpha[..., None] * e) -- and prices both on the sampled rows against the fp64 computation
with e on both sides.  e alone is E H F 4 bytes (5.5 GB at 8x16, 22 GB at 8x64) and de the same again; the chain holds several
tensors of that size at once.  Free device memory is asked for first: a contender that does not fit is left out and the record
says so (`skipped`), a shape where not even the fused op fits is skipped whole; the tool does not fail over it."""
import argparse
import math
import os

import pattern_bench as pb


def fused_forward_bytes(E, N, M, H, F):
    """Per entry: the k and v rows and the column index.  Per row: q read, out, m and Z written, the row pointer."""
    R = H * F
    return E * (2 * R * 4 + 4) + N * (2 * R * 4 + 2 * H * 4 + 4)


def bf16_forward_bytes(E, N, M, H, F):
    """bfloat16 k and v tables (inference).  Per entry: the two rows at 2 bytes a value and the column index.  Per row: q read and out
    written in float32, the row pointer; m and Z are not written."""
    R = H * F
    return E * (2 * R * 2 + 4) + N * (2 * R * 4 + 4)


def composed_forward_bytes(E, N, M, H, F):
    """SDDMM: the q and k rows and the (row, col) pair per entry, u written.  K18: u read by the row pass and again by the entry pass
    with the pair, alpha written; m and Z per row.  SpMM: alpha, the column index and the v row per entry, out per row."""
    R = H * F
    sddmm = E * (2 * R * 4 + 8 + H * 4)
    softmax = E * (3 * H * 4 + 8) + N * (2 * 2 * H * 4 + 4)
    spmm = E * (H * 4 + 4 + R * 4) + N * (R * 4 + 4)
    return sddmm + softmax + spmm


def fused_backward_bytes(E, N, M, H, F):
    """Row pass: the k and v rows and the column index per entry, P and S written; q, G, out, m, Z read and dq written per row.
    Column side, two SpMMs on the transposed pattern: S (P) with the row index and the permutation entry and the q (G) row per entry,
    dk (dv) per column."""
    R = H * F
    rows = E * (2 * R * 4 + 4 + 2 * H * 4) + N * (4 * R * 4 + 2 * H * 4 + 4)
    cols = 2 * (E * (H * 4 + 8 + R * 4) + M * (R * 4 + 4))
    return rows + cols


def composed_backward_bytes(E, N, M, H, F):
    """SpMM's backward: an SDDMM over G and v (dalpha written) and the transposed SpMM of alpha and G (dv).  K18's backward: alpha and
    dalpha read by both passes, dlogits written, c per row.  edge_dot's backward: the SpMM of dlogits and k (dq) and the transposed SpMM of
    dlogits and q (dk)."""
    R = H * F
    spmm_b = E * (2 * R * 4 + 8 + H * 4) + E * (H * 4 + 8 + R * 4) + M * (R * 4 + 4)
    softmax_b = E * (5 * H * 4 + 8) + N * (2 * H * 4 + 4)
    dot_b = E * (H * 4 + 4 + R * 4) + N * (R * 4 + 4) + E * (H * 4 + 8 + R * 4) + M * (R * 4 + 4)
    return spmm_b + softmax_b + dot_b


def bias_forward_bytes(E, H, perm):
    """What a [E, H] bias adds to the fused forward: its values, and the entry index where the pattern carries a permutation."""
    return E * (4 * H + (4 if perm else 0))


def bias_backward_bytes(E, H, perm):
    """... and to the row pass of the backward: the values read, their gradient written (the entry index is read there anyway)."""
    return E * 8 * H


def edge_forward_bytes(E, H, F, perm):
    """What e adds to the fused forward: its row per entry, and the entry index where the pattern carries a permutation."""
    return E * (4 * H * F + (4 if perm else 0))


def edge_backward_bytes(E, H, F, perm):
    """... and to the row pass of the backward: the row read again and its gradient written (the entry index is read there anyway)."""
    return E * 8 * H * F


def chain_edge_forward_bytes(E, N, H, F):
    """What e adds to the composition's forward, counted in torch's elementwise passes.  Key side: q[row] gathered and written, the
    product with e read twice and written, its sum over F read, the [E, H] result scaled and added to edge_dot's.  Value side:
    alpha e formed (e read, the product written), read again by index_add and added to [N, R] zeros with float atomics, and the sum
    with spmm's out."""
    R = H * F
    key = E * (R * 4 + 8 + R * 4) + E * (3 * R * 4) + E * (R * 4 + H * 4) + E * (5 * H * 4)
    value = E * (H * 4 + 2 * R * 4) + E * (R * 4 + 8 + 2 * R * 4) + N * (R * 4) + N * (3 * R * 4)
    return key + value


def chain_edge_backward_bytes(E, N, H, F):
    """... and to its backward, at least: G[row] gathered and written for the scatter; d(alpha e) = that times e and alpha (e and
    G[row] read twice, [E, R] and its sum over F written); the key-side product's two factors' gradients (g e and g q[row]: two
    reads and a write each), the scatter of the first into dq with float atomics, and the sum of the two parts of de."""
    R = H * F
    value = E * (2 * R * 4 + 8) + E * (3 * R * 4 + H * 4) + E * (R * 4 + H * 4 + R * 4)
    key = 2 * E * (2 * R * 4 + H * 4) + E * (R * 4 + 8 + 2 * R * 4) + E * (3 * R * 4)
    return value + key


def record_bytes(mode, E, N, H, F, perm=False):
    """The byte-model fields of a record of `mode` (None, "bias", "kv_bf16", "dropout" or "edge"), in the record's order; the bench's
    pattern is square, M = N."""
    fused_f, fused_b = fused_forward_bytes(E, N, N, H, F), fused_backward_bytes(E, N, N, H, F)
    if mode == "bias":
        return {"fused_forward_bytes": fused_f, "bias_forward_bytes": bias_forward_bytes(E, H, perm), "fused_backward_bytes": fused_b,
                "bias_backward_bytes": bias_backward_bytes(E, H, perm)}
    if mode == "kv_bf16":
        return {"fused_forward_bytes": fused_f, "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F)}
    if mode == "dropout":
        return {"fused_forward_bytes": fused_f, "fused_backward_bytes": fused_b, "mask_tensor_bytes": E * H * 4}
    composed_f, composed_b = composed_forward_bytes(E, N, N, H, F), composed_backward_bytes(E, N, N, H, F)
    if mode == "edge":
        # e, de and a margin for the fused op; the chain holds q[row], two products, their gradients and autograd's saved copies besides
        e_bytes = E * H * F * 4
        return {"e_bytes": e_bytes, "needed_device_bytes": {"fused_edge": 3 * e_bytes + (2 << 30), "composed_edge": 12 * e_bytes + (2 << 30)},
                "fused_forward_bytes": fused_f + edge_forward_bytes(E, H, F, perm),
                "fused_backward_bytes": fused_b + edge_backward_bytes(E, H, F, perm),
                "composed_forward_bytes": composed_f + chain_edge_forward_bytes(E, N, H, F),
                "composed_backward_bytes": composed_b + chain_edge_backward_bytes(E, N, H, F)}
    return {"fused_forward_bytes": fused_f, "composed_forward_bytes": composed_f, "fused_backward_bytes": fused_b,
            "composed_backward_bytes": composed_b}


def entry_terms(q, k, v, scale, bias=None, edge=None):
    """The family's part of pattern_bench.sampled_reference: the score scale q_i . k_j (+ bias [E, H], at the CSR position) and the
    values v_j; edge [E, H, F], at the CSR position: added to k_j and to v_j."""
    def terms(dtype, part, idx, sub, cols, inv):
        kk, vv = pb.taken(k, cols, dtype)[inv], pb.taken(v, cols, dtype)[inv]
        if edge is not None:
            es = pb.taken(edge, idx, dtype)
            kk, vv = kk + es, vv + es
        s = (pb.taken(q, part, dtype)[sub] * kk).sum(-1) * scale
        if bias is not None:
            s = s + pb.taken(bias, idx, dtype)
        return s, vv
    return terms


def measure_plain(args, w, shape, H, F):
    """No flag: the fused op against the composition; one JSON object."""
    import torch
    import pygat_amd as pg
    scale = 1.0 / math.sqrt(F)
    g = w.generator()
    q, k, v, G = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(4))
    qs = q * scale

    def fused(*leaves):
        return pg.dot_attention(w.pattern, *leaves, scale)

    def composed(qs_, k_, v_):
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, pg.edge_dot(w.pattern, qs_, k_)), v_)

    contenders = {"fused": (fused, (q, k, v)), "composed": (composed, (qs, k, v))}
    # the same seeded inputs, both contenders priced on the sampled rows
    out_f, out_c = pb.forward_of(*contenders["fused"])(), pb.forward_of(*contenders["composed"])()
    err_of, ref_err = pb.pricer(w, entry_terms(q, k, v, scale))
    res = pb.base_record(None, args, w, H, F, scale=scale)
    res.update({"out_err_fused": err_of(out_f, f"{shape} fused out"), "out_err_composed": err_of(out_c, f"{shape} composed out"),
                "out_err_fp32_reference": ref_err, "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
                **record_bytes(None, w.E, w.N, H, F, w.perm)})
    del out_f, out_c
    pb.add_legs(res, pb.run_legs(args, contenders, G), speedup=("composed", "fused"))
    pb.write(res, args.out)


def measure_bias(args, w, shape, H, F):
    """--bias: fused with a bias, the composition with the same bias, fused without one; one JSON object."""
    import torch
    import pygat_amd as pg
    scale = 1.0 / math.sqrt(F)
    g = w.generator()
    q, k, v, G = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(4))
    bias = torch.randn(w.E, H, generator=g, device=w.dev)
    qs = q * scale

    def fused_bias(q_, k_, v_, b_):
        return pg.dot_attention(w.pattern, q_, k_, v_, scale, b_)

    def composed_bias(qs_, k_, v_, b_):
        return pg.spmm(w.pattern, pg.edge_softmax(w.pattern, pg.edge_dot(w.pattern, qs_, k_) + b_), v_)

    def fused(q_, k_, v_):
        return pg.dot_attention(w.pattern, q_, k_, v_, scale)

    contenders = {"fused_bias": (fused_bias, (q, k, v, bias)), "composed_bias": (composed_bias, (qs, k, v, bias)), "fused": (fused, (q, k, v))}
    out_f, out_c = pb.forward_of(*contenders["fused_bias"])(), pb.forward_of(*contenders["composed_bias"])()
    err_of, ref_err = pb.pricer(w, entry_terms(q, k, v, scale, bias))
    res = pb.base_record("dot_attention --bias", args, w, H, F, scale=scale)
    res.update({"out_err_fused_bias": err_of(out_f, f"{shape} fused, bias: out"),
                "out_err_composed_bias": err_of(out_c, f"{shape} composed, bias: out"), "out_err_fp32_reference": ref_err,
                **record_bytes("bias", w.E, w.N, H, F, w.perm)})
    res["bias_forward_expected_increment"] = res["bias_forward_bytes"] / res["fused_forward_bytes"]
    del out_f, out_c

    def increment(what):
        res[f"bias_{what}_measured_increment"] = res[f"fused_bias_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
    pb.add_legs(res, pb.run_legs(args, contenders, G), speedup=("composed_bias", "fused_bias"), each=increment)
    pb.write(res, args.out)
    print(f"{shape}: the byte model expects the bias to add {100 * res['bias_forward_expected_increment']:.1f} % to the fused "
          f"forward; measured {100 * res['bias_forward_measured_increment']:.1f} %", flush=True)


def measure_kv_bf16(args, w, shape, H, F):
    """--kv-bf16: the fused forward on float32 tables against the fused forward on bfloat16 tables; one JSON object."""
    import torch
    import pygat_amd as pg
    R = H * F
    scale = 1.0 / math.sqrt(F)
    g = w.generator()
    q = torch.randn(w.N, H, F, generator=g, device=w.dev)
    k16, v16 = (torch.randn(w.N, H, F, generator=g, device=w.dev).bfloat16() for _ in range(2))
    kw, vw = k16.float(), v16.float()                           # the same values, widened: what the float32 contender is fed

    def fused(*leaves):
        return pg.dot_attention(w.pattern, *leaves, scale)

    run_fp32, run_bf16 = pb.forward_of(fused, (q, kw, vw)), pb.forward_of(fused, (q, k16, v16))
    out_w, out_h = run_fp32(), run_bf16()
    equal = bool(torch.equal(out_w, out_h))
    err_of, ref_err = pb.pricer(w, entry_terms(q, kw, vw, scale))
    res = pb.base_record("dot_attention --kv-bf16", args, w, H, F, scale=scale)
    res.update({"out_bf16_equals_out_fp32_on_widened_tables": equal, "out_err_fused_bf16": err_of(out_h, f"{shape} fused, bf16 tables: out"),
                "out_err_fp32_reference": ref_err, **record_bytes("kv_bf16", w.E, w.N, H, F),
                "byte_model_ratio_per_entry": (4 * R + 4) / (8 * R + 4)})
    res["byte_model_ratio"] = res["fused_bf16_forward_bytes"] / res["fused_forward_bytes"]
    del out_w, out_h
    pb.add_legs(res, [("forward", pb.alternate({"fused_fp32": run_fp32, "fused_bf16": run_bf16}, args.rounds, args.steps, args.warmup))])
    pb.add_bf16_ratio(res)
    pb.write(res, args.out)
    print(f"{shape}: bf16 tables take {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
          f"{res['byte_model_ratio']:.3f} ({res['byte_model_ratio_per_entry']:.3f} per entry); outputs "
          f"{'bit-equal' if equal else 'DIFFER'}", flush=True)


def measure_dropout(args, w, shape, H, F):
    """--dropout: fused with dropout, fused without, the composition with the mask as a tensor; one JSON object."""
    import torch
    import pygat_amd as pg
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=w.dev)
    scale = 1.0 / math.sqrt(F)
    g = w.generator()
    q, k, v, G = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(4))
    qs = q * scale

    def fused_dropout(q_, k_, v_):
        return pg.dot_attention_dropout(w.pattern, q_, k_, v_, p, scale, seed=seed)

    def composed_dropout(qs_, k_, v_):
        alpha = pg.edge_softmax(w.pattern, pg.edge_dot(w.pattern, qs_, k_))
        return pg.spmm(w.pattern, alpha * pg.attention_dropout_mask(w.pattern, H, p, seed), v_)

    def fused(q_, k_, v_):
        return pg.dot_attention(w.pattern, q_, k_, v_, scale)

    contenders = {"fused_dropout": (fused_dropout, (q, k, v)), "composed_dropout": (composed_dropout, (qs, k, v)), "fused": (fused, (q, k, v))}
    out_f, out_c = pb.forward_of(*contenders["fused_dropout"])(), pb.forward_of(*contenders["composed_dropout"])()
    mask = pg.attention_dropout_mask(w.pattern, H, p, seed)
    err_of, ref_err = pb.pricer(w, entry_terms(q, k, v, scale), mask)
    res = pb.base_record("dot_attention --dropout", args, w, H, F, p=p, scale=scale)
    res.update({"kept_fraction": float((mask != 0).float().mean()), "out_err_fused_dropout": err_of(out_f, f"{shape} fused, dropout: out"),
                "out_err_composed_dropout": err_of(out_c, f"{shape} composed, dropout: out"), "out_err_fp32_reference": ref_err,
                **record_bytes("dropout", w.E, w.N, H, F)})
    del out_f, out_c, mask

    def increment(what):
        res[f"dropout_{what}_measured_increment"] = res[f"fused_dropout_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
    pb.add_legs(res, pb.run_legs(args, contenders, G), speedup=("composed_dropout", "fused_dropout"), each=increment)
    pb.write(res, args.out)
    print(f"{shape}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged bytes; "
          f"the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)


def measure_edge(args, w, shape, H, F):
    """--edge: dot_attention_edge against the chain of parts; one JSON object, a shape or a contender that does not fit the free
    device memory left out and named in the record."""
    import torch
    import pygat_amd as pg
    row = w.row_d
    scale = 1.0 / math.sqrt(F)
    model = record_bytes("edge", w.E, w.N, H, F, w.perm)
    e_bytes, need = model.pop("e_bytes"), model.pop("needed_device_bytes")
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(w.dev)[0]
    fits = [name for name in need if need[name] <= free]
    res = pb.base_record("dot_attention --edge", args, w, H, F, scale=scale)
    checked = {key: res.pop(key) for key in ("checked_rows", "longest_checked_row")}      # (behind the memory fields in this record)
    res.update({"e_bytes": e_bytes, "free_device_bytes": free, "needed_device_bytes": need,
                "skipped": {name: f"needs {need[name]} bytes of device memory, {free} are free" for name in need if name not in fits}})
    if "fused_edge" not in fits:
        pb.write(res, args.out)
        print(f"{shape}: skipped, e alone is {e_bytes / 1e9:.1f} GB and {free / 1e9:.1f} GB are free", flush=True)
        return
    g = w.generator()
    q, k, v, G = (torch.randn(w.N, H, F, generator=g, device=w.dev) for _ in range(4))
    e = torch.randn(w.E, H, F, generator=g, device=w.dev)

    def fused_edge(q_, k_, v_, e_):
        return pg.dot_attention_edge(w.pattern, q_, k_, v_, e_, scale)

    def composed_edge(q_, k_, v_, e_):
        s = pg.edge_dot(w.pattern, q_, k_, scale) + scale * (q_[row] * e_).sum(-1)
        alpha = pg.edge_softmax(w.pattern, s)
        return pg.spmm(w.pattern, alpha, v_) + torch.zeros_like(q_).index_add(0, row, alpha[..., None] * e_)

    fns, leaves = {"fused_edge": fused_edge, "composed_edge": composed_edge}, (q, k, v, e)
    err_of, ref_err = pb.pricer(w, entry_terms(q, k, v, scale, edge=e))
    res.update({**checked, "out_err_fp32_reference": ref_err})
    for name in list(fits):
        try:                                                    # (the estimate above is one: what does not fit after all is left out too)
            out = pb.forward_of(fns[name], leaves)()
            res[f"out_err_{name}"] = err_of(out, f"{shape} {name}: out")
            del out
            if not args.forward_only:
                pb.both_of(fns[name], leaves, G, clone=False)()      # (fresh leaves on the same memory: no second e)
        except torch.cuda.OutOfMemoryError as err:
            fits.remove(name)
            res["skipped"][name] = "out of device memory in a trial call: " + str(err).split("\n")[0]
        torch.cuda.empty_cache()
    if not fits:
        pb.write(res, args.out)
        return
    res.update(model)
    legs = pb.run_legs(args, {name: (fns[name], leaves) for name in fits}, G, clone=False)
    pb.add_legs(res, legs, speedup=("composed_edge", "fused_edge") if "composed_edge" in fits else None)
    res["peak_device_bytes"] = torch.cuda.max_memory_allocated(w.dev)
    pb.write(res, args.out)


def measure(args):
    w = pb.Workload(args, "dot_attention_bench", row_d=args.edge)
    one_shape = (measure_bias if args.bias else measure_kv_bf16 if args.kv_bf16 else measure_dropout if args.dropout else
                 measure_edge if args.edge else measure_plain)
    for shape, H, F in pb.shapes(args):
        one_shape(args, w, shape, H, F)


def parse(argv=None):
    """-> (the parser, the arguments with --out and what else depends on the mode filled in)."""
    ap = argparse.ArgumentParser()
    pb.common_arguments(ap, 420, "profiles/dot_attention_bench.jsonl; profiles/dot_attention_bias_bench.jsonl with --bias, "
                        "profiles/dot_attention_bf16_bench.jsonl with --kv-bf16, profiles/dot_attention_dropout_bench.jsonl with --dropout, "
                        "profiles/dot_attention_edge_bench.jsonl with --edge",
                        forward_only_help="skip the forward + backward leg (a kernel trace of the forward alone)")
    ap.add_argument("--bias", action="store_true", help="measure the per-entry bias: fused with a bias, the composition with it, fused without")
    ap.add_argument("--kv-bf16", action="store_true", help="measure bfloat16 k and v tables: the fused forward on float32 tables "
                    "against the fused forward on bfloat16 tables (forward only)")
    ap.add_argument("--dropout", action="store_true", help="measure seeded attention dropout at p = 0.5: fused with dropout, fused "
                    "without, the composition with the mask as a tensor")
    ap.add_argument("--edge", action="store_true", help="measure dot_attention_edge, per-entry key and value features: the fused op "
                    "against the chain of parts; a shape or contender that does not fit the free device memory is skipped")
    args = ap.parse_args(argv)
    if args.bias + args.kv_bf16 + args.dropout + args.edge > 1:
        ap.error("--bias, --kv-bf16, --dropout and --edge are separate measurements")
    if args.out is None:
        name = ("dot_attention_bias_bench.jsonl" if args.bias else "dot_attention_bf16_bench.jsonl" if args.kv_bf16 else
                "dot_attention_dropout_bench.jsonl" if args.dropout else "dot_attention_edge_bench.jsonl" if args.edge else
                "dot_attention_bench.jsonl")
        args.out = os.path.join(pb.ROOT, "profiles", name)
    return ap, args


def main():
    args = parse()[1]
    if args.child:
        return measure(args)
    pb.run_in_child(__file__, args.limit)


if __name__ == "__main__":
    main()
