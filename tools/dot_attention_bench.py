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

The measuring step runs in a child process under `timeout -k 10 <--limit seconds>`; this process never opens the GPU.  Both contenders
run in that one process, alternated round by round: a round times `steps` calls of one contender, each between two HIP events, then
the same of the other.  Reported per contender: the median over all rounds x steps timed calls (at least 50) and the spread of the
rounds' medians (largest minus smallest): a difference below that spread is not a difference.  The composition is given q already
multiplied by the scale, so it runs the parent's kernels and nothing else.

Before timing, both contenders' outputs are priced on the same seeded inputs by the rule of tests/parity.py against an fp64
computation on the CPU, on a sample of rows (the row of most entries among them): the whole [E, H, F] product does not fit an fp64
CPU run.  Algorithmic bytes are computed from the shapes (E entries, N rows, M columns, R = H F floats per row), `*_bytes` below.
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
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLE_ROWS = 1024


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


def timed_round(fn, steps):
    """-> the ms of `steps` calls, each between two events."""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def alternate(contenders, rounds, steps, warmup):
    """{name: fn} -> {name: (median ms of all timed calls, spread of the rounds' medians)}."""
    for fn in contenders.values():
        for _ in range(warmup):
            fn()
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, fn in contenders.items():
            times[name].append(timed_round(fn, steps))
    out = {}
    for name, per_round in times.items():
        medians = [statistics.median(r) for r in per_round]
        out[name] = (statistics.median([t for r in per_round for t in r]), max(medians) - min(medians))
    return out


def sampled_reference(rp, col, rows, q, k, v, scale, dtype, bias=None, mask=None, edge=None):
    """out of `rows` by torch on the CPU in `dtype`: the softmax over each row's entries of scale q_i . k_j (+ bias [E, H], at the
    CSR position), times mask [E, H] (pre-scaled, after the softmax) where given, times v_j.  edge [E, H, F], at the CSR position:
    added to k_j and to v_j."""
    import torch
    deg = rp[rows + 1] - rp[rows]
    idx = torch.cat([torch.arange(int(rp[r]), int(rp[r + 1])) for r in rows.tolist()])
    sub = torch.repeat_interleave(torch.arange(rows.numel()), deg)
    cols, inv = torch.unique(col[idx], return_inverse=True)
    qs, ks, vs = q[rows].cpu().to(dtype), k[cols].cpu().to(dtype), v[cols].cpu().to(dtype)
    kk, vv = ks[inv], vs[inv]
    if edge is not None:
        es = edge[idx.to(edge.device)].cpu().to(dtype)
        kk, vv = kk + es, vv + es
    s = (qs[sub] * kk).sum(-1) * scale
    if bias is not None:
        s = s + bias[idx.to(bias.device)].cpu().to(dtype)
    m = torch.full(qs.shape[:2], -float("inf"), dtype=dtype).scatter_reduce(0, sub[:, None].expand(-1, s.shape[1]), s, "amax")
    p = torch.exp(s - m[sub])
    alpha = p / torch.zeros_like(m).index_add(0, sub, p)[sub]
    if mask is not None:
        alpha = alpha * mask[idx.to(mask.device)].cpu().to(dtype)
    return torch.zeros_like(qs).index_add(0, sub, alpha[:, :, None] * vv)


def measure_bias(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows):
    """--bias: fused with a bias, the composition with the same bias, fused without one; one JSON object per shape."""
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        scale = 1.0 / math.sqrt(F)
        g = torch.Generator(device=dev).manual_seed(2)
        q, k, v, G = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(4))
        bias = torch.randn(E, H, generator=g, device=dev)
        qs = q * scale

        def fused_bias(q_, k_, v_, b_):
            return pg.dot_attention(pattern, q_, k_, v_, scale, b_)

        def composed_bias(qs_, k_, v_, b_):
            return pg.spmm(pattern, pg.edge_softmax(pattern, pg.edge_dot(pattern, qs_, k_) + b_), v_)

        def fused(q_, k_, v_):
            return pg.dot_attention(pattern, q_, k_, v_, scale)

        def forward_of(fn, leaves):
            def run():
                with torch.no_grad():
                    return fn(*leaves)
            return run

        def both_of(fn, leaves):
            leaves = [t.detach().clone().requires_grad_(True) for t in leaves]

            def run():
                return torch.autograd.grad(fn(*leaves), leaves, G)
            return run

        out_f, out_c = forward_of(fused_bias, (q, k, v, bias))(), forward_of(composed_bias, (qs, k, v, bias))()
        ref64 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float64, bias)
        ref32 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float32, bias)
        err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} fused, bias: out", ref32)
        err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} composed, bias: out", ref32)
        perm = pattern.perm is not None
        res = {"bench": "dot_attention --bias", "device": torch.cuda.get_device_name(0),
               "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "scale": scale,
               "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
               "longest_checked_row": int(deg[rows].max()), "out_err_fused_bias": err_f, "out_err_composed_bias": err_c,
               "out_err_fp32_reference": parity.err(ref32, ref64), "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F),
               "bias_forward_bytes": bias_forward_bytes(E, H, perm), "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F),
               "bias_backward_bytes": bias_backward_bytes(E, H, perm)}
        res["bias_forward_expected_increment"] = res["bias_forward_bytes"] / res["fused_forward_bytes"]
        del out_f, out_c
        legs = [("forward", alternate({"fused_bias": forward_of(fused_bias, (q, k, v, bias)),
                                       "composed_bias": forward_of(composed_bias, (qs, k, v, bias)),
                                       "fused": forward_of(fused, (q, k, v))}, args.rounds, args.steps, args.warmup))]
        if not args.forward_only:
            legs.append(("forward_backward", alternate({"fused_bias": both_of(fused_bias, (q, k, v, bias)),
                                                        "composed_bias": both_of(composed_bias, (qs, k, v, bias)),
                                                        "fused": both_of(fused, (q, k, v))}, args.rounds, args.steps, args.warmup)))
        for what, r in legs:
            for name in ("fused_bias", "composed_bias", "fused"):
                res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
            res[f"{what}_speedup"] = res[f"composed_bias_{what}_ms"] / res[f"fused_bias_{what}_ms"]
            res[f"bias_{what}_measured_increment"] = res[f"fused_bias_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
        print(f"{shape}: the byte model expects the bias to add {100 * res['bias_forward_expected_increment']:.1f} % to the fused "
              f"forward; measured {100 * res['bias_forward_measured_increment']:.1f} %", flush=True)
        del q, k, v, G, qs, bias
        torch.cuda.empty_cache()


def measure_kv_bf16(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows):
    """--kv-bf16: the fused forward on float32 tables against the fused forward on bfloat16 tables; one JSON object per shape."""
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        R = H * F
        scale = 1.0 / math.sqrt(F)
        g = torch.Generator(device=dev).manual_seed(2)
        q = torch.randn(N, H, F, generator=g, device=dev)
        k16, v16 = (torch.randn(N, H, F, generator=g, device=dev).bfloat16() for _ in range(2))
        kw, vw = k16.float(), v16.float()                           # the same values, widened: what the float32 contender is fed

        def run_fp32():
            with torch.no_grad():
                return pg.dot_attention(pattern, q, kw, vw, scale)

        def run_bf16():
            with torch.no_grad():
                return pg.dot_attention(pattern, q, k16, v16, scale)

        out_w, out_h = run_fp32(), run_bf16()
        equal = bool(torch.equal(out_w, out_h))
        ref64 = sampled_reference(rp_t, col_t, rows, q, kw, vw, scale, torch.float64)
        ref32 = sampled_reference(rp_t, col_t, rows, q, kw, vw, scale, torch.float32)
        err_h = parity.close_fwd(out_h[rows.to(dev)], ref64, f"{shape} fused, bf16 tables: out", ref32)
        res = {"bench": "dot_attention --kv-bf16", "device": torch.cuda.get_device_name(0),
               "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "scale": scale,
               "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
               "longest_checked_row": int(deg[rows].max()), "out_bf16_equals_out_fp32_on_widened_tables": equal,
               "out_err_fused_bf16": err_h, "out_err_fp32_reference": parity.err(ref32, ref64),
               "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F), "fused_bf16_forward_bytes": bf16_forward_bytes(E, N, N, H, F),
               "byte_model_ratio_per_entry": (4 * R + 4) / (8 * R + 4)}
        res["byte_model_ratio"] = res["fused_bf16_forward_bytes"] / res["fused_forward_bytes"]
        del out_w, out_h
        r = alternate({"fused_fp32": run_fp32, "fused_bf16": run_bf16}, args.rounds, args.steps, args.warmup)
        for name in ("fused_fp32", "fused_bf16"):
            res[f"{name}_forward_ms"], res[f"{name}_forward_spread_ms"] = r[name]
        res["measured_ratio"] = res["fused_bf16_forward_ms"] / res["fused_fp32_forward_ms"]
        res["faster_by_more_than_the_spread"] = (res["fused_fp32_forward_ms"] - res["fused_bf16_forward_ms"]
                                                 > max(res["fused_fp32_forward_spread_ms"], res["fused_bf16_forward_spread_ms"]))
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
        print(f"{shape}: bf16 tables take {res['measured_ratio']:.3f} of the float32 forward's time; the byte model says "
              f"{res['byte_model_ratio']:.3f} ({res['byte_model_ratio_per_entry']:.3f} per entry); outputs "
              f"{'bit-equal' if equal else 'DIFFER'}", flush=True)
        del q, k16, v16, kw, vw
        torch.cuda.empty_cache()


def measure_dropout(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows):
    """--dropout: fused with dropout, fused without, the composition with the mask as a tensor; one JSON object per shape."""
    p = 0.5
    seed = torch.tensor([20240607], dtype=torch.int64, device=dev)
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        scale = 1.0 / math.sqrt(F)
        g = torch.Generator(device=dev).manual_seed(2)
        q, k, v, G = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(4))
        qs = q * scale

        def fused_dropout(q_, k_, v_):
            return pg.dot_attention_dropout(pattern, q_, k_, v_, p, scale, seed=seed)

        def composed_dropout(qs_, k_, v_):
            alpha = pg.edge_softmax(pattern, pg.edge_dot(pattern, qs_, k_))
            return pg.spmm(pattern, alpha * pg.attention_dropout_mask(pattern, H, p, seed), v_)

        def fused(q_, k_, v_):
            return pg.dot_attention(pattern, q_, k_, v_, scale)

        def forward_of(fn, leaves):
            def run():
                with torch.no_grad():
                    return fn(*leaves)
            return run

        def both_of(fn, leaves):
            leaves = [t.detach().clone().requires_grad_(True) for t in leaves]

            def run():
                return torch.autograd.grad(fn(*leaves), leaves, G)
            return run

        out_f, out_c = forward_of(fused_dropout, (q, k, v))(), forward_of(composed_dropout, (qs, k, v))()
        mask = pg.attention_dropout_mask(pattern, H, p, seed)
        ref64 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float64, mask=mask)
        ref32 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float32, mask=mask)
        err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} fused, dropout: out", ref32)
        err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} composed, dropout: out", ref32)
        res = {"bench": "dot_attention --dropout", "device": torch.cuda.get_device_name(0), "p": p,
               "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "scale": scale,
               "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "checked_rows": int(rows.numel()),
               "longest_checked_row": int(deg[rows].max()), "kept_fraction": float((mask != 0).float().mean()),
               "out_err_fused_dropout": err_f, "out_err_composed_dropout": err_c, "out_err_fp32_reference": parity.err(ref32, ref64),
               "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F), "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F),
               "mask_tensor_bytes": E * H * 4}
        del out_f, out_c, mask
        legs = [("forward", alternate({"fused_dropout": forward_of(fused_dropout, (q, k, v)),
                                       "composed_dropout": forward_of(composed_dropout, (qs, k, v)),
                                       "fused": forward_of(fused, (q, k, v))}, args.rounds, args.steps, args.warmup))]
        if not args.forward_only:
            legs.append(("forward_backward", alternate({"fused_dropout": both_of(fused_dropout, (q, k, v)),
                                                        "composed_dropout": both_of(composed_dropout, (qs, k, v)),
                                                        "fused": both_of(fused, (q, k, v))}, args.rounds, args.steps, args.warmup)))
        for what, r in legs:
            for name in ("fused_dropout", "composed_dropout", "fused"):
                res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
            res[f"{what}_speedup"] = res[f"composed_dropout_{what}_ms"] / res[f"fused_dropout_{what}_ms"]
            res[f"dropout_{what}_measured_increment"] = res[f"fused_dropout_{what}_ms"] / res[f"fused_{what}_ms"] - 1.0
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
        print(f"{shape}: dropout adds {100 * res['dropout_forward_measured_increment']:.1f} % to the fused forward at unchanged bytes; "
              f"the fused op with dropout takes 1 / {res['forward_speedup']:.2f} of the composition's forward", flush=True)
        del q, k, v, G, qs
        torch.cuda.empty_cache()


def measure_edge(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows):
    """--edge: dot_attention_edge against the chain of parts; one JSON object per shape, a shape or a contender that does not fit the
    free device memory left out and named in the record."""
    row = pattern.edge_rc[:, 0].long()
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        scale = 1.0 / math.sqrt(F)
        e_bytes = E * H * F * 4
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info(dev)[0]
        # e, de and a margin for the fused op; the chain holds q[row], two products, their gradients and autograd's saved copies besides
        need = {"fused_edge": 3 * e_bytes + (2 << 30), "composed_edge": 12 * e_bytes + (2 << 30)}
        fits = [name for name in need if need[name] <= free]
        res = {"bench": "dot_attention --edge", "device": torch.cuda.get_device_name(0),
               "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E, "H": H, "F": F, "scale": scale,
               "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup, "e_bytes": e_bytes,
               "free_device_bytes": free, "needed_device_bytes": need,
               "skipped": {name: f"needs {need[name]} bytes of device memory, {free} are free" for name in need if name not in fits}}
        if "fused_edge" not in fits:
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
            print(json.dumps(res), flush=True)
            print(f"{shape}: skipped, e alone is {e_bytes / 1e9:.1f} GB and {free / 1e9:.1f} GB are free", flush=True)
            continue
        g = torch.Generator(device=dev).manual_seed(2)
        q, k, v, G = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(4))
        e = torch.randn(E, H, F, generator=g, device=dev)

        def fused_edge(q_, k_, v_, e_):
            return pg.dot_attention_edge(pattern, q_, k_, v_, e_, scale)

        def composed_edge(q_, k_, v_, e_):
            s = pg.edge_dot(pattern, q_, k_, scale) + scale * (q_[row] * e_).sum(-1)
            alpha = pg.edge_softmax(pattern, s)
            return pg.spmm(pattern, alpha, v_) + torch.zeros_like(q_).index_add(0, row, alpha[..., None] * e_)

        fns = {"fused_edge": fused_edge, "composed_edge": composed_edge}

        def forward_of(fn):
            def run():
                with torch.no_grad():
                    return fn(q, k, v, e)
            return run

        def both_of(fn):
            leaves = [t.detach().requires_grad_(True) for t in (q, k, v, e)]      # (fresh leaves on the same memory: no second e)

            def run():
                return torch.autograd.grad(fn(*leaves), leaves, G)
            return run

        ref64 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float64, edge=e)
        ref32 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float32, edge=e)
        res.update({"checked_rows": int(rows.numel()), "longest_checked_row": int(deg[rows].max()),
                    "out_err_fp32_reference": parity.err(ref32, ref64)})
        for name in list(fits):
            try:                                                    # (the estimate above is one: what does not fit after all is left out too)
                out = forward_of(fns[name])()
                res[f"out_err_{name}"] = parity.close_fwd(out[rows.to(dev)], ref64, f"{shape} {name}: out", ref32)
                del out
                if not args.forward_only:
                    both_of(fns[name])()
            except torch.cuda.OutOfMemoryError as err:
                fits.remove(name)
                res["skipped"][name] = "out of device memory in a trial call: " + str(err).split("\n")[0]
            torch.cuda.empty_cache()
        if not fits:
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
            print(json.dumps(res), flush=True)
            continue
        perm = pattern.perm is not None
        res.update({"fused_forward_bytes": fused_forward_bytes(E, N, N, H, F) + edge_forward_bytes(E, H, F, perm),
                    "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F) + edge_backward_bytes(E, H, F, perm),
                    "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F) + chain_edge_forward_bytes(E, N, H, F),
                    "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F) + chain_edge_backward_bytes(E, N, H, F)})
        legs = [("forward", alternate({name: forward_of(fns[name]) for name in fits}, args.rounds, args.steps, args.warmup))]
        if not args.forward_only:
            legs.append(("forward_backward", alternate({name: both_of(fns[name]) for name in fits}, args.rounds, args.steps,
                                                       args.warmup)))
        for what, r in legs:
            for name in fits:
                res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
            if "composed_edge" in fits:
                res[f"{what}_speedup"] = res[f"composed_edge_{what}_ms"] / res[f"fused_edge_{what}_ms"]
        res["peak_device_bytes"] = torch.cuda.max_memory_allocated(dev)
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
        del q, k, v, G, e
        torch.cuda.empty_cache()


def measure(args):
    import torch
    if not torch.cuda.is_available():
        sys.exit("dot_attention_bench: needs a GPU (a time taken anywhere else says nothing)")
    import pygat_amd as pg
    from pygat_amd.rmat import rmat_csr_numpy
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity                                                     # the one tolerance rule (tests/parity.py)
    dev = torch.device("cuda", 0)
    rp, col = rmat_csr_numpy(args.scale, args.draws, seed=1)
    graph = pg.CSRGraph(torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev))
    pattern = graph.edge_pattern()
    pattern.transposed()
    N, E = graph.n, graph.nnz
    rp_t, col_t = torch.from_numpy(rp).long(), torch.from_numpy(col).long()
    deg = rp_t[1:] - rp_t[:-1]
    picked = torch.randperm(N, generator=torch.Generator().manual_seed(3))[:SAMPLE_ROWS]
    rows = torch.unique(torch.cat([picked, torch.argmax(deg)[None]]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.bias:
        return measure_bias(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows)
    if args.kv_bf16:
        return measure_kv_bf16(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows)
    if args.dropout:
        return measure_dropout(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows)
    if args.edge:
        return measure_edge(args, torch, pg, parity, dev, pattern, N, E, rp_t, col_t, deg, rows)
    for shape in args.shapes.split(","):
        H, F = (int(x) for x in shape.split("x"))
        scale = 1.0 / math.sqrt(F)
        g = torch.Generator(device=dev).manual_seed(2)
        q, k, v, G = (torch.randn(N, H, F, generator=g, device=dev) for _ in range(4))
        qs = q * scale

        def fused(*leaves):
            return pg.dot_attention(pattern, *leaves, scale)

        def composed(qs_, k_, v_):
            return pg.spmm(pattern, pg.edge_softmax(pattern, pg.edge_dot(pattern, qs_, k_)), v_)

        def forward_of(fn, leaves):
            def run():
                with torch.no_grad():
                    return fn(*leaves)
            return run

        def both_of(fn, leaves):
            leaves = [t.detach().clone().requires_grad_(True) for t in leaves]

            def run():
                return torch.autograd.grad(fn(*leaves), leaves, G)
            return run

        # the same seeded inputs, both contenders priced on the sampled rows
        out_f, out_c = forward_of(fused, (q, k, v))(), forward_of(composed, (qs, k, v))()
        ref64 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float64)
        ref32 = sampled_reference(rp_t, col_t, rows, q, k, v, scale, torch.float32)
        err_f = parity.close_fwd(out_f[rows.to(dev)], ref64, f"{shape} fused out", ref32)
        err_c = parity.close_fwd(out_c[rows.to(dev)], ref64, f"{shape} composed out", ref32)
        res = {"device": torch.cuda.get_device_name(0), "graph": f"rmat scale {args.scale}, {args.draws} draws, seed 1", "N": N, "E": E,
               "H": H, "F": F, "scale": scale, "rounds": args.rounds, "steps_per_round": args.steps, "warmup": args.warmup,
               "checked_rows": int(rows.numel()), "longest_checked_row": int(deg[rows].max()),
               "out_err_fused": err_f, "out_err_composed": err_c, "out_err_fp32_reference": parity.err(ref32, ref64),
               "out_max_abs_fused_minus_composed": float((out_f - out_c).abs().max()),
               "fused_forward_bytes": fused_forward_bytes(E, N, N, H, F), "composed_forward_bytes": composed_forward_bytes(E, N, N, H, F),
               "fused_backward_bytes": fused_backward_bytes(E, N, N, H, F), "composed_backward_bytes": composed_backward_bytes(E, N, N, H, F)}
        del out_f, out_c
        fwd = alternate({"fused": forward_of(fused, (q, k, v)), "composed": forward_of(composed, (qs, k, v))}, args.rounds, args.steps,
                        args.warmup)
        legs = [("forward", fwd)]
        if not args.forward_only:
            legs.append(("forward_backward", alternate({"fused": both_of(fused, (q, k, v)), "composed": both_of(composed, (qs, k, v))},
                                                       args.rounds, args.steps, args.warmup)))
        for what, r in legs:
            for name in ("fused", "composed"):
                res[f"{name}_{what}_ms"], res[f"{name}_{what}_spread_ms"] = r[name]
            res[f"{what}_speedup"] = res[f"composed_{what}_ms"] / res[f"fused_{what}_ms"]
        with open(args.out, "a") as f:
            f.write(json.dumps(res) + "\n")
        print(json.dumps(res), flush=True)
        del q, k, v, G, qs
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x16,8x64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="timed calls per round and contender")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--forward-only", action="store_true", help="skip the forward + backward leg (a kernel trace of the forward alone)")
    ap.add_argument("--scale", type=int, default=20)
    ap.add_argument("--draws", type=int, default=5_000_000)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--bias", action="store_true", help="measure the per-entry bias: fused with a bias, the composition with it, fused without")
    ap.add_argument("--kv-bf16", action="store_true", help="measure bfloat16 k and v tables: the fused forward on float32 tables "
                    "against the fused forward on bfloat16 tables (forward only)")
    ap.add_argument("--dropout", action="store_true", help="measure seeded attention dropout at p = 0.5: fused with dropout, fused "
                    "without, the composition with the mask as a tensor")
    ap.add_argument("--edge", action="store_true", help="measure dot_attention_edge, per-entry key and value features: the fused op "
                    "against the chain of parts; a shape or contender that does not fit the free device memory is skipped")
    ap.add_argument("--out", default=None, help="profiles/dot_attention_bench.jsonl; profiles/dot_attention_bias_bench.jsonl with --bias, "
                    "profiles/dot_attention_bf16_bench.jsonl with --kv-bf16, profiles/dot_attention_dropout_bench.jsonl with --dropout, "
                    "profiles/dot_attention_edge_bench.jsonl with --edge")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.bias + args.kv_bf16 + args.dropout + args.edge > 1:
        ap.error("--bias, --kv-bf16, --dropout and --edge are separate measurements")
    if args.out is None:
        name = ("dot_attention_bias_bench.jsonl" if args.bias else "dot_attention_bf16_bench.jsonl" if args.kv_bf16 else
                "dot_attention_dropout_bench.jsonl" if args.dropout else "dot_attention_edge_bench.jsonl" if args.edge else
                "dot_attention_bench.jsonl")
        args.out = os.path.join(ROOT, "profiles", name)
    if args.child:
        return measure(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()
