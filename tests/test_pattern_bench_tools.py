"""The measuring harness of the attention bench tools (tools/pattern_bench.py) and what the three tools keep of their own, on the CPU:
the byte models against every committed record, the shared sampled reference against a row-by-row loop, `alternate` on scripted times,
and the command lines against the table of the commit that introduced the harness."""
import glob
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import additive_attention_bench as additive  # noqa: E402
import dot_attention_bench as dot  # noqa: E402
import edge_softmax_bench as edge_softmax  # noqa: E402
import gatv2_attention_bench as gatv2  # noqa: E402
import pattern_bench as pb  # noqa: E402

# ---------------------------------------------------------------------------------------------------------------------------------
# 1. byte models against the committed evidence
# ---------------------------------------------------------------------------------------------------------------------------------
MEASURED = ("peak_device_bytes", "free_device_bytes")     # read off the device by the run, not computed from the shapes
DEFAULT_FILES = ("dot_attention_bench.jsonl", "additive_attention_bench.jsonl", "gatv2_attention_bench.jsonl")
# (file, line, key, reason) of a field the tool's function did not reproduce when the harness was introduced: none.  All 208 fields
# of the 13 files were recomputed exactly by the functions of the commit before, the records without a "bench" key in the dot files
# (the plain mode writes none) among them.
NOT_REPRODUCED = ()


def expected_bytes(name, rec):
    """The *_bytes fields of one record from its own E, N, H, F, values and the mode flags in its "bench" string; the bench pattern
    carries no permutation."""
    flags = set(re.findall(r"--[\w-]+", rec.get("bench", "")))
    E, N, H, F = rec["E"], rec["N"], rec["H"], rec["F"]
    if name.startswith("dot_attention"):
        mode = {"--bias": "bias", "--kv-bf16": "kv_bf16", "--dropout": "dropout", "--edge": "edge"}
        assert len(flags) <= 1
        return dot.record_bytes(mode[flags.pop()] if flags else None, E, N, H, F, perm=False)
    mode = "tables_bf16" if "--tables-bf16" in flags else "dropout" if "--dropout" in flags else None
    if name.startswith("additive_attention"):
        return additive.record_bytes(mode, E, N, H, F, "--logit" in flags, perm=False)
    return gatv2.record_bytes(mode, E, N, H, F, rec["values"] == "shared", "--edge" in flags, perm=False)


def test_byte_models_reproduce_every_committed_record():
    files = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "*_attention*_bench.jsonl"))
                   if os.path.basename(p).split("_attention")[0] in ("dot", "additive", "gatv2"))
    assert len(files) == 13, files
    checked = {}
    for path in files:
        name = os.path.basename(path)
        with open(path) as f:
            for line, rec in enumerate((json.loads(s) for s in f), 1):
                want = expected_bytes(name, rec)
                keys = [k for k in rec if k.endswith("_bytes") and k not in MEASURED and (name, line, k) not in
                        {skip[:3] for skip in NOT_REPRODUCED}]
                assert keys == list(want), (name, line)                     # the same fields in the record's order
                for k in keys:
                    assert rec[k] == want[k] and type(rec[k]) is type(want[k]), (name, line, k, rec[k], want[k])
                checked[name] = checked.get(name, 0) + len(keys)
    # the three default files allow no skips: 2 + 4 + 4 records of four fields each (the additive file holds two --logit records too)
    assert sum(checked[name] for name in DEFAULT_FILES) == 40 and not any(skip[0] in DEFAULT_FILES for skip in NOT_REPRODUCED)
    assert sum(checked.values()) == 208 - len(NOT_REPRODUCED)


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the shared sampled reference against a plain loop over rows
# ---------------------------------------------------------------------------------------------------------------------------------
N_NODES, H, F, SCALE = 40, 2, 4, 0.5


def small_workload():
    """40 nodes, 120 entries: row 0 holds one, row 1 forty (a third of all), rows 2-4 three and the rest two, at seeded columns; all
    rows but two are checked."""
    g = torch.Generator().manual_seed(11)
    degs = [1, 40, 3, 3, 3] + [2] * 35
    cols = [torch.sort(torch.randperm(N_NODES, generator=g)[:d]).values for d in degs]
    rp = torch.cumsum(torch.tensor([0] + degs), 0)
    assert int(rp[-1]) == 120 and max(degs) * 3 == 120
    rows = torch.tensor([r for r in range(N_NODES) if r not in (5, 17)])
    return types.SimpleNamespace(rp_t=rp, col_t=torch.cat(cols), rows=rows)


def draws():
    g = torch.Generator().manual_seed(12)
    t = {name: torch.randn(N_NODES, H, F, generator=g, dtype=torch.float64) for name in ("q", "k", "v", "x_dst", "x_src")}
    t.update({name: torch.randn(N_NODES, H, generator=g, dtype=torch.float64) for name in ("s_dst", "s_src")})
    t["a"] = torch.randn(H, F, generator=g, dtype=torch.float64)
    t["u"] = torch.randn(120, H, generator=g, dtype=torch.float64)              # bias / edge_logit
    t["e"] = torch.randn(120, H, F, generator=g, dtype=torch.float64)
    t["mask"] = (torch.rand(120, H, generator=g) < 0.5).double() * 2.0          # dropout at p = 0.5, pre-scaled
    return t


def leaky(x):
    return torch.where(x > 0, x, 0.2 * x)


def looped(w, score, value, mask):
    """out of the checked rows, one row and one entry at a time: score(r, c, p) -> [H], value(c, p) -> [H, F], p the CSR position."""
    out = []
    for r in w.rows.tolist():
        ps = range(int(w.rp_t[r]), int(w.rp_t[r + 1]))
        s = torch.stack([score(r, int(w.col_t[p]), p) for p in ps])
        alpha = torch.softmax(s, 0)
        if mask is not None:
            alpha = alpha * mask[list(ps)]
        out.append(sum(alpha[i][:, None] * value(int(w.col_t[p]), p) for i, p in enumerate(ps)))
    return torch.stack(out)


def family_cases(t):
    """name -> (the tool's entry_terms, the same score and value written out per entry)."""
    q, k, v, u, e, a = t["q"], t["k"], t["v"], t["u"], t["e"], t["a"]
    sd, ss, xd, xs = t["s_dst"], t["s_src"], t["x_dst"], t["x_src"]
    return {
        "dot": (dot.entry_terms(q, k, v, SCALE), lambda r, c, p: SCALE * (q[r] * k[c]).sum(-1), lambda c, p: v[c]),
        "dot bias": (dot.entry_terms(q, k, v, SCALE, bias=u), lambda r, c, p: SCALE * (q[r] * k[c]).sum(-1) + u[p], lambda c, p: v[c]),
        "dot e": (dot.entry_terms(q, k, v, SCALE, edge=e), lambda r, c, p: SCALE * (q[r] * (k[c] + e[p])).sum(-1), lambda c, p: v[c] + e[p]),
        "additive": (additive.entry_terms(sd, ss, v), lambda r, c, p: leaky(sd[r] + ss[c]), lambda c, p: v[c]),
        "additive edge_logit": (additive.entry_terms(sd, ss, v, u), lambda r, c, p: leaky(sd[r] + ss[c] + u[p]), lambda c, p: v[c]),
        "gatv2": (gatv2.entry_terms(xd, xs, a, v), lambda r, c, p: (a * leaky(xd[r] + xs[c])).sum(-1), lambda c, p: v[c]),
        "gatv2 e": (gatv2.entry_terms(xd, xs, a, v, e), lambda r, c, p: (a * leaky(xd[r] + xs[c] + e[p])).sum(-1), lambda c, p: v[c]),
    }


@pytest.mark.parametrize("masked", (False, True), ids=("no mask", "mask"))
@pytest.mark.parametrize("family", ("dot", "dot bias", "dot e", "additive", "additive edge_logit", "gatv2", "gatv2 e"))
def test_sampled_reference_equals_a_loop_over_rows(family, masked):
    """rtol 1e-12: fp64 rounding (1e-16) over rows of at most forty entries, with two orders of magnitude to spare."""
    w, t = small_workload(), draws()
    terms, score, value = family_cases(t)[family]
    mask = t["mask"] if masked else None
    got = pb.sampled_reference(w, torch.float64, terms, mask)
    want = looped(w, score, value, mask)
    assert got.shape == want.shape == (38, H, F) and got.dtype == torch.float64
    torch.testing.assert_close(got, want, rtol=1e-12, atol=0.0)
    assert torch.equal(got, pb.sampled_reference(w, torch.float64, terms, mask, rows_chunk=7))      # 256 against 7 rows at a time


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. alternate on a scripted timed_round
# ---------------------------------------------------------------------------------------------------------------------------------
def test_alternate_order_median_and_spread(monkeypatch):
    log = []
    script = {"a": [[1.0, 3.0], [2.0, 2.0], [10.0, 20.0]], "b": [[5.0, 5.0], [4.0, 6.0], [7.0, 1.0]]}
    contenders = {name: (lambda name=name: log.append(("call", name))) for name in ("b", "a")}      # dict order: b, then a
    by_fn = {fn: name for name, fn in contenders.items()}

    def scripted(fn, steps):
        assert steps == 2
        log.append(("round", by_fn[fn]))
        return script[by_fn[fn]].pop(0)

    monkeypatch.setattr(pb, "timed_round", scripted)
    got = pb.alternate(contenders, rounds=3, steps=2, warmup=4)
    assert log == [("call", "b")] * 4 + [("call", "a")] * 4 + [("round", "b"), ("round", "a")] * 3
    # a: all calls 1 2 2 3 10 20 -> median 2.5; the rounds' medians 2, 2, 15 -> spread 13.  b: 1 4 5 5 6 7 -> 5; 5, 5, 4 -> 1
    assert got == {"b": (5.0, 1.0), "a": (2.5, 13.0)} and list(got) == ["b", "a"]


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the command lines
# ---------------------------------------------------------------------------------------------------------------------------------
COMMON = {"--rounds": ("rounds", 5), "--steps": ("steps", 10), "--warmup": ("warmup", 10), "--forward-only": ("forward_only", False),
          "--scale": ("scale", 20), "--draws": ("draws", 5_000_000), "--out": ("out", None), "--child": ("child", False)}
COMMAND_LINES = {        # option string -> (dest, default), as the four tools had them before the harness
    dot: {**COMMON, "--shapes": ("shapes", "8x16,8x64"), "--limit": ("limit", 420), "--bias": ("bias", False),
          "--kv-bf16": ("kv_bf16", False), "--dropout": ("dropout", False), "--edge": ("edge", False)},
    additive: {**COMMON, "--shapes": ("shapes", "8x16,8x64"), "--limit": ("limit", 420), "--logit": ("logit", False),
               "--dropout": ("dropout", False), "--tables-bf16": ("tables_bf16", False)},
    gatv2: {**COMMON, "--shapes": ("shapes", None), "--values": ("values", "shared,separate"), "--limit": ("limit", 540),
            "--dropout": ("dropout", False), "--edge": ("edge", False), "--tables-bf16": ("tables_bf16", False)},
    edge_softmax: {"--heads": ("heads", 8), "--by": ("by", "row"), "--perm": ("perm", False), "--reps": ("reps", 50),
                   "--warmup": ("warmup", 10), "--scale": ("scale", 20), "--draws": ("draws", 5_000_000), "--limit": ("limit", 240),
                   "--out": ("out", os.path.join(ROOT, "profiles", "edge_softmax_bench.jsonl")), "--child": ("child", False)},
}
DEFAULT_OUT = {          # flags -> the file under profiles/ that --out defaults to, and the --shapes a mode changes
    dot: {"": "dot_attention_bench.jsonl", "--bias": "dot_attention_bias_bench.jsonl", "--kv-bf16": "dot_attention_bf16_bench.jsonl",
          "--dropout": "dot_attention_dropout_bench.jsonl", "--edge": "dot_attention_edge_bench.jsonl"},
    additive: {"": "additive_attention_bench.jsonl", "--logit": "additive_attention_bench.jsonl",
               "--dropout": "additive_attention_dropout_bench.jsonl", "--tables-bf16": "additive_attention_bf16_bench.jsonl",
               "--tables-bf16 --logit": "additive_attention_bf16_bench.jsonl"},
    gatv2: {"": "gatv2_attention_bench.jsonl", "--dropout": "gatv2_attention_dropout_bench.jsonl", "--edge": "gatv2_attention_edge_bench.jsonl",
            "--tables-bf16": "gatv2_attention_bf16_bench.jsonl", "--tables-bf16 --edge": "gatv2_attention_edge_bf16_bench.jsonl"},
    edge_softmax: {"": "edge_softmax_bench.jsonl"},
}
TOOLS = (dot, additive, gatv2, edge_softmax)


@pytest.mark.parametrize("tool", TOOLS, ids=lambda m: m.__name__)
def test_command_line_is_what_it_was(tool):
    parser, args = tool.parse([])
    got = {a.option_strings[0]: (a.dest, a.default) for a in parser._actions if a.dest != "help"}
    assert got == COMMAND_LINES[tool]
    assert all(len(a.option_strings) == 1 for a in parser._actions if a.dest != "help")
    for flags, name in DEFAULT_OUT[tool].items():
        args = tool.parse(flags.split())[1]
        assert args.out == os.path.join(ROOT, "profiles", name), flags
        if tool is gatv2:
            assert args.shapes == ("8x16,8x32" if "--edge" in flags else "8x16,8x64")
    assert tool.parse(["--out", "x.jsonl", "--child"])[1].out == "x.jsonl"


@pytest.mark.parametrize("tool", TOOLS, ids=lambda m: m.__name__)
def test_help_needs_no_gpu(tool):
    run = subprocess.run([sys.executable, tool.__file__, "--help"], capture_output=True, text=True, cwd=ROOT)
    assert run.returncode == 0 and "--limit" in run.stdout, run.stderr
