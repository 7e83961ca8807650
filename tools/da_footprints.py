#!/usr/bin/env python
"""Device code of K19, K20 and K21 of two trees, per kernel by its pygat_kernel_footprint name, without a device run.

    tools/da_footprints.py PARENT_CSRC THIS_CSRC > profiles/attention_dropout_footprints.txt     (..._edge_, ..._bf16_footprints.txt)

Each directory holds the three files compiled for the device alone (the Makefile's flags and --cuda-device-only -c, to
<file>.dev.o).  Per kernel: clang-offload-bundler --unbundle, llvm-readelf --notes (register counts, scratch bytes, spill counts) and
llvm-objdump -d (a kernel's text: its instruction lines with operands, without addresses and encodings).  A kernel both trees have is
identical (the same text), reordered (the same multiset of instruction lines in another order) or changed; one that only this tree has
is new.  The footprint names are read from the mangled symbols."""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
FILES = ("k19_dot_attention", "k20_additive_attention", "k21_gatv2_attention")
K19 = {0: "k19_", 1: "k19b_", 8: "k19h_", 9: "k19hb_", 2: "k19d_", 3: "k19db_", 4: "k19e_", 5: "k19eb_"}
K20 = {(0, 0, 0): "k20_", (1, 0, 0): "k20u_", (0, 1, 0): "k20d_", (1, 1, 0): "k20du_", (0, 0, 1): "k20h_", (1, 0, 1): "k20hu_"}   # LOGIT, DROP, BF16
K21 = {(0, 0, 0, 0): "k21_", (1, 0, 0, 0): "k21s_", (0, 1, 0, 0): "k21d_", (1, 1, 0, 0): "k21ds_", (0, 0, 1, 0): "k21e_", (1, 0, 1, 0): "k21es_",
       (0, 0, 0, 1): "k21h_", (1, 0, 0, 1): "k21hs_", (0, 0, 1, 1): "k21he_", (1, 0, 1, 1): "k21hes_"}                  # SHARED, DROP, EDGE, BF16


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def footprint_name(sym):
    """The pygat_kernel_footprint name of a mangled kernel symbol of the three files, or None."""
    m = re.fullmatch(r"_ZN5pygat\d+(da|aa|v2)_(fwd|bwd|col)_(long|row)_kernelI(.*)EEvNS_6DaArgsE", sym)
    if not m:
        return {"_ZN5pygat18v2_da_stage_kernelEiiPKfPf": "k21_da_stage", "_ZN5pygat18v2_da_final_kernelEiPKfPf": "k21_da_final"}.get(sym)
    owner, d, kind, args = m.groups()
    fam = re.match(r"NS_(\w+?)I(.*?)EE(.*)", args)
    flags = lambda s: tuple(int(x) for x in re.findall(r"Lb([01])", s))
    ints = lambda s: [int(x) for x in re.findall(r"L[ij](\d+)", s)]
    if fam:                                                     # a kernel of da_family.h on a family type
        name, fargs, rest = fam.groups()
        lpr, vec = ints(rest)
        if name.endswith("DaFam"):
            prefix = K19[ints(fargs)[0]]
        elif name.endswith("AaFam"):
            prefix = K20[(flags(fargs) + (0, 0))[:3]]
        else:
            prefix = K21[(flags(fargs) + (0, 0, 0))[:4]]            # (a tree from before a flag has the kernels without it)
    else:
        lpr, vec = ints(args)[:2]
        prefix = K20[(flags(args) + (0,))[:2] + (0,)] if owner == "aa" else ("k21e_" if flags(args) == (1,) else "k21_")
    return f"{prefix}{d}_{kind}_l{lpr}v{vec}"


def kernels(path):
    """{footprint name: (instruction lines, notes)} of one device-only object."""
    with tempfile.TemporaryDirectory() as tmp:
        elf = os.path.join(tmp, "k.elf")
        run(f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hip-amdgcn-amd-amdhsa--gfx950", f"--input={path}", f"--output={elf}",
            "--unbundle")
        notes, dis = run(f"{LLVM}/llvm-readelf", "--notes", elf), run(f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", elf)
    meta = {}
    for block in notes.split("- .agpr_count:")[1:]:
        get = lambda key: re.search(rf"\.{key}:\s+(\S+)", block)[1]
        meta[get("name")] = {k: int(get(k)) for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
                                                       "sgpr_spill_count")}
    text, cur = collections.defaultdict(list), None
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m[1]
        elif cur and line.startswith("\t") and not line.strip().startswith(("s_code_end", "s_nop 0", "...")):      # (padding behind a kernel)
            text[cur].append(re.sub(r"\s*//.*", "", line.strip()))
    out = {}
    for sym, mt in meta.items():
        name = footprint_name(sym)
        if name:
            assert name not in out, (name, sym)
            out[name] = (text[sym], mt)
    return out


def waves(vgpr):
    return min(8, 512 // (-(-vgpr // 8) * 8))


def main(parent, this):
    version = run(f"{LLVM}/clang", "--version").splitlines()[0]
    rows, summary = [], []
    for f in FILES:
        old, new = kernels(os.path.join(parent, f + ".dev.o")), kernels(os.path.join(this, f + ".dev.o"))
        cls = collections.Counter()
        for name in sorted(new):
            t, mt = new[name]
            if name not in old:
                c, (t0, m0) = "new", ([], None)
            else:
                t0, m0 = old[name]
                c = "identical" if t == t0 else "reordered" if collections.Counter(t) == collections.Counter(t0) else "changed"
            cls[c] += 1
            col = lambda k: f"{'-' if m0 is None else m0[k]:>4} {mt[k]:>4}"
            w0 = "-" if m0 is None else waves(m0["vgpr_count"])
            rows.append(f"{name:<26} {c:<10} instructions {len(t0) if m0 else '-':>5} {len(t):>5}  vgpr {col('vgpr_count')}  sgpr "
                        f"{col('sgpr_count')}  waves/SIMD {w0} {waves(mt['vgpr_count'])}  scratch {col('private_segment_fixed_size')}  "
                        f"vgpr spills {col('vgpr_spill_count')}  sgpr spills {col('sgpr_spill_count')}")
        gone = sorted(set(old) - set(new))
        summary.append(f"{f + '.hip':<30} {len(new):>3} kernels: " + ", ".join(f"{k} {cls[k]}" for k in ("identical", "reordered", "changed", "new"))
                       + (f"; missing from this tree: {gone}" if gone else ""))
    print("Device code of K19, K20 and K21, the parent commit against this tree, per kernel by its pygat_kernel_footprint name.  No device run:")
    print("hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --cuda-device-only -c on both trees' three files,")
    print("then tools/da_footprints.py (clang-offload-bundler --unbundle, llvm-readelf --notes, llvm-objdump -d).  identical: the same")
    print("instruction lines, operands included; reordered: the same multiset of lines in another order; changed: anything else; new: only")
    print(f"this tree has the kernel.  compiler: {version}")
    print()
    print("\n".join(summary))
    print("columns: class; then parent and this tree of: instructions, vgpr_count, sgpr_count, waves per SIMD (512 registers a SIMD, granule 8,")
    print("at most 8), scratch bytes (private_segment_fixed_size), vgpr_spill_count, sgpr_spill_count (SGPRs parked in VGPR lanes, no memory)")
    print("\n".join(rows))


if __name__ == "__main__":
    main(*sys.argv[1:3])
