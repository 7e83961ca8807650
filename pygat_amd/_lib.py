"""ctypes binding of libpygat_amd.so, taken from the one declaration of its C ABI: include/pygat_amd.h.

The header is read when this module is imported; every entry point's restype / argtypes, the struct mirrors and the
constants below come from it, so a new entry point is declared once, there.  The header is plain C (no macros in
declarations, no function pointers, no varargs); parse_header refuses anything it does not understand rather than guess.

There is NO fallback: if the HIP library is missing or does not export the
expected symbols, importing this module raises.  PyTorch is used by the callers
only to own device memory and streams.
"""
from __future__ import annotations

import ctypes as C
import os
import re

# torch FIRST: it brings its own HIP runtime (torch/lib/libamdhip64.so); libpygat_amd.so must bind to that one.  Loaded
# before torch, the library pulls in /opt/rocm/lib/libamdhip64.so.7 instead, the process then holds two HIP runtimes and
# the library's launches fail with "no ROCm-capable device is detected" while torch sees the GPU (met on the GPU box when
# __graft_entry__.build() imported the package before anything had imported torch).
import torch  # noqa: F401,E402

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpygat_amd.so")
# the library is loaded in-tree and never installed: the header it was built from lies beside the package
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "pygat_amd.h")
# development aid (tools/build_variant.sh, same-lease A/B runs): another build of the same library.  Still a HIP library or
# nothing -- it is bound from this tree's header, and the ABI-version check below refuses a stale one.
from .config import config as _config  # noqa: E402
if _config.lib_path:
    LIB_PATH = os.path.abspath(_config.lib_path)

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float,
           "double": C.c_double, "size_t": C.c_size_t}
# pointers that are not plain addresses to ctypes; a `const pygat_<struct>*` is a POINTER of its mirror, every other one a c_void_p
POINTERS = {"size_t*": C.POINTER(C.c_size_t), "int*": C.POINTER(C.c_int), "char*": C.c_char_p, "const char*": C.c_char_p}
_POINTEES = set(SCALARS) | {"void", "char", "unsigned char"}


class HeaderError(ValueError):
    """A declaration of the header that parse_header does not understand."""


def _spelling(text: str, where: str, structs) -> str:
    """`const  float *const*` -> `const float* const*`; refuses anything that is not a known scalar or a pointer to a known type."""
    if not re.fullmatch(r"[\w\s*]+", text):
        raise HeaderError(f"{where}: cannot read the type in `{text.strip()}`")
    t = re.sub(r" \*", "*", " ".join(re.findall(r"\w+|\*", text)))
    base = re.sub(r"^const ", "", t.split("*")[0])
    if not (t in SCALARS or ("*" in t and (base in _POINTEES or base in structs))):
        raise HeaderError(f"{where}: unknown type `{t}`")
    return t


def parse_header(text: str):
    """The C ABI declared by the text of include/pygat_amd.h, as (consts, structs, funcs):
    consts   {name: int} of every `#define PYGAT_X <int>` and every `PYGAT_X = <int>` of an enum;
    structs  {name: [(type, field, array extent or None), ...]} of every `typedef struct { ... } name;`, fields in order;
    funcs    {name: (return type, [(type, parameter), ...])} of every `ret pygat_name(params);`, in order.
    Types are C spellings with single spaces and `*` bound to the left (`const float* const*`).  Raises HeaderError, naming
    the declaration, for whatever it cannot read: nothing is skipped and no type is guessed."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef __cplusplus.*?#endif", "", text, flags=re.S)      # extern "C" { and its }
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#define[ \t]+(PYGAT_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

    def enum(m):
        for entry in filter(None, map(str.strip, m[1].split(","))):
            e = re.fullmatch(r"(PYGAT_\w+)\s*=\s*(-?\d+)", entry)
            if not e:
                raise HeaderError(f"enum entry `{entry}`: expected PYGAT_NAME = <integer>")
            consts[e[1]] = int(e[2])
        return ""
    text = re.sub(r"\benum\s*\{(.*?)\}\s*;", enum, text, flags=re.S)

    def extent(expr, where):
        e = re.fullmatch(r"(?:(\d+)|(\w+)(?:\s*\+\s*(\d+))?)", expr.strip())
        if not e or (e[2] and e[2] not in consts):
            raise HeaderError(f"{where}: cannot resolve the extent [{expr}]")
        return int(e[1]) if e[1] else consts[e[2]] + int(e[3] or 0)

    structs = {}

    def struct(m):
        name, fields = m[2], []
        for decl in filter(None, map(str.strip, m[1].split(";"))):
            f = re.fullmatch(r"(.*?)(\w+)\s*(?:\[(.*)\])?", decl, flags=re.S)
            where = f"{name}.{f[2]}" if f else name
            if not f:
                raise HeaderError(f"{where}: cannot read the field `{decl}`")
            fields.append((_spelling(f[1], where, structs), f[2], None if f[3] is None else extent(f[3], where)))
        structs[name] = fields
        return ""
    text = re.sub(r"\btypedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)

    funcs = {}
    for decl in filter(None, map(str.strip, text.split(";"))):
        f = re.fullmatch(r"(.*?)\b(pygat_\w+)\s*\((.*)\)", decl, flags=re.S)
        if not f:
            named = re.search(r"\bpygat_\w+", decl)
            raise HeaderError(f"{named[0] if named else decl[:60]!r}: not a function declaration `ret pygat_name(params)`")
        name, params = f[2], f[3].strip()
        if "(" in params or "..." in params:
            raise HeaderError(f"{name}: function-pointer and variadic parameters are not supported")
        args = []
        for k, param in enumerate([] if params == "void" else params.split(",")):
            p = re.fullmatch(r"(.*?)(\w+)\s*", param, flags=re.S)
            if not p:
                raise HeaderError(f"{name}: cannot read parameter {k} `{param.strip()}`")
            args.append((_spelling(p[1], f"{name}({p[2]})", structs), p[2]))
        funcs[name] = (_spelling(f[1], f"{name} (return type)", structs), args)
    skipped = set(re.findall(r"\b(pygat_\w+)\s*\(", text)) - set(funcs)
    if skipped:
        raise HeaderError(f"{sorted(skipped)}: named before `(` but not parsed as functions")
    return consts, structs, funcs


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise ImportError(f"pygat_amd: {HEADER_PATH} not found. The binding is read from the C header of the tree the package "
                          f"lies in; the package is used in-tree and not installed without it.")
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except HeaderError as e:
        raise ImportError(f"pygat_amd: {HEADER_PATH}: {e}") from e


_CONSTS, _STRUCTS, _FUNCS = _read_header()
SYMBOLS = list(_FUNCS)          # every entry point declared in include/pygat_amd.h

ABI_VERSION = _CONSTS["PYGAT_ABI_VERSION"]
EINVAL = _CONSTS["PYGAT_EINVAL"]
F_ELU = _CONSTS["PYGAT_F_ELU"]
F_SKIP = _CONSTS["PYGAT_F_SKIP"]
F_MAIN_ONLY = _CONSTS["PYGAT_F_MAIN_ONLY"]
F_FIXUP_ONLY = _CONSTS["PYGAT_F_FIXUP_ONLY"]
GEMM_DEFAULT = _CONSTS["PYGAT_GEMM_DEFAULT"]
GEMM_SPLIT_BF16 = _CONSTS["PYGAT_GEMM_SPLIT_BF16"]
GEMM_FP32_MFMA = _CONSTS["PYGAT_GEMM_FP32_MFMA"]
MAX_SEGMENTS = _CONSTS["PYGAT_MAX_SEGMENTS"]
MAX_HEADS_TABLE = _CONSTS["PYGAT_MAX_HEADS_TABLE"]
MAX_ADAM_TENSORS = _CONSTS["PYGAT_ADAM_MAX_TENSORS"]
ADAM_STATE_BYTES = _CONSTS["PYGAT_ADAM_STATE_BYTES"]


def _fields(struct: str):
    """_fields_ of a struct of the header: a pointer field is an address, an array field element type * extent."""
    fields = []
    for t, name, extent in _STRUCTS[struct]:
        ct = C.c_void_p if "*" in t else SCALARS[t]
        fields.append((name, ct if extent is None else ct * extent))
    return fields


class OutSegments(C.Structure):
    _fields_ = _fields("pygat_out_segments")


class ColBlocks(C.Structure):
    """pygat_col_blocks: a [rows x cols] matrix stored as cols / w blocks of [rows x w], `stride` floats apart."""
    _fields_ = _fields("pygat_col_blocks")


class Graph(C.Structure):
    _fields_ = _fields("pygat_graph")


_MIRRORS = {"pygat_out_segments": OutSegments, "pygat_col_blocks": ColBlocks, "pygat_graph": Graph}


def _ctype(t: str):
    """The ctypes type of a parameter or return type as parse_header spells it."""
    if t in SCALARS or t in POINTERS:
        return SCALARS.get(t) or POINTERS[t]
    pointee = re.sub(r"^const ", "", t.split("*")[0])
    if pointee in _STRUCTS:
        if t != f"const {pointee}*" or pointee not in _MIRRORS:
            raise ImportError(f"pygat_amd: {HEADER_PATH}: no ctypes mirror for `{t}`")
        return C.POINTER(_MIRRORS[pointee])
    return C.c_void_p


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"pygat_amd: {LIB_PATH} not found. Build it with `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C pygat_amd/csrc`. There is no CPU/PyTorch fallback for the hot path.")
    lib = C.CDLL(LIB_PATH)
    missing = [s for s in SYMBOLS if not hasattr(lib, s)]
    if missing:
        raise ImportError(f"pygat_amd: {LIB_PATH} lacks symbols {missing}")
    for name, (ret, params) in _FUNCS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _ctype(ret), [_ctype(t) for t, _ in params]
    if lib.pygat_abi_version() != ABI_VERSION:
        raise ImportError(f"pygat_amd: ABI version {lib.pygat_abi_version()} != {ABI_VERSION}")
    return lib


lib = _load()


def check(rc: int, what: str = "") -> None:
    """Turn a negative C return code into the reference-style Python error."""
    if rc == 0:
        return
    msg = lib.pygat_last_error().decode(errors="replace")
    if rc == EINVAL:
        raise ValueError(f"pygat_amd {what}: {msg}")
    raise RuntimeError(f"pygat_amd {what}: {msg} (code {rc})")


def _workspace_bytes(what: str, *sizes) -> int:
    """A size query that answers through its last argument: pygat_<what>(sizes..., size_t* bytes)."""
    n = C.c_size_t(0)
    check(getattr(lib, "pygat_" + what)(*map(int, sizes), C.byref(n)), what)
    return n.value


def alpha_grad_workspace_bytes(nnz: int, H: int) -> int:
    """Partial records of the long rows of pygat_alpha_grad_rows / _cols (pygat_alpha_grad_workspace_bytes)."""
    return _workspace_bytes("alpha_grad_workspace_bytes", nnz, H)


def edge_workspace_bytes(nnz: int, H: int, f_out: int) -> int:
    """Scratch of the edge-logit passes (pygat_gat_edge_workspace_bytes)."""
    return _workspace_bytes("gat_edge_workspace_bytes", nnz, H, f_out)


def bf16_workspace_bytes(nnz: int, slot_edges: int, H: int, f_out: int) -> int:
    """Partial records of the bf16-table forward (pygat_gat_bf16_workspace_bytes)."""
    return _workspace_bytes("gat_bf16_workspace_bytes", nnz, slot_edges, H, f_out)


def spmm_workspace_bytes(nnz: int, H: int, F: int) -> int:
    """Partial records of the long rows of pygat_spmm_forward (pygat_spmm_workspace_bytes)."""
    return _workspace_bytes("spmm_workspace_bytes", nnz, H, F)


def edge_softmax_workspace_bytes(nnz: int, H: int) -> int:
    """Partial records of the long rows of pygat_edge_softmax_rows / _grad_rows (pygat_edge_softmax_workspace_bytes)."""
    return _workspace_bytes("edge_softmax_workspace_bytes", nnz, H)


def dot_attn_workspace_bytes(nnz: int, H: int, F: int) -> int:
    """Partial records of the long rows of pygat_dot_attn_forward / _backward_rows (pygat_dot_attn_workspace_bytes)."""
    return _workspace_bytes("dot_attn_workspace_bytes", nnz, H, F)


def add_attn_workspace_bytes(nnz: int, H: int, F: int) -> int:
    """Partial records of the long rows of pygat_add_attn_forward / _backward_rows (pygat_add_attn_workspace_bytes)."""
    return _workspace_bytes("add_attn_workspace_bytes", nnz, H, F)


def v2_attn_workspace_bytes(nnz: int, H: int, F: int) -> int:
    """Partial records of the long rows and columns and the da records of pygat_v2_attn_forward / _backward_rows / _backward_cols
    (pygat_v2_attn_workspace_bytes)."""
    return _workspace_bytes("v2_attn_workspace_bytes", nnz, H, F)


def padded_width(f_out: int) -> int:
    fp = lib.pygat_padded_width(int(f_out))
    if fp == 0:
        raise ValueError(f"pygat_amd: head width {f_out} unsupported (1..256)")
    return fp
