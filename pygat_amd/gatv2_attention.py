"""The GATv2 score over the entries of a sparse pattern whose two sides are different tables -- a sampled block of a large graph
(destination nodes x sampled sources: what pygat_amd.sample_neighbors returns), attention from one node set to another, a GATv2 head inside a model built from the pattern ops.

  gatv2_attention  out[i, h, :] = sum over the entries e = (i, j) of row i of
                   softmax_row(sum_f a[h, f] LeakyReLU(x_dst[i, h, f] + x_src[j, h, f]))[e, h] * v[j, h, :]
                   fused, on the K21 kernels (csrc/k21_gatv2_attention.hip): an online softmax per row, nothing written per entry

    pattern = EdgePattern.from_indices(indices [2, E], (n_dst, n_src))      # or graph.edge_pattern()
    out = gatv2_attention(pattern, x_dst, x_src, a)                         # x_dst [n_dst, H, F], x_src [n_src, H, F], a [H, F]; v is x_src
    out = gatv2_attention(pattern, Whi, Whj, a, v=Whi)                      # the reference's SpGraphAttentionLayerV2 (layers.py:270-300)
    e = (a * F.leaky_relu(x_dst[row] + x_src[col], 0.2)).sum(-1)            # the same from parts: an [E, H, F] tensor, kept for autograd
    out = spmm(pattern, edge_softmax(pattern, e), x_src)
    out = gatv2_attention_dropout(pattern, x_dst, x_src, a, 0.6, training=self.training)    # training: dropout p on the coefficients, after
                                                                # the softmax, drawn in the kernels from a seed on the device
    out = gatv2_attention_edge(pattern, x_dst, x_src, a, lin_edge(edge_attr).view(E, H, F))    # edge features inside the score, before
                                                                # LeakyReLU (PyG's GATv2Conv with edge_dim); differentiable in e too
    with torch.no_grad():                                       # inference: bf16 tables, made once -- half the gathered bytes, the bits
        out = gatv2_attention_bf16(pattern, x_dst, x_src16, a)       # of gatv2_attention(pattern, x_dst, x_src16.float(), a)
        out = gatv2_attention_edge_bf16(pattern, x_dst, x_src16, a, e16)      # ... and of gatv2_attention_edge on the widened tables

The nonlinearity sits inside the sum over the features, so the score needs a whole F-wide row per entry and cannot be written as
additive_attention's sum of two per-node scalars.  A row's softmax runs over exactly its entries; repeated (row, col) pairs are separate
entries; entries may be unsorted and the pattern rectangular.  Differentiable in x_dst, x_src, a and v.  The backward keeps out and
(m, Z) per row; its two per-entry tensors P and S ([E, H] each) live only inside backward, between the row pass, the column pass on the
transposed pattern (dx_src and da) and the transposed SpMM that forms dv.  fp32, no float atomics, a fixed summation order: two runs
give the same bits.  Nothing is read back to the host.  There is no CPU path and no fallback to torch.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check
from ._pattern_ops import (EdgePattern, _E_WANT, _backward_opening, _dropout_front, _entry_buffers, _forward_buffers, _ptr,
                           _require_dtypes, _require_entry_rows, _require_heads, _require_inference, _require_pattern, _require_rows,
                           _require_tensor, _slope, _stream)
from .dropout import STREAM_ATT
from .spmm import _launch_spmm

_OP = "gatv2_attention"
_OP_DROP = "gatv2_attention_dropout"
_OP_EDGE = "gatv2_attention_edge"
_OP_BF16 = "gatv2_attention_bf16"
_OP_EDGE_BF16 = "gatv2_attention_edge_bf16"
_PAD_HINT = ("zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing "
             "to a score, and the first F columns of the result are unchanged")


def _checked(pattern, x_dst, x_src, a, v, op: str = _OP, sfx: str = ""):
    """Every refusal that looks at the pattern and the tensors, under the op's name -> (H, F).  sfx "16": x_src and v are the bfloat16
    tables x_src16 and v16 of the bf16 ops (their dtypes were looked at by _require_dtypes)."""
    _require_pattern(op, pattern)
    xn, vn = "x_src" + sfx, "v" + sfx
    for name, t in (("x_dst", x_dst), (xn, x_src), ("a", a), (vn, v)):
        _require_tensor(op, pattern, name, t, torch.bfloat16 if sfx and name in (xn, vn) else torch.float32)
    if x_dst.dim() not in (2, 3):
        raise ValueError(f"pygat_amd {op}: x_dst [n_rows, F] or [n_rows, H, F] expected, got {tuple(x_dst.shape)}")
    for name, t in ((xn, x_src), (vn, v)):
        if t.dim() != x_dst.dim() or t.shape[1:] != x_dst.shape[1:]:
            raise ValueError(f"pygat_amd {op}: {name} {tuple(t.shape)} does not match x_dst {tuple(x_dst.shape)}: the same number of "
                             f"heads and the same width expected")
    if a.shape != x_dst.shape[1:]:
        raise ValueError(f"pygat_amd {op}: a {tuple(a.shape)} does not match x_dst {tuple(x_dst.shape)}: a [F] with x_dst [n_rows, F], "
                         f"or a [H, F] with x_dst [n_rows, H, F], expected")
    _require_rows(op, (("x_dst", x_dst, pattern.n_rows, "rows"), (xn, x_src, pattern.n_cols, "columns"),
                       (vn, v, pattern.n_cols, "columns")))
    H, F = (1 if x_dst.dim() == 2 else int(x_dst.shape[1])), int(x_dst.shape[-1])
    _require_heads(op, H, F, _PAD_HINT)
    return H, F


def _workspace(pattern, H: int, F: int, dev):
    return torch.empty(_lib.v2_attn_workspace_bytes(pattern.nnz, H, F), dtype=torch.uint8, device=dev)


def _edge_rows(e, HF: int):
    """e as the launchers take it -> (tensor, leading dimension): the tensor itself where its rows are H * F dense elements a multiple
    of 4 elements apart and aligned to a lane's chunk of 4 (16 bytes of float32, 8 of bfloat16; a column slice of a wider tensor: no
    copy), a contiguous copy otherwise."""
    e = e.detach()
    inner = e.dim() == 2 or e.shape[1] == 1 or e.stride(1) == e.shape[2]
    chunk = 4 * e.element_size()
    if e.shape[0] > 1 and e.stride(-1) == 1 and inner and e.stride(0) >= HF and e.stride(0) % 4 == 0 and e.data_ptr() % chunk == 0:
        return e, e.stride(0)
    return e.contiguous(), HF


def _launch(pattern, which: str, H: int, F: int, slope: float, xd, xs, ac, vc, edge, drop, rest, ws, bf16: bool = False):
    """One K21 launcher call, `which` "forward", "backward_rows" or "backward_cols" (the pass on the transposed pattern: no v, and
    under dropout the plain entry point, since it reads S alone), at the entry point of what is present -- edge, the (rows, leading
    dimension) of _edge_rows, a dropout (p, seed), bf16 tables, or none -- on its argument list: the pattern's arrays, the tables, the
    group of e or of dropout, then `rest`, the pass's own arguments up to the workspace ws (one serves both passes of a backward)."""
    cols, HF = which == "backward_cols", H * F
    kind = ("edge_" if edge is not None else "dropout_" if drop is not None and not cols else "") + ("bf16_" if bf16 else "")
    n, csr = (pattern.n_cols, pattern.transposed()) if cols else (pattern.n_rows, (pattern.rowptr, pattern.col, pattern.perm))
    args = (n, pattern.nnz, _ptr(csr[0]), _ptr(csr[1]))
    if edge is not None or drop is not None or which != "forward":     # (the forward without either walks in CSR order alone; the
        args += (_ptr(csr[2]),)                                        # entry index places the rows of e and the mask's draws)
    args += (H, F, slope, _ptr(xd), HF, _ptr(xs), HF, _ptr(ac))
    if not cols:
        args += (_ptr(vc), HF)
    if edge is not None:
        args += (_ptr(edge[0]), edge[1])
    elif kind == "dropout_":
        args += (drop[0], _ptr(drop[1]), STREAM_ATT)
    check(getattr(lib, f"pygat_v2_attn_{kind}{which}")(*args, *rest, _ptr(ws), _stream()), f"v2_attn_{kind}{which}")


class _Gatv2AttentionFn(torch.autograd.Function):
    """gatv2_attention, gatv2_attention_dropout and gatv2_attention_edge.  shared: v is x_src (the op's v=None).  The tensor arrives
    in both places all the same, so autograd adds the two parts of its gradient -- the score's (the column pass) and the value's (the
    transposed SpMM) -- and the kernels get a null v.  drop: None or (p, seed) of gatv2_attention_dropout: the mask of the coefficients,
    drawn in the kernels of the two row passes from the int64 [1] seed tensor on the device; the column pass reads S alone and is the
    same launch.  e: None or the [E, H, F] rows of gatv2_attention_edge, which all three passes read (the EDGE entry points); not with
    drop."""

    @staticmethod
    def forward(ctx, pattern, x_dst, x_src, a, v, slope, shared, drop=None, e=None):
        op = _OP_EDGE if e is not None else _OP if drop is None else _OP_DROP
        H, F = _checked(pattern, x_dst, x_src, a, v, op)
        if e is not None:
            _require_entry_rows(op, pattern, "e", e, "x_dst", x_dst)
        p, seed = (None, None) if drop is None else drop
        ctx.pattern, ctx.slope, ctx.hf, ctx.shared, ctx.op, ctx.p = pattern, slope, (H, F), shared, op, p
        if pattern.nnz == 0:                                       # every row is without entries: zeros, and nothing is launched
            ctx.save_for_backward(x_dst, x_src, a, v, None, None, None, None, e)
            return torch.zeros_like(x_dst)
        xd, xs, ac = (t.detach().contiguous() for t in (x_dst, x_src, a))
        vc = None if shared else v.detach().contiguous()
        n, HF, dev = pattern.n_rows, H * F, xd.device
        with torch.cuda.device(dev):
            out, m, Z = _forward_buffers(n, H, F, dev)
            ws = _workspace(pattern, H, F, dev)
            _launch(pattern, "forward", H, F, slope, xd, xs, ac, vc, None if e is None else _edge_rows(e, HF), drop,
                    (_ptr(out), HF, _ptr(m), _ptr(Z)), ws)
        out = out.view(x_dst.shape)
        ctx.save_for_backward(x_dst, x_src, a, v, out, m, Z, seed, e)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x_dst, x_src, a, v, out, m, Z, seed, e = ctx.saved_tensors
        pattern, slope, (H, F), shared = ctx.pattern, ctx.slope, ctx.hf, ctx.shared
        need_d, need_s, need_a, need_v = ctx.needs_input_grad[1:5]
        need_e = e is not None and ctx.needs_input_grad[8]
        early = _backward_opening(ctx.op, G, out, 9,
                                  {1: (x_dst, need_d), 2: (x_src, need_s), 3: (a, need_a), 4: (v, need_v), 8: (e, need_e)})
        if early is not None:
            return early
        n, nnz, HF, dev = pattern.n_rows, pattern.nnz, H * F, x_dst.device
        xd, xs, ac = (t.detach().contiguous() for t in (x_dst, x_src, a))
        vc = None if shared else v.detach().contiguous()
        Gc = G.contiguous().view(n, HF)
        with torch.cuda.device(dev):
            dd = torch.empty(n, HF, dtype=torch.float32, device=dev)
            P, S = _entry_buffers(nnz, H, dev)
            ws = _workspace(pattern, H, F, dev)
            edge, drop, tail, de = None, None if seed is None else (ctx.p, seed), (), None
            if e is not None:
                edge = _edge_rows(e, HF)
                de = torch.empty(nnz, HF, dtype=torch.float32, device=dev) if need_e else None    # (every row is written once)
                tail = (_ptr(de), HF)
            _launch(pattern, "backward_rows", H, F, slope, xd, xs, ac, vc, edge, drop,
                    (_ptr(out), HF, _ptr(m), _ptr(Z), _ptr(Gc), HF, _ptr(dd), HF, _ptr(P), _ptr(S)) + tail, ws)
            ds = da = dv = None
            if need_s or need_a or need_v:
                rowptr_t, row_t, perm_t = pattern.transposed()
                if need_s or need_a:                # one pass forms both: the column's dx_src in registers, da from per-wave records
                    ds = torch.empty(pattern.n_cols, HF, dtype=torch.float32, device=dev)
                    da = torch.empty(HF, dtype=torch.float32, device=dev)
                    _launch(pattern, "backward_cols", H, F, slope, xd, xs, ac, None, edge, drop, (_ptr(S), _ptr(ds), HF, _ptr(da)), ws)
                if need_v:
                    dv = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, F, P, Gc).view(v.shape)
        return (None, dd.view(x_dst.shape) if need_d else None, ds.view(x_src.shape) if need_s else None,
                da.view(a.shape) if need_a else None, dv, None, None, None, de.view(e.shape) if need_e else None)


def gatv2_attention(pattern: EdgePattern, x_dst: torch.Tensor, x_src: torch.Tensor, a: torch.Tensor, v: Optional[torch.Tensor] = None,
                    negative_slope: float = 0.2) -> torch.Tensor:
    """out [n_rows, H, F] (x_dst [n_rows, H, F], x_src [n_cols, H, F], a [H, F], v [n_cols, H, F]) or out [n_rows, F] (x_dst
    [n_rows, F], x_src [n_cols, F], a [F], v [n_cols, F]): out[i] = sum over the entries (i, j) of row i of
    softmax_j(sum_f a[f] LeakyReLU(x_dst[i, f] + x_src[j, f])) * v[j], per head -- the GATv2 attention with the row side and the column
    side as different tables.  t = x_dst[i] + x_src[j] is one rounded add; LeakyReLU has the slope negative_slope (a finite float) for
    t <= 0, and its derivative at t == 0 is negative_slope, as torch's.  v=None: v is x_src, one gather per entry serves the score and
    the sum (PyG's GATv2Conv: x_dst = x W_r, x_src = x W_l).  The reference's SpGraphAttentionLayerV2 (layers.py:270-300) is
    gatv2_attention(pattern, Whi, Whj, a, v=Whi): the score on Whi_i + Whj_j, the sum over the left projection at the neighbour.
    A row without entries gets zeros; a pattern without entries launches nothing.
    Differentiable in x_dst, x_src, a and v; with v=None the gradient of x_src is the sum of the score's part and the value's.  A
    gradient that is not asked for costs no launch where a whole launch serves only it: dx_dst alone is the row pass; dx_src and da
    share the column pass on the transposed pattern; dv is one K17 launch there.  float32 GPU tensors on the pattern's device;
    1 <= H <= 64, F a power of two in 4..256, H * F <= 1024; for another F zero-pad the columns of all four tensors: zero columns of a
    add nothing to a score.
    Not provided: a per-entry term or edge features in this op (a feature row per entry inside the score is the sibling op's,
    gatv2_attention_edge; a scalar term per entry is not provided), dropout on the coefficients (that is the sibling op's,
    gatv2_attention_dropout), the value product fused into the column pass (dv is a K17 launch on the transposed pattern).
    Inference on bfloat16 tables is the sibling op's, gatv2_attention_bf16."""
    slope = _slope(_OP, negative_slope)
    if v is None:
        return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, x_src, slope, True)
    return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, v, slope, False)


def gatv2_attention_dropout(pattern: EdgePattern, x_dst: torch.Tensor, x_src: torch.Tensor, a: torch.Tensor, p: float,
                            v: Optional[torch.Tensor] = None, negative_slope: float = 0.2, *, seed: Optional[torch.Tensor] = None,
                            generator=None, training: bool = True) -> torch.Tensor:
    """gatv2_attention with dropout p on the attention coefficients, as a GATv2 trains (the reference's dropout after the
    normalisation, PyG's GATv2Conv): out[i] = sum over the entries e = (i, j) of row i of
    softmax_row(sum_f a[f] LeakyReLU(x_dst[i, f] + x_src[j, f]))[e] * mask[e] * v[j], per head, mask in {0, 1 / (1 - p)}.  The softmax
    runs over all entries of the row -- a dropped entry keeps its share of the denominator -- so this is dropout after the softmax, not
    masking before it.  Fused on the DROP instantiations of the two K21 row passes: the decision for (entry, head) is drawn in registers
    (Philox-4x32-10) in the forward and again in the backward, and no [E, H] mask exists outside backward; the column pass (dx_src and
    da) reads S alone and is gatv2_attention's.
    seed: an int64 [1] tensor on the pattern's device, read by the kernels (refill it in place between replays of a captured graph);
    None draws one with torch.randint(0, 2**62, ..., generator=generator).  The mask is attention_dropout_mask(pattern, H, p, seed), at
    the caller's entry index -- the mask dot_attention_dropout and additive_attention_dropout draw from the same seed; the same seed
    gives the same bits.  training=False or p == 0 is gatv2_attention itself; p == 1 gives zeros; a row whose entries are all dropped
    gets exact zeros.  v=None: v is x_src, as in gatv2_attention.  Differentiable in x_dst, x_src, a and v; a gradient that is not asked
    for costs no launch where a whole launch serves only it.  float32 GPU tensors with gatv2_attention's limits; bfloat16 tensors are
    refused."""
    op = _OP_DROP
    slope, drop = _dropout_front(op, pattern, (x_dst, x_src, a, v), "x_dst, x_src, a and v must be float32: there is no training path on "
                                 "bfloat16 tensors", p, negative_slope, seed, generator, training,
                                 lambda: _checked(pattern, x_dst, x_src, a, x_src if v is None else v, op))
    if drop is None:
        return gatv2_attention(pattern, x_dst, x_src, a, v, slope)
    return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, x_src if v is None else v, slope, v is None, drop)


def gatv2_attention_edge(pattern: EdgePattern, x_dst: torch.Tensor, x_src: torch.Tensor, a: torch.Tensor, e: torch.Tensor,
                         v: Optional[torch.Tensor] = None, negative_slope: float = 0.2) -> torch.Tensor:
    """gatv2_attention with a feature row per entry inside the score, as a GATv2 uses its edge features (PyG's GATv2Conv with edge_dim:
    e = lin_edge(edge_attr).view(E, H, F)): out[i] = sum over the entries c = (i, j) of row i of
    softmax_j(sum_f a[f] LeakyReLU(x_dst[i, f] + x_src[j, f] + e[c, f])) * v[j], per head.  The nonlinearity sits inside the sum over
    the features, so the edge term cannot be a scalar per entry as additive_attention's edge_logit is: it is a whole row, added before
    LeakyReLU.  e enters the score only; the sum runs over v (x_src under v=None), as in PyG.
    e is [E, H, F] ([E, F] where the tables have no head axis), float32, on the pattern's device, its rows at the caller's entry index
    as spmm's values; a row-strided e -- a column slice of a wider tensor, the row stride a multiple of 4 floats and the first row
    16-byte aligned -- is read in place by its leading dimension, without a copy.  t = (x_dst[i] + x_src[j]) + e[c] is two rounded
    adds in this order in every pass, so e = 0 gives gatv2_attention's bits in out and every gradient.  Fused on the EDGE
    instantiations of the K21 kernels: a lane reads its 16 bytes of the e row with the gathered rows of the entry, in the forward, the
    row pass and the column pass; the gradient of e, de[c] = S[c] * a * LeakyReLU'(t), is written by the row pass, once per entry: no
    atomics, two runs give the same bits.  Differentiable in x_dst, x_src, a, v and e; a gradient that is not asked for costs no
    launch that serves only it: when e does not require grad no [E, H, F] tensor is made in backward, and without dx_src and da
    there is no column pass.  A row without entries gets zeros; a row of one entry (i, j) gets v[j] bit for bit and an all-zero row of
    de; a pattern without entries launches nothing.  float32 GPU tensors with gatv2_attention's limits (1 <= H <= 64, F a power of two
    in 4..256, H * F <= 1024).
    Not provided: dropout on the coefficients together with edge features, e in the value sum, a scalar term per entry, the value
    product fused into the column pass.  Inference on bfloat16 tables is the sibling op's, gatv2_attention_edge_bf16."""
    op = _OP_EDGE
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for t in (x_dst, x_src, a, v, e)):
        raise ValueError(f"pygat_amd {op}: x_dst, x_src, a, v and e must be float32: there are no bfloat16 tables in this op")
    slope = _slope(op, negative_slope)
    _require_tensor(op, pattern, "e", e, want=_E_WANT)             # (a None here would be gatv2_attention)
    _checked(pattern, x_dst, x_src, a, x_src if v is None else v, op)
    _require_entry_rows(op, pattern, "e", e, "x_dst", x_dst)
    return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, x_src if v is None else v, slope, v is None, None, e)


def _forward_bf16(op: str, pattern, x_dst, x_src16, a, v16, e16, negative_slope):
    """gatv2_attention_bf16 (e16 None) and gatv2_attention_edge_bf16: every refusal, then one launch of the bf16 forward on the tables
    as they are -- nothing is widened, nothing is kept for a backward."""
    slope = _slope(op, negative_slope)
    _require_inference(op, _OP_EDGE if op == _OP_EDGE_BF16 else _OP, (x_dst, x_src16, a, v16, e16))
    _require_dtypes(op, (("x_dst", x_dst, torch.float32), ("x_src16", x_src16, torch.bfloat16), ("a", a, torch.float32),
                         ("v16", v16, torch.bfloat16), ("e16", e16, torch.bfloat16)))
    if op == _OP_EDGE_BF16:
        _require_tensor(op, pattern, "e16", e16, torch.bfloat16, want=_E_WANT)     # (a None here would be gatv2_attention_bf16)
    H, F = _checked(pattern, x_dst, x_src16, a, x_src16 if v16 is None else v16, op, sfx="16")
    if e16 is not None:
        _require_entry_rows(op, pattern, "e16", e16, "x_dst", x_dst)
    if pattern.nnz == 0:                                           # every row is without entries: zeros, and nothing is launched
        return torch.zeros_like(x_dst)
    xd, xs, ac = (t.detach().contiguous() for t in (x_dst, x_src16, a))
    vc = None if v16 is None else v16.detach().contiguous()
    n, HF, dev = pattern.n_rows, H * F, xd.device
    with torch.cuda.device(dev):
        out = _forward_buffers(n, H, F, dev, state=False)[0]
        ws = _workspace(pattern, H, F, dev)
        _launch(pattern, "forward", H, F, slope, xd, xs, ac, vc, None if e16 is None else _edge_rows(e16, HF), None, (_ptr(out), HF), ws,
                bf16=True)
    return out.view(x_dst.shape)


def gatv2_attention_bf16(pattern: EdgePattern, x_dst: torch.Tensor, x_src16: torch.Tensor, a: torch.Tensor,
                         v16: Optional[torch.Tensor] = None, negative_slope: float = 0.2) -> torch.Tensor:
    """gatv2_attention for inference on bfloat16 tables: x_src16 [n_cols, H, F] (or [n_cols, F]) and v16 (None, or like x_src16) are
    torch.bfloat16, made once (x_src.bfloat16()); x_dst, a and the result stay float32.  The result is gatv2_attention(pattern, x_dst,
    x_src16.float(), a, None if v16 is None else v16.float(), negative_slope) bit for bit: on the BF16 instantiations of the K21
    forward kernels a lane loads the same 4 row elements as 8 bytes and widens them in registers, and everything after the load is the
    float32 kernels' arithmetic in their order -- at half the gathered bytes and half the memory of the tables; no float32 copy of
    either is made.  v16=None: the widened x_src16 row of the one gather per entry serves the score and the sum.  Forward only: nothing
    is saved, no per-row softmax state is written and no transpose of the pattern is built.  With grad mode on and an argument that
    requires grad it raises: call it under torch.no_grad(), or use gatv2_attention on float32 tables.  A float32 x_src16 or v16, or a
    bfloat16 x_dst or a, is refused.  A row without entries gets zeros; a pattern without entries launches nothing.  The limits are
    gatv2_attention's: 1 <= H <= 64, F a power of two in 4..256, H * F <= 1024.
    Not provided: a backward, dropout, bfloat16 x_dst, a or results."""
    return _forward_bf16(_OP_BF16, pattern, x_dst, x_src16, a, v16, None, negative_slope)


def gatv2_attention_edge_bf16(pattern: EdgePattern, x_dst: torch.Tensor, x_src16: torch.Tensor, a: torch.Tensor, e16: torch.Tensor,
                              v16: Optional[torch.Tensor] = None, negative_slope: float = 0.2) -> torch.Tensor:
    """gatv2_attention_edge for inference on bfloat16 tables: x_src16, v16 (None, or like x_src16) and e16 [E, H, F] (or [E, F]; a row
    per entry at the caller's entry index) are torch.bfloat16; x_dst, a and the result stay float32.  The result is
    gatv2_attention_edge on x_src16.float(), v16.float() and e16.float() bit for bit (the BF16 | EDGE instantiations of the K21 forward
    kernels: 8-byte loads widened in registers, the float32 kernels' arithmetic after them) -- at half the bytes of the e stream, the
    largest of the op and one no cache can hold, and of the gathered rows.  A row-strided e16 -- a column slice of a wider bfloat16
    tensor, the row stride a multiple of 4 elements and the first row 8-byte aligned -- is read in place by its leading dimension; no
    float32 copy of any table is made.  Forward only, as gatv2_attention_bf16: with grad mode on and an argument that requires grad it
    raises (torch.no_grad(), or gatv2_attention_edge on float32 tables).  A float32 x_src16, v16 or e16, or a bfloat16 x_dst or a, is
    refused.  A pattern without entries launches nothing.  The limits are gatv2_attention's.
    Not provided: a backward, dropout, bfloat16 x_dst, a or results."""
    return _forward_bf16(_OP_EDGE_BF16, pattern, x_dst, x_src16, a, v16, e16, negative_slope)
