"""The GATv2 score over the entries of a sparse pattern whose two sides are different tables -- a sampled block of a large graph
(destination nodes x sampled sources), attention from one node set to another, a GATv2 head inside a model built from the pattern ops.

  gatv2_attention  out[i, h, :] = sum over the entries e = (i, j) of row i of
                   softmax_row(sum_f a[h, f] LeakyReLU(x_dst[i, h, f] + x_src[j, h, f]))[e, h] * v[j, h, :]
                   fused, on the K21 kernels (csrc/k21_gatv2_attention.hip): an online softmax per row, nothing written per entry

    pattern = EdgePattern.from_indices(indices [2, E], (n_dst, n_src))      # or graph.edge_pattern()
    out = gatv2_attention(pattern, x_dst, x_src, a)                         # x_dst [n_dst, H, F], x_src [n_src, H, F], a [H, F]; v is x_src
    out = gatv2_attention(pattern, Whi, Whj, a, v=Whi)                      # the reference's SpGraphAttentionLayerV2 (layers.py:270-300)
    e = (a * F.leaky_relu(x_dst[row] + x_src[col], 0.2)).sum(-1)            # the same from parts: an [E, H, F] tensor, kept for autograd
    out = spmm(pattern, edge_softmax(pattern, e), x_src)

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
from .dot_attention import _require_heads, _require_pattern, _require_tensor, _slope
from .spmm import EdgePattern, _launch_spmm, _ptr, _stream

_OP = "gatv2_attention"
_PAD_HINT = ("zero-pad the columns of all four tensors (x_dst, x_src, a and v) to the next allowed F: zero columns of a add nothing "
             "to a score, and the first F columns of the result are unchanged")


def _checked(pattern, x_dst, x_src, a, v):
    """Every refusal that looks at the pattern and the tensors -> (H, F)."""
    _require_pattern(_OP, pattern)
    for name, t in (("x_dst", x_dst), ("x_src", x_src), ("a", a), ("v", v)):
        _require_tensor(_OP, pattern, name, t)
    if x_dst.dim() not in (2, 3):
        raise ValueError(f"pygat_amd {_OP}: x_dst [n_rows, F] or [n_rows, H, F] expected, got {tuple(x_dst.shape)}")
    for name, t in (("x_src", x_src), ("v", v)):
        if t.dim() != x_dst.dim() or t.shape[1:] != x_dst.shape[1:]:
            raise ValueError(f"pygat_amd {_OP}: {name} {tuple(t.shape)} does not match x_dst {tuple(x_dst.shape)}: the same number of "
                             f"heads and the same width expected")
    if a.shape != x_dst.shape[1:]:
        raise ValueError(f"pygat_amd {_OP}: a {tuple(a.shape)} does not match x_dst {tuple(x_dst.shape)}: a [F] with x_dst [n_rows, F], "
                         f"or a [H, F] with x_dst [n_rows, H, F], expected")
    for name, t, rows, side in (("x_dst", x_dst, pattern.n_rows, "rows"), ("x_src", x_src, pattern.n_cols, "columns"),
                                ("v", v, pattern.n_cols, "columns")):
        if t.shape[0] != rows:
            raise ValueError(f"pygat_amd {_OP}: {name} has {t.shape[0]} rows but the pattern has {rows} {side}")
    H, F = (1 if x_dst.dim() == 2 else int(x_dst.shape[1])), int(x_dst.shape[-1])
    _require_heads(_OP, H, F, _PAD_HINT)
    return H, F


def _workspace(pattern, H: int, F: int, dev):
    return torch.empty(_lib.v2_attn_workspace_bytes(pattern.nnz, H, F), dtype=torch.uint8, device=dev)


class _Gatv2AttentionFn(torch.autograd.Function):
    """shared: v is x_src (the op's v=None).  The tensor arrives in both places all the same, so autograd adds the two parts of its
    gradient -- the score's (the column pass) and the value's (the transposed SpMM) -- and the kernels get a null v."""

    @staticmethod
    def forward(ctx, pattern, x_dst, x_src, a, v, slope, shared):
        H, F = _checked(pattern, x_dst, x_src, a, v)
        ctx.pattern, ctx.slope, ctx.hf, ctx.shared = pattern, slope, (H, F), shared
        if pattern.nnz == 0:                                       # every row is without entries: zeros, and nothing is launched
            ctx.save_for_backward(x_dst, x_src, a, v, None, None, None)
            return torch.zeros_like(x_dst)
        xd, xs, ac = (t.detach().contiguous() for t in (x_dst, x_src, a))
        vc = None if shared else v.detach().contiguous()
        n, HF, dev = pattern.n_rows, H * F, xd.device
        with torch.cuda.device(dev):
            out = torch.empty(n, HF, dtype=torch.float32, device=dev)
            m, Z = (torch.empty(n, H, dtype=torch.float32, device=dev) for _ in range(2))
            ws = _workspace(pattern, H, F, dev)
            check(lib.pygat_v2_attn_forward(n, pattern.nnz, _ptr(pattern.rowptr), _ptr(pattern.col), H, F, slope, _ptr(xd), HF,
                                            _ptr(xs), HF, _ptr(ac), _ptr(vc), HF, _ptr(out), HF, _ptr(m), _ptr(Z), _ptr(ws), _stream()),
                  "v2_attn_forward")
        out = out.view(x_dst.shape)
        ctx.save_for_backward(x_dst, x_src, a, v, out, m, Z)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        x_dst, x_src, a, v, out, m, Z = ctx.saved_tensors
        pattern, slope, (H, F), shared = ctx.pattern, ctx.slope, ctx.hf, ctx.shared
        if G.dtype != torch.float32:
            raise ValueError(f"pygat_amd {_OP}: the gradient of the output must be float32, not {G.dtype}")
        need_d, need_s, need_a, need_v = ctx.needs_input_grad[1:5]
        if not (need_d or need_s or need_a or need_v):
            return (None,) * 7
        if out is None:                                            # no entries: zeros, nothing launched
            return (None,) + tuple(torch.zeros_like(t) if need else None
                                   for t, need in ((x_dst, need_d), (x_src, need_s), (a, need_a), (v, need_v))) + (None, None)
        n, nnz, HF, dev = pattern.n_rows, pattern.nnz, H * F, x_dst.device
        xd, xs, ac = (t.detach().contiguous() for t in (x_dst, x_src, a))
        vc = None if shared else v.detach().contiguous()
        Gc = G.contiguous().view(n, HF)
        with torch.cuda.device(dev):
            dd = torch.empty(n, HF, dtype=torch.float32, device=dev)
            P, S = torch.empty(nnz, H, dtype=torch.float32, device=dev), torch.empty(nnz, H, dtype=torch.float32, device=dev)
            ws = _workspace(pattern, H, F, dev)
            check(lib.pygat_v2_attn_backward_rows(n, nnz, _ptr(pattern.rowptr), _ptr(pattern.col), _ptr(pattern.perm), H, F, slope,
                                                  _ptr(xd), HF, _ptr(xs), HF, _ptr(ac), _ptr(vc), HF, _ptr(out), HF, _ptr(m), _ptr(Z),
                                                  _ptr(Gc), HF, _ptr(dd), HF, _ptr(P), _ptr(S), _ptr(ws), _stream()),
                  "v2_attn_backward_rows")
            ds = da = dv = None
            if need_s or need_a or need_v:
                rowptr_t, row_t, perm_t = pattern.transposed()
                if need_s or need_a:                # one pass forms both: the column's dx_src in registers, da from per-wave records
                    ds = torch.empty(pattern.n_cols, HF, dtype=torch.float32, device=dev)
                    da = torch.empty(HF, dtype=torch.float32, device=dev)
                    check(lib.pygat_v2_attn_backward_cols(pattern.n_cols, nnz, _ptr(rowptr_t), _ptr(row_t), _ptr(perm_t), H, F, slope,
                                                          _ptr(xd), HF, _ptr(xs), HF, _ptr(ac), _ptr(S), _ptr(ds), HF, _ptr(da),
                                                          _ptr(ws), _stream()), "v2_attn_backward_cols")
                if need_v:
                    dv = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, F, P, Gc).view(v.shape)
        return (None, dd.view(x_dst.shape) if need_d else None, ds.view(x_src.shape) if need_s else None,
                da.view(a.shape) if need_a else None, dv, None, None)


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
    Not provided: a per-entry term or edge features, dropout on the coefficients, bfloat16 tables, the value product fused into the
    column pass (dv is a K17 launch on the transposed pattern)."""
    slope = _slope(_OP, negative_slope)
    if v is None:
        return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, x_src, slope, True)
    return _Gatv2AttentionFn.apply(pattern, x_dst, x_src, a, v, slope, False)
