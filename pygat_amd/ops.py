"""torch.autograd.Function over the C ABI: one GAT level (all local heads) per call.

This is the op boundary that replaces `SpecialSpmmFunction` (reference
layers.py:70-90) and the ATen op sequence of `GraphAttentionLayer.forward` /
`SpGraphAttentionLayer.forward` (layers.py:32-53, 125-173) for ALL heads of a
level at once (the reference loops over heads in Python, models.py:32,34).

    out = gat_level(x, graph, Ws, As, Wskips, alpha, concat)

concat=True  -> [N, H*F'], each head ELU'd         (hidden level, models.py:32)
concat=False -> [N, F'], mean over heads, no ELU   (last level, models.py:34)

PyTorch owns memory and the stream; every FLOP of the path runs in the HIP
library.  There is no CPU or eager fallback.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import lib, check, padded_width
from .config import config as _config
from .graph import CSRGraph, slot_edges_for


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class KernelTimer:
    """Optional HIP-event spans around the kernel launches (bench.py uses it for the roofline
    figure).  Events are recorded on the stream the kernels are launched on."""

    def __init__(self):
        self.spans = []   # (name, start_event, end_event)

    def times_ms(self):
        out = {}
        for name, a, b in self.spans:
            out.setdefault(name, []).append(a.elapsed_time(b))
        return out


TIMER: Optional[KernelTimer] = None

# Backward flavour.  False: the column pass K4 writes dz per transposed edge and a light row-sum pass (4H-byte
# records fetched through perm_f) takes ds_i = sum_j dz_ij -- no second gather of a Wh row per edge.
# True: the row pass K3b recomputes dz from a gathered Wh_j first, then K4.  None (default) = by row width:
# a record fetch costs one 64-byte sector whatever H is, so below 64 floats per row (1-2 heads of 16: the
# shard of an 8- or 4-GPU head-parallel run) the second gather is the cheaper one (config-5 graph, one
# head: 1.15 ms against 1.46 ms per step; four heads: 2.45 against 2.34; eight: 4.30 against 3.84).
# PYGAT_TWO_GATHER_BACKWARD=1/0 forces either.  Both are free of atomics and bitwise reproducible; they
# differ only in the summation order of ds.
TWO_GATHER_BACKWARD: Optional[bool] = _config.two_gather_backward

# Default since round 2 for rows of up to 256 floats (above: "rowsum"): "rowlocal".  The training forward (K2) also accumulates the share of every row sum that
# went through the alpha branch of the LeakyReLU (aneg, qneg); since sum_j de_ij = 0 the row sums of dz follow
# row-locally in K3a, ds_i = -(1 - alpha)(Gp_i . aneg_i - D_i qneg_i), so the backward needs neither the second
# gather (K3b) nor per-edge dz records and their row-sum pass (K3c): K3a -> K4 -> da -> dW.  Costs one more [N, R]
# table (written by K2, read by K3a).  BACKWARD_FLAVOUR / PYGAT_BACKWARD = rowlocal | rowsum | two-gather forces a
# flavour; a non-None TWO_GATHER_BACKWARD (the older switch) selects between the two older ones.
BACKWARD_FLAVOUR: Optional[str] = _config.backward


def two_gather_backward(row_floats: int) -> bool:
    return TWO_GATHER_BACKWARD if TWO_GATHER_BACKWARD is not None else row_floats < 64


def backward_flavour(row_floats: int) -> str:
    if BACKWARD_FLAVOUR:
        if BACKWARD_FLAVOUR not in ("rowlocal", "rowsum", "two-gather"):
            raise ValueError(f"PYGAT_BACKWARD={BACKWARD_FLAVOUR!r}: expected rowlocal, rowsum or two-gather")
        return BACKWARD_FLAVOUR
    if TWO_GATHER_BACKWARD is not None:
        return "two-gather" if TWO_GATHER_BACKWARD else "rowsum"
    # measured, config-5 graph, 8 heads x F': step with rowlocal / rowsum at 128 floats per row 3.69 / 3.81 ms, at 256
    # 6.90 / 7.23, at 512 14.76 / 14.43, at 1024 29.4 / 28.3: from two 16-byte chunks per lane on the extra accumulators
    # of the training forward cost more than the row-sum pass they replace
    return "rowlocal" if row_floats <= 256 else "rowsum"


# Heads per window of the backward passes = layout of a GR row (include/pygat_amd.h, pygat_head_group): None = the library's
# default for the level's (N, H, F'); a number of FLOATS = windows of at most that many floats on rows wider than it,
# whatever the table size (tests walk tiny graphs in windows of 256 this way; until ABI 12 an environment variable of the
# C library did that).  The choice is fixed per level in its forward and handed to every backward entry point.
BWD_WINDOW_FLOATS: Optional[int] = None

# da inside the column pass (pygat_gat_backward_col with da_part + pygat_a_grad_fold) instead of a pass of its own over Wh,
# ds and dt: on tables of DA_MIN_BYTES and more (the a-gradient stream is HBM time there: 0.12 ms at config 5); a small
# graph's epoch is launch-bound and gains nothing from it (two launches either way).  PYGAT_DA_IN_K4=0 switches it off.
DA_IN_K4 = _config.da_in_k4
DA_MIN_BYTES = 32 << 20


# INTERNAL node order (round 5; CSRGraph.degree_ordered).  A level whose input carries no gradient (a first
# level: its features are the same tensor every epoch) and whose gathered table is RENUMBER_MIN_BYTES and more runs on the
# graph renumbered by descending degree: x is permuted ONCE per feature tensor (features.permuted_rows, cached like the padded
# and the sparse copies), every node table between the kernels is in internal order, K2 writes `out` and K3a reads G / the saved
# output at the caller's rows through the map inside the kernels -- no permutation pass in the step.  Results: the caller-order
# results up to the summation order inside a softmax row.  RENUMBER = False / PYGAT_RENUMBER=0 switches it off.
# Measured on the headline graph (same run, bench.py `alt_node_order`): 8 heads x 16 (512 MB table) 3.16 -> 3.06 ms (K2 0.98 -> 0.95,
# K4 1.24 -> 1.17, K3a 0.37 -> 0.40: its G / y rows are now gathers); 4 heads (256 MB) 1.90 -> 1.84; 2 heads (128 MB) 1.114 -> 1.111;
# 1 head (64 MB) 0.860 -> 0.887 -- narrow rows lose: K3a's gathers cost what K2 / K4 gain.  Hence the threshold.
# With the self-loop-only tail streamed by itself (TAIL below) every width gains on that graph: one head 0.853 -> 0.816 ms, two
# 1.107 -> 1.036, four 1.949 -> 1.751, eight 3.10 -> 2.77 (8 x 8: 1.96 -> 1.77, 8 x 64: 12.76 -> 12.34).  So: tables of
# RENUMBER_MIN_BYTES and more always, tables from RENUMBER_MIN_BYTES_TAIL when the graph has such a tail.
RENUMBER = _config.renumber
RENUMBER_MIN_BYTES = 160 << 20
RENUMBER_MIN_BYTES_TAIL = 48 << 20
# In internal order the self-loop-only nodes (alpha_ii = 1: forward = ELU(Wh_i), backward dWh_i = Gp_i) are a contiguous tail of
# the rows and a suffix of the slots: the fused kernels run on the slot prefix, two plain streams take the tail
# (csrc/k12_tail.hip).  Symmetric patterns, concat levels, the row-local backward in one head window, tails of TAIL_MIN_SHARE of
# the nodes and more.  TAIL = False / PYGAT_TAIL=0 switches it off.
TAIL = _config.tail
TAIL_MIN_SHARE = 0.05
# ... and where the projection takes it (ABI 15), the forward stream does not run: the projection's epilogue stores the tail's
# output ELU(Wh_i) at its user row instead of Wh_i (pygat_project_tail_blocked) -- the tail's Wh rows are neither written nor
# read.  Bitwise the same results.  Split-bf16 mode, no skip projection, F' = Fp, an ordinary x, and nothing in the backward
# reading the tail's Wh rows (the a-gradient folded into the column pass).  Measured at config 5 (profiles/INDEX.md, tail):
# projection 229 -> 254 us, the 125 us stream gone.  (The backward's dWh rows formed inside the weight gradient from G / y: a
# first build took the streamed-K kernel from 244 to 453 us, more than the 151 us stream it replaced
# (profiles/tail_bwd_wgrad_negative.txt).  Not because the G / y rows are gathers -- inside the tail user_row is increasing, and
# the stream reads the same rows at 5.7 TB/s -- but because of its loader: row ids fetched by global loads in the prefetch ring's
# own vmcnt queue, and selects between address computations that hipcc turns into branches, whose joins drain the ring.  With the
# ids in LDS and a branch-free loader it pays: TAIL_WGRAD_MIN_BYTES below.)  TAIL_FUSED = False / PYGAT_TAIL_FUSED=0 keeps the
# forward stream too.
TAIL_FUSED = _config.tail_fused
# The backward's tail stream and the column pass's cut-row fix-up in ONE launch (pygat_gat_backward_col_finish: the fix-up's
# work-groups first, the stream's behind them; disjoint rows, no work-group waits for another, bitwise the two launches'
# results), on tables of COL_FINISH_MIN_BYTES and more: there the fix-up is a launch of tens of microseconds of latency (some
# ten thousand cut rows) that hides beside the stream.  Below it the level keeps the two launches -- a fix-up of a few
# work-groups has nothing to hide, and the call sequence of small levels is what the tail tests pin.
COL_FINISH_MIN_BYTES = 32 << 20
# No backward tail stream at all (pygat_wgrad_tail_blocked, csrc/k1_gemm_x3.hip gemm_tn_x3w_kernel<true>): on tables of
# TAIL_WGRAD_MIN_BYTES and more the weight-gradient GEMM forms the tail's B rows G_u ELU'(out_u) itself, with the stream's one
# multiply, and the tail's dWh, ds and dt rows are neither written nor read: prepare -> column pass (main + its own fix-up) ->
# a-gradient fold -> weight gradient.  Bitwise the stream's dW.  Only where nothing else reads those rows (no input gradient, no
# skip projection, da folded in the column pass, dense x, no loss through alpha); the entry answers "not taken" for what its kernel
# does not run (product mode, a blocked x, F' != Fp, ...) and the level then streams the tail after all.  PYGAT_TAIL_WGRAD_MIN_BYTES.
TAIL_WGRAD_MIN_BYTES = _config.tail_wgrad_min_bytes


def head_group(N: int, H: int, Fo: int) -> int:
    """Heads per backward window for a level of H heads (see BWD_WINDOW_FLOATS)."""
    if BWD_WINDOW_FLOATS is None:
        return lib.pygat_head_group(N, H, Fo)
    Fp = padded_width(Fo)
    return H if H * Fp <= BWD_WINDOW_FLOATS else max(1, min(H, BWD_WINDOW_FLOATS // Fp))


class _span:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        if TIMER is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if TIMER is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            TIMER.spans.append((self.name, self.a, b))
        return False


def _ptr(t):
    return None if t is None else t.data_ptr()


# Side stream for the part of the backward that does not feed the weight-gradient GEMM: the `a` gradient (an
# HBM-bound stream over Wh, ds, dt) runs beside the MFMA-bound dW GEMM.  One per device; fork/join with events, so a
# HIP-graph capture of the level records the two branches as parallel graph nodes.
_side = {}


def _side_stream(dev) -> "torch.cuda.Stream":
    key = torch.device(dev).index
    if key not in _side:
        _side[key] = torch.cuda.Stream(device=dev)
    return _side[key]


_K1_SLAB = _config.k1_split_min_k   # measured: Cora epoch 0.614 / 0.596 / 0.595 ms at 256 / 128 / 64
OVERLAP_BACKWARD = _config.overlap_backward   # measured: the fork/join costs more than it hides


def _segments(cols_ptr_ld) -> _lib.OutSegments:
    seg = _lib.OutSegments()
    seg.nseg = len(cols_ptr_ld)
    c = 0
    for k, (ncol, t, ld) in enumerate(cols_ptr_ld):
        seg.col_start[k] = c
        seg.ptr[k] = t.data_ptr()
        seg.ld[k] = ld
        c += ncol
    seg.col_start[len(cols_ptr_ld)] = c
    return seg


def _x3g_takes(transA: bool, transB: bool, M: int, N: int, K: int) -> bool:
    """Shapes the general split-bf16 kernel takes (csrc/k1_gemm_x3.hip try_gemm_x3g; rows are assumed 16-byte aligned
    and, for a k-strided operand, padded to a multiple of 4 columns)."""
    kca, kcb = not transA, transB
    return M >= 64 and N > 64 and K >= 32 and ((K % 4) == 0 or not (kca or kcb))


def _split_k(M: int, N: int, K: int, streamed_k: bool = False, mode: Optional[str] = None, transB: bool = False) -> int:
    """K slabs of a GEMM.  General kernel: up to ~4 work-groups per CU, slabs of >= 256, at most 256 of them,
    and the partial sums (written + re-read) below a quarter of the operand bytes -- the dropout projection
    [N, H*Fin] x [H*Fin, R] streams a 100+ MB operand through few output tiles and wants 5-20 slabs, not the 2
    that "one work-group per CU" gives.  Streamed-K weight gradient (transA, K >= 4096, tools/gemm_tn_sweep.py):
    exactly one work-group per CU is the optimum at every width -- slabs x column tiles = 256 (128 columns:
    256 slabs 0.37 ms; 512 columns: 64 slabs 1.41 ms against 2.68 ms with 256; 1024 columns: 32 slabs)."""
    nt = -(-N // 32)
    if streamed_k and K >= 4096 and M * N <= 512 * 512 and (mode or get_gemm_mode()) == "split-bf16" and M > 64 and N > 64 \
            and M % 4 == 0 and N % 4 == 0:
        # the split-bf16 kernel (128 x 128 tiles): an upper bound of 512 work-groups, sized for round 4's two 4-wave
        # work-groups per CU -- try_gemm_tn_x3 caps it at one 8-wave work-group per CU (256)
        tiles = -(-M // 128) * -(-N // 128)
        return max(1, min(512 // tiles, K // 256)) if tiles < 512 else 1
    if streamed_k and K >= 4096 and M * N <= 512 * 512:
        tiles = -(-M // 128) * -(-N // (32 * min(nt, 5 if nt == 5 else 4)))
        return max(1, min(256 // tiles, K // 256)) if tiles < 256 else 1
    if (mode or get_gemm_mode()) == "split-bf16" and _x3g_takes(streamed_k, transB, M, N, K) and not (not streamed_k and K <= 256 and M >= 8192):
        # general split kernel, 128 x 128 tiles (try_gemm_x3g caps the slabs at one 8-wave work-group per CU; the figures
        # below are round 4's, two 4-wave work-groups per CU).  Its partial sums are expensive (written and
        # re-read by the reduce launch): measured on PPI level 2 (tools/gemm_bench.py --splits), projection 3144 x 2056 x
        # 1024 (425 tiles) 145 / 221 us at 1 / 2 slabs, input gradient 3144 x 1024 x 1024 (200 tiles) 82 / 115 us, weight
        # gradient 1024 x 1024 x 3144 (64 tiles) 217 / 140 / 105 / 89 / 82 us at 1 / 2 / 3 / 4 / 8: slabs only when the
        # tiles alone leave most of the chip idle, then up to 512 work-groups
        tiles = -(-M // 128) * -(-N // 128)
        return 1 if tiles >= 96 else max(1, min(K // 256, 512 // tiles))
    bn = 32 * (nt if nt <= 5 else 4)
    tiles = -(-M // 128) * -(-N // bn)
    by_traffic = int(0.125 * K * (M + N) / (M * N))
    # weight-gradient shapes of the general kernel (K = nodes, few output tiles) want ~2 work-groups per CU: the PPI
    # level-2 dW (1024 x 1024 x 3144) takes 160 us with 4 slabs, 127 us with 8 (tools/diag/gemm_split_sweep.py);
    # projections and input gradients (many tiles) lose with any split: their partial sums are as big as the output
    want = (512 if streamed_k else 256) // tiles
    return max(1, min(256, 1024 // tiles, K // 256, max(by_traffic, want))) if tiles < 1024 else 1


GEMM_MODES = {"split-bf16": _lib.GEMM_SPLIT_BF16, "fp32-mfma": _lib.GEMM_FP32_MFMA}
_mode_tls = threading.local()                        # the calling thread's choice; None = the library's default


def _mode_code(mode: Optional[str] = None) -> int:
    """The `gemm_mode` argument of a C call: an explicit name, else this thread's set_gemm_mode choice, else
    PYGAT_GEMM_DEFAULT (split-bf16 unless PYGAT_GEMM_F32=1 was in the environment when the library was loaded)."""
    mode = mode or getattr(_mode_tls, "mode", None)
    return _lib.GEMM_DEFAULT if mode is None else GEMM_MODES[mode]


def set_gemm_mode(mode: Optional[str]) -> None:
    """'split-bf16': the GEMMs cut every fp32 operand exactly into three bf16 pieces and sum all nine piece products
    in fp32 on the bf16 MFMA pipe; 'fp32-mfma': fp32 MFMA throughout; None: back to the library default
    (include/pygat_amd.h).  The C library holds no mode: this is the CALLING THREAD's choice, handed to every GEMM
    entry point as an argument; a level's backward uses the mode its forward ran with."""
    if mode is not None and mode not in GEMM_MODES:
        raise ValueError(f"gemm mode {mode!r}: expected one of {sorted(GEMM_MODES)}")
    _mode_tls.mode = mode


def get_gemm_mode() -> str:
    code = _mode_code()
    if code < 0:
        code = lib.pygat_default_gemm_mode()
    return next(k for k, v in GEMM_MODES.items() if v == code)


class gemm_mode:
    """with pygat_amd.gemm_mode("fp32-mfma"): ...  -- the product mode of the calls made inside, this thread only."""

    def __init__(self, mode: Optional[str]):
        self.mode = mode

    def __enter__(self):
        self.prev = getattr(_mode_tls, "mode", None)
        set_gemm_mode(self.mode)

    def __exit__(self, *exc):
        _mode_tls.mode = self.prev
        return False


def gemm(transA: bool, transB: bool, M: int, N: int, K: int, A: torch.Tensor, lda: int, B: torch.Tensor,
         ldb: int, segments, accumulate: bool = False, split_k: Optional[int] = None, mode: Optional[str] = None,
         a_blocks=None, c_blocks=None) -> None:
    """C = op(A) op(B), fp32 in / fp32 accumulate; `segments` = [(ncols, tensor, ld), ...]; mode: see set_gemm_mode.
    a_blocks / c_blocks: _lib.ColBlocks of a column-blocked A (stored matrix) / C (one segment), include/pygat_amd.h."""
    if c_blocks is not None:
        split_k = 1
    if split_k is None:
        split_k = _split_k(M, N, K, streamed_k=transA and not transB, mode=mode, transB=transB)
    ws = None
    if split_k > 1:
        ws = torch.empty(lib.pygat_gemm_workspace_bytes(M, N, split_k) // 4, dtype=torch.float32, device=A.device)
    seg = _segments(segments)
    if a_blocks is None and c_blocks is None:
        check(lib.pygat_gemm_f32(int(transA), int(transB), M, N, K, A.data_ptr(), lda, B.data_ptr(), ldb,
                                 C.byref(seg), int(accumulate), split_k, _ptr(ws), _mode_code(mode), _stream()), "gemm_f32")
    else:
        check(lib.pygat_gemm_f32_blocked(int(transA), int(transB), M, N, K, A.data_ptr(), lda,
                                         None if a_blocks is None else C.byref(a_blocks), B.data_ptr(), ldb, C.byref(seg),
                                         None if c_blocks is None else C.byref(c_blocks), int(accumulate), split_k, _ptr(ws),
                                         _mode_code(mode), _stream()), "gemm_f32_blocked")


class _Level:
    """Shapes and packed operands of one call."""

    def __init__(self, x, H, Fo, skip):
        # x [N, Fin], or column-blocked [blocks, N, w] (Fin = blocks * w: the head exchange's layout, pygat_amd/dist.py)
        self.blocks = None if x.dim() == 2 else _lib.ColBlocks(int(x.shape[2]), int(x.shape[1]) * int(x.shape[2]))
        self.N, self.Fin = (x.shape[0], x.shape[1]) if x.dim() == 2 else (x.shape[1], x.shape[0] * x.shape[2])
        self.ldx = self.Fin if x.dim() == 2 else int(x.shape[2])
        self.H, self.Fo, self.skip = H, Fo, skip
        self.Fp = padded_width(Fo)
        self.R = H * self.Fp
        self.hg = head_group(self.N, H, Fo)   # heads per backward pass = layout of a GR row
        self.ldw = -(-(self.R * (2 if skip else 1) + 2 * H) // 4) * 4
        self.ts = 0        # slot length of the nnz-split kernels (rows cut by a slot border cost a partial record)

    def xb(self):
        """pygat_col_blocks* of the level's input (None: an ordinary matrix)."""
        return None if self.blocks is None else C.byref(self.blocks)

    def gp_windows(self):
        """(first column in the R-wide tables, width, first column inside a GR row) of each head window's Gp."""
        for h0 in range(0, self.H, self.hg):
            hc = min(self.hg, self.H - h0)
            yield h0 * self.Fp, hc * self.Fp, h0 * (self.Fp + 4)

    def gp_col(self, h):
        """Column of head h's Gp slice inside a GR row (include/pygat_amd.h, K3a)."""
        h0 = (h // self.hg) * self.hg
        return h0 * (self.Fp + 4) + (h - h0) * self.Fp


def _in_features(x) -> int:
    """Input width of a level: x [N, Fin], or column-blocked [blocks, N, w] with Fin = blocks * w."""
    return x.shape[1] if x.dim() == 2 else x.shape[0] * x.shape[2]


def blocked_input_ok(x3: torch.Tensor) -> bool:
    """Can the level read this column-blocked activation [blocks, N, w] in place (include/pygat_amd.h, pygat_col_blocks)?
    w a power of two >= 16; float32 on the GPU."""
    w = int(x3.shape[2])
    return x3.dim() == 3 and x3.is_cuda and x3.dtype == torch.float32 and w >= 16 and (w & (w - 1)) == 0


class GATLevelFn(torch.autograd.Function):
    """forward(x, W[H,Fin,F'], a[H,2F'], Wskip[H,Fin,F']|None, graph, alpha, concat[, bwd_heads]) -> out
    (att = an AttentionTarget with grad=True: -> (out, alpha), both differentiable).

    x may be COLUMN-BLOCKED: a 3-D tensor [blocks, N, w] = the activation of a head-parallel hidden level as the exchange
    left it (block b = rank b's head columns of every node; pygat_amd/dist.py), read in place by the projection and the
    weight-gradient GEMMs; its gradient comes back in the same layout -- the one the reduce-scatter sends.

    bwd_heads = (first, count): the forward covers all H heads, the backward only that range -- dW / da of the
    other heads come back as zeros.  For a rank of a head-parallel run that computes every head's forward
    itself (cheaper than receiving the outputs over xGMI) and owns the gradients of its own heads only.
    Needs Wskip = None and no gradient into x.

    pipeline = (nchunks, on_chunk): the edge-softmax + aggregation pass (K2) runs chunk of rows by chunk of rows
    and `on_chunk(c, row_first, row_end, out)` is called after chunk c's launches are enqueued -- rows
    [row_first, row_end) of `out` are final once they have run -- so that a caller can send them off (RCCL
    all-gather on its own stream, pygat_amd/dist.py) while the next chunk is computed.  concat levels only."""

    @staticmethod
    def forward(ctx, x, W, a, Wskip, graph: CSRGraph, alpha: float, concat: bool, bwd_heads=None, pipeline=None, att=None):
        if not x.is_cuda:
            raise RuntimeError("pygat_amd: inputs must be on the GPU; the hot path has no CPU fallback")
        # the path computes in float32 (like the reference's sparse layer, layers.py:150); other float dtypes are cast
        # on the way in and their gradients cast back on the way out
        ctx.in_dtypes = (x.dtype, W.dtype, a.dtype, None if Wskip is None else Wskip.dtype)
        x = x.contiguous().float()
        W = W.contiguous().float(); a = a.contiguous().float()
        H, Fin, Fo = W.shape
        if _in_features(x) != Fin or a.shape != (H, 2 * Fo):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, W {tuple(W.shape)}, a {tuple(a.shape)}")
        skip = Wskip is not None
        if skip:
            Wskip = Wskip.contiguous().float()

        def pack(Wcat, ldw, a_pad, st):
            check(lib.pygat_pack_params(H, Fin, Fo, W.data_ptr(), a.data_ptr(), _ptr(Wskip), Wcat.data_ptr(), ldw,
                                        a_pad.data_ptr(), st), "pack_params")
        return _level_forward(ctx, tuple(ctx.needs_input_grad[:4]), x, H, Fo, skip, pack, graph, alpha, concat, bwd_heads, pipeline,
                              att=att)

    @staticmethod
    def backward(ctx, G, A=None):
        dx, dW, da, dWs = _level_backward(ctx, G, A)
        cast = lambda g_, k: g_ if g_ is None or g_.dtype == ctx.in_dtypes[k] else g_.to(ctx.in_dtypes[k])  # noqa: E731
        return (cast(dx, 0), cast(dW, 1), cast(da, 2), cast(dWs, 3), None, None, None, None, None, None)


class GATEdgeLevelFn(torch.autograd.Function):
    """The GAT level with a per-edge logit term (csrc/k15_edge_logit.hip): z_ij = s_i + t_j + u_ij in front of the LeakyReLU.
    forward(x, W [H,Fin,F'], a [H,2F'], Wskip [H,Fin,F'] | None, u [E,H], graph, alpha, concat, att) -> out; u follows the
    edge order of `graph` (graph.edge_index()) and its gradient is du_ij = dz_ij.  att: a float32 [E, H] tensor the forward
    fills with the attention coefficients (detached), or None.  The level runs in the caller's node order on an ordinary 2-D
    x: no renumbering, no self-loop tail, no head windows (H x padded F' <= 1024)."""

    @staticmethod
    def forward(ctx, x, W, a, Wskip, u, graph: CSRGraph, alpha: float, concat: bool, att):
        if not x.is_cuda:
            raise RuntimeError("pygat_amd: inputs must be on the GPU; the hot path has no CPU fallback")
        ctx.in_dtypes = (x.dtype, W.dtype, a.dtype, None if Wskip is None else Wskip.dtype, u.dtype)
        x = x.contiguous().float()
        W = W.contiguous().float(); a = a.contiguous().float(); u = u.contiguous().float()
        H, Fin, Fo = W.shape
        if x.dim() != 2 or x.shape[1] != Fin or a.shape != (H, 2 * Fo):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, W {tuple(W.shape)}, a {tuple(a.shape)}")
        skip = Wskip is not None
        if skip:
            Wskip = Wskip.contiguous().float()
        L = _Level(x, H, Fo, skip)
        if L.N != graph.n:
            raise ValueError(f"x has {L.N} rows but the graph has {graph.n} nodes")
        if tuple(u.shape) != (graph.nnz, H):
            raise ValueError(f"pygat_amd: edge_logit {tuple(u.shape)}: expected {(graph.nnz, H)} (one row per edge of the graph)")
        if L.R > 1024:
            raise ValueError(f"pygat_amd: edge_logit takes rows of at most 1024 floats (H x padded F'), not {H} x {L.Fp}")
        L.mode = get_gemm_mode()
        dev, f32 = x.device, torch.float32
        f = graph.fwd
        flags = (_lib.F_ELU if concat else 0) | (_lib.F_SKIP if skip else 0)
        with torch.cuda.device(dev):
            st = _stream()
            Wcat = torch.empty(Fin, L.ldw, dtype=f32, device=dev)
            a_pad = torch.empty(H, 2, L.Fp, dtype=f32, device=dev)
            check(lib.pygat_pack_params(H, Fin, Fo, W.data_ptr(), a.data_ptr(), _ptr(Wskip), Wcat.data_ptr(), L.ldw, a_pad.data_ptr(), st),
                  "pack_params")
            Wh = torch.empty(L.N, L.R, dtype=f32, device=dev)
            Sk = torch.empty(L.N, L.R, dtype=f32, device=dev) if skip else None
            s = torch.empty(L.N, H, dtype=f32, device=dev)
            t = torch.empty(L.N, H, dtype=f32, device=dev)
            ncols = L.R * (2 if skip else 1) + H
            tiles = -(-L.N // 128) * -(-ncols // 128)
            split_k = max(1, min(-(-384 // tiles), Fin // _K1_SLAB)) if tiles < 256 else 1
            ws = torch.empty(lib.pygat_gemm_workspace_bytes(L.N, ncols, split_k) // 4, dtype=f32, device=dev) if split_k > 1 else None
            with _span("k1_project"):
                check(lib.pygat_project_blocked(L.N, Fin, H, Fo, x.data_ptr(), L.ldx, None, Wcat.data_ptr(), L.ldw, a_pad.data_ptr(),
                                                Wh.data_ptr(), _ptr(Sk), s.data_ptr(), split_k, _ptr(ws), GEMM_MODES[L.mode], st),
                      "project")
                # s and t both from the Wh table, as the attention kernels form them
                check(lib.pygat_attn_scores(L.N, H, Fo, Wh.data_ptr(), None, a_pad.data_ptr(), s.data_ptr(), t.data_ptr(), st),
                      "attn_scores")
            hattn = torch.empty(L.N, L.R, dtype=f32, device=dev)
            m = torch.empty(L.N, H, dtype=f32, device=dev)
            Z = torch.empty(L.N, H, dtype=f32, device=dev)
            out = torch.empty(L.N, H * Fo if concat else Fo, dtype=f32, device=dev)
            part = torch.empty(_lib.edge_workspace_bytes(graph.nnz, H, Fo) // 4, dtype=f32, device=dev)
            with _span("k15_edge_forward"):
                check(lib.pygat_gat_edge_forward(f.n, f.nnz, f.rowptr.data_ptr(), f.edge_rc.data_ptr(), H, Fo, float(alpha), flags,
                                                 Wh.data_ptr(), s.data_ptr(), t.data_ptr(), _ptr(Sk), u.data_ptr(), u.shape[0],
                                                 out.data_ptr() if concat else None, hattn.data_ptr(), m.data_ptr(), Z.data_ptr(),
                                                 part.data_ptr(), st), "gat_edge_forward")
            if not concat:
                check(lib.pygat_head_mean(L.N, H, Fo, hattn.data_ptr(), _ptr(Sk), out.data_ptr(), st), "head_mean")
            if att is not None:
                with _span("k15_edge_alpha"):
                    check(lib.pygat_gat_edge_alpha(f.n, f.nnz, f.edge_rc.data_ptr(), H, float(alpha), s.data_ptr(), t.data_ptr(),
                                                       m.data_ptr(), Z.data_ptr(), u.data_ptr(), u.shape[0], att.data_ptr(), st),
                          "gat_edge_alpha")
        if any(ctx.needs_input_grad[:5]):
            ctx.save_for_backward(x, Wcat, a_pad, Wh, Sk, s, t, m, Z, hattn, out if concat else None, u)
            ctx.graph, ctx.L, ctx.alpha, ctx.concat, ctx.flags = graph, L, float(alpha), concat, flags
        return out

    @staticmethod
    def backward(ctx, G):
        x, Wcat, a_pad, Wh, Sk, s, t, m, Z, hattn, y, u = ctx.saved_tensors
        graph, L = ctx.graph, ctx.L
        H, Fo, Fin = L.H, L.Fo, L.Fin
        need = ctx.needs_input_grad
        dev, f32 = x.device, torch.float32
        G = G.contiguous().float()
        f, b = graph.fwd, graph.bwd
        with torch.cuda.device(dev):
            st = _stream()
            Gp = torch.empty(L.N, L.R, dtype=f32, device=dev)
            du = torch.empty(graph.nnz, H, dtype=f32, device=dev)
            ds = torch.empty(L.N, H, dtype=f32, device=dev)
            dt = torch.empty(L.N, H, dtype=f32, device=dev)
            dWh = torch.empty(L.N, L.R, dtype=f32, device=dev)
            part = torch.empty(_lib.edge_workspace_bytes(graph.nnz, H, Fo) // 4, dtype=f32, device=dev)
            with _span("k15_edge_rows"):
                check(lib.pygat_gat_edge_backward_rows(f.n, f.nnz, f.rowptr.data_ptr(), f.edge_rc.data_ptr(), H, Fo, ctx.alpha, ctx.flags,
                                                       Wh.data_ptr(), s.data_ptr(), t.data_ptr(), m.data_ptr(), Z.data_ptr(),
                                                       u.data_ptr(), u.shape[0], G.data_ptr(), _ptr(y), hattn.data_ptr(),
                                                       Gp.data_ptr(), du.data_ptr(), ds.data_ptr(), part.data_ptr(), st),
                      "gat_edge_backward_rows")
            with _span("k15_edge_cols"):
                check(lib.pygat_gat_edge_backward_cols(b.n, b.nnz, b.rowptr.data_ptr(), b.edge_rc.data_ptr(), graph.perm_t.data_ptr(),
                                                       H, Fo, ctx.alpha, s.data_ptr(), t.data_ptr(), m.data_ptr(), Z.data_ptr(),
                                                       u.data_ptr(), u.shape[0], Gp.data_ptr(), du.data_ptr(), ds.data_ptr(),
                                                       a_pad.data_ptr(), dt.data_ptr(), dWh.data_ptr(), part.data_ptr(), st),
                      "gat_edge_backward_cols")
            dx = dW = da = dWs = None
            if need[2]:
                da = torch.empty(H, 2 * Fo, dtype=f32, device=dev)
                wsa = torch.empty(lib.pygat_agrad_workspace_bytes(H, Fo) // 4, dtype=f32, device=dev)
                with _span("k5_agrad"):
                    check(lib.pygat_a_grad(L.N, H, Fo, Wh.data_ptr(), ds.data_ptr(), dt.data_ptr(), da.data_ptr(), wsa.data_ptr(),
                                           None, None, None, 0, 0, st), "a_grad")
            if need[1]:
                split_k = _split_k(Fin, L.R, L.N, streamed_k=True, mode=L.mode)
                wsw = torch.empty(lib.pygat_wgrad_workspace_bytes(Fin, H, Fo, split_k) // 4, dtype=f32, device=dev)
                dW = torch.empty(H, Fin, Fo, dtype=f32, device=dev)
                with _span("k5_wgrad"):
                    check(lib.pygat_wgrad_blocked(L.N, Fin, H, Fo, x.data_ptr(), L.ldx, None, dWh.data_ptr(), None, a_pad.data_ptr(),
                                                  dW.data_ptr(), split_k, wsw.data_ptr(), 0, 0, GEMM_MODES[L.mode], st), "wgrad")
            if L.skip and need[3]:
                dSc = torch.empty(Fin, L.R, dtype=f32, device=dev)
                gemm(True, False, Fin, L.R, L.N, x, L.ldx, Gp, L.R, [(L.R, dSc, L.R)], mode=L.mode)
                dWs = torch.empty(H, Fin, Fo, dtype=f32, device=dev)
                check(lib.pygat_unpack_wgrad(H, Fin, Fo, dSc.data_ptr(), L.R, 0, dWs.data_ptr(), st), "unpack")
            if need[0]:
                dx = torch.empty(x.shape, dtype=f32, device=dev)
                with _span("k5_xgrad"):
                    gemm(False, True, L.N, Fin, L.R, dWh, L.R, Wcat, L.ldw, [(Fin, dx, L.ldx)], mode=L.mode)
                    if L.skip:
                        gemm(False, True, L.N, Fin, L.R, Gp, L.R, Wcat[:, L.R:], L.ldw, [(Fin, dx, L.ldx)], accumulate=True, split_k=1,
                             mode=L.mode)
        outs = [dx, dW, da, dWs, du if need[4] else None]
        outs = [g_ if g_ is None or g_.dtype == dt_ else g_.to(dt_) for g_, dt_ in zip(outs, ctx.in_dtypes)]
        return (*outs, None, None, None, None)


def _edge_logit_level(x, graph, Ws, As, Wskips, alpha, concat, edge_logit, return_attention, pipeline, xs, attention_order,
                      bwd_heads=None):
    """gat_level(..., edge_logit=u): checks, broadcast of u over the heads, and the level (GATEdgeLevelFn)."""
    from .graph import InternalOrderView
    H = len(Ws)
    for name, val in (("pipeline", pipeline), ("xs", xs), ("bwd_heads", bwd_heads), ("attention_order", attention_order)):
        if val is not None:
            raise ValueError(f"pygat_amd: edge_logit does not take {name}: the edge-logit level runs whole, on a dense x, in the "
                             "caller's node order")
    if isinstance(return_attention, str):
        attention_mode(return_attention)
        raise ValueError("pygat_amd: edge_logit does not take return_attention=\"grad\"; return_attention=True gives the detached "
                         "coefficients")
    if isinstance(graph, InternalOrderView) or getattr(graph, "user_row", None) is not None:
        raise ValueError("pygat_amd: edge_logit needs the caller's graph (a CSRGraph without a row map), not an InternalOrderView "
                         "or CSRGraph.degree_ordered(): its rows follow graph.edge_index()")
    if not isinstance(edge_logit, torch.Tensor) or not edge_logit.is_floating_point():
        raise ValueError("pygat_amd: edge_logit must be a floating-point tensor [E, H], [E, 1] or [E]")
    if x.dim() != 2:
        raise ValueError("pygat_amd: edge_logit does not take a column-blocked x")
    u = edge_logit
    E = graph.nnz
    if u.dim() == 1:
        u = u[:, None]
    if u.dim() != 2 or u.shape[0] != E or u.shape[1] not in (1, H):
        raise ValueError(f"pygat_amd: edge_logit {tuple(edge_logit.shape)}: expected [{E}, {H}], [{E}, 1] or [{E}] "
                         "(one row per edge of graph.edge_index())")
    if u.shape[1] != H:
        u = u.expand(E, H)       # (autograd sums the gradient over the heads)
    u = u.to(x.device)
    W = torch.stack(list(Ws), 0)
    a = torch.stack([p.reshape(-1) for p in As], 0)
    Wskip = torch.stack(list(Wskips), 0) if Wskips is not None else None
    att = torch.empty(E, H, dtype=torch.float32, device=x.device) if return_attention else None
    out = GATEdgeLevelFn.apply(x, W, a, Wskip, u, graph, alpha, concat, att)
    return (out, att) if return_attention else out


def _bf16_level(x, graph, Ws, As, Wskips, alpha, concat, table_dtype, return_attention, pipeline, xs, attention_order, edge_logit):
    """gat_level(..., table_dtype=torch.bfloat16): the inference forward on a bf16 feature table (csrc/k16_bf16_forward.hip).
    The projection runs as always (K1, the caller's GEMM mode, fp32); the pack pass rounds it once to Whq = bf16(Wh) (nearest,
    ties to even) and forms s from the rounded rows; the forward gathers Whq, forms t from the gathered rows and does everything
    else in fp32: the level is the fp32 level applied to Whq.  The skip term stays fp32.  No backward."""
    from .graph import InternalOrderView
    if table_dtype is not torch.bfloat16:
        raise ValueError(f"pygat_amd: table_dtype={table_dtype!r}: expected None (the fp32 tables) or torch.bfloat16")
    for name, val in (("pipeline", pipeline), ("sparse xs", xs), ("attention_order", attention_order), ("edge_logit", edge_logit)):
        if val is not None:
            raise ValueError(f"pygat_amd: table_dtype does not take {name}: the bf16-table forward runs whole, on a dense x, in the "
                             "caller's node order")
    if return_attention:
        raise ValueError("pygat_amd: table_dtype does not take return_attention (the bf16-table forward keeps no softmax state)")
    if isinstance(graph, InternalOrderView) or getattr(graph, "user_row", None) is not None:
        raise ValueError("pygat_amd: table_dtype needs the caller's graph (a CSRGraph without a row map), not an InternalOrderView "
                         "or CSRGraph.degree_ordered()")
    if x.dim() != 2:
        raise ValueError("pygat_amd: table_dtype does not take a column-blocked x")
    params = list(Ws) + list(As) + (list(Wskips) if Wskips is not None else [])
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        raise ValueError("pygat_amd: the bf16-table forward is inference only (it has no backward): call it under torch.no_grad() "
                         "or on detached parameters")
    if not x.is_cuda:
        raise RuntimeError("pygat_amd: inputs must be on the GPU; the hot path has no CPU fallback")
    with torch.no_grad():
        x = x.contiguous().float()
        W = torch.stack([w.float() for w in Ws], 0).contiguous()
        a = torch.stack([p.reshape(-1).float() for p in As], 0).contiguous()
        Wskip = torch.stack([w.float() for w in Wskips], 0).contiguous() if Wskips is not None else None
        H, Fin, Fo = W.shape
        if x.shape[1] != Fin or a.shape != (H, 2 * Fo):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, W {tuple(W.shape)}, a {tuple(a.shape)}")
        skip = Wskip is not None
        L = _Level(x, H, Fo, skip)
        if L.N != graph.n:
            raise ValueError(f"x has {L.N} rows but the graph has {graph.n} nodes")
        L.ts = slot_edges_for(L.R, graph.slot_edges)
        L.mode = get_gemm_mode()
        dev, f32 = x.device, torch.float32
        flags = (_lib.F_ELU if concat else 0) | (_lib.F_SKIP if skip else 0)
        with torch.cuda.device(dev):
            st = _stream()
            Wcat = torch.empty(Fin, L.ldw, dtype=f32, device=dev)
            a_pad = torch.empty(H, 2, L.Fp, dtype=f32, device=dev)
            check(lib.pygat_pack_params(H, Fin, Fo, W.data_ptr(), a.data_ptr(), _ptr(Wskip), Wcat.data_ptr(), L.ldw, a_pad.data_ptr(), st),
                  "pack_params")
            Wh = torch.empty(L.N, L.R, dtype=f32, device=dev)
            Sk = torch.empty(L.N, L.R, dtype=f32, device=dev) if skip else None
            s = torch.empty(L.N, H, dtype=f32, device=dev)
            ncols = L.R * (2 if skip else 1) + H
            tiles = -(-L.N // 128) * -(-ncols // 128)
            split_k = max(1, min(-(-384 // tiles), Fin // _K1_SLAB)) if tiles < 256 else 1
            ws = torch.empty(lib.pygat_gemm_workspace_bytes(L.N, ncols, split_k) // 4, dtype=f32, device=dev) if split_k > 1 else None
            with _span("k1_project"):
                check(lib.pygat_project_blocked(L.N, Fin, H, Fo, x.data_ptr(), L.ldx, None, Wcat.data_ptr(), L.ldw, a_pad.data_ptr(),
                                                Wh.data_ptr(), _ptr(Sk), s.data_ptr(), split_k, _ptr(ws), GEMM_MODES[L.mode], st),
                      "project")
            Whq = torch.empty(L.N, L.R, dtype=torch.int16, device=dev)      # bf16 bit patterns
            with _span("k16_pack"):
                check(lib.pygat_gat_pack_bf16(L.N, H, Fo, Wh.data_ptr(), L.R, a_pad.data_ptr(), Whq.data_ptr(), s.data_ptr(), st),
                      "gat_pack_bf16")      # (s: K1's scores are replaced by the ones of the rounded rows)
            single = (not concat) and H == 1      # a mean over one head is that head: the forward writes `out` itself
            hattn = torch.empty(L.N, L.R, dtype=f32, device=dev) if not (concat or single) else None
            out = torch.empty(L.N, H * Fo if concat else Fo, dtype=f32, device=dev)
            part = torch.empty(_lib.bf16_workspace_bytes(graph.nnz, L.ts, H, Fo) // 4, dtype=f32, device=dev)
            with _span("k16_forward"):
                check(lib.pygat_gat_forward_bf16(graph.fwd.ref(L.ts), H, Fo, float(alpha), flags, Whq.data_ptr(), s.data_ptr(),
                                                 a_pad.data_ptr(), _ptr(Sk), out.data_ptr() if (concat or single) else None, _ptr(hattn),
                                                 0, part.data_ptr(), st), "gat_forward_bf16")
            if hattn is not None:
                check(lib.pygat_head_mean(L.N, H, Fo, hattn.data_ptr(), _ptr(Sk), out.data_ptr(), st), "head_mean")
    return out


def no_table_dtype(table_dtype, what: str) -> None:
    """The entry points the bf16 feature table (gat_level(..., table_dtype=torch.bfloat16), csrc/k16_bf16_forward.hip) does not cover."""
    if table_dtype is not None:
        raise ValueError(f"pygat_amd: {what} does not take table_dtype: the bf16 feature table covers the inference forward of the "
                         "plain GAT (v1) level (ops.gat_level) only")


PAD_K = _config.pad_k     # development knob: 0 = run odd input widths as they are
MAX_HEAD_TABLE = _lib.MAX_HEADS_TABLE     # heads whose parameter pointers travel as kernel arguments


class GATLevelHeadsFn(torch.autograd.Function):
    """The same level with its parameters given as they live in the model -- one W [Fin,F'], a (2F' values) and
    skip_projection [Fin,F'] tensor PER HEAD (layers.py:21-28,111-119; models.py:15-27) -- instead of stacked: the packing
    kernel reads them through a pointer table (pygat_pack_params_heads), so no torch.stack (a cat launch per parameter
    kind, level and forward: a tenth of a small graph's epoch) precedes the level.
    forward(x, graph, alpha, concat, pipeline, H, skip, xs, att, *Ws, *As[, *Wskips]) -> out (att: see AttentionTarget;
    an att with grad=True: -> (out, alpha), both differentiable)."""

    @staticmethod
    def forward(ctx, x, graph: CSRGraph, alpha: float, concat: bool, pipeline, H: int, skip: bool, xs, att, *params):
        if not x.is_cuda:
            raise RuntimeError("pygat_amd: inputs must be on the GPU; the hot path has no CPU fallback")
        Ws, As = params[:H], params[H:2 * H]
        Ss = params[2 * H:3 * H] if skip else ()
        Fin, Fo = Ws[0].shape
        ctx.in_dtype_x = x.dtype
        ctx.param_shapes = [tuple(p.shape) for p in params]
        ctx.param_dtypes = [p.dtype for p in params]
        x = x.contiguous().float()
        Ws = [w.contiguous().float() for w in Ws]; As = [v.contiguous().float() for v in As]; Ss = [w.contiguous().float() for w in Ss]
        if _in_features(x) != Fin or any(w.shape != (Fin, Fo) for w in Ws) or any(v.numel() != 2 * Fo for v in As):
            raise ValueError(f"shape mismatch: x {tuple(x.shape)}, W {tuple(Ws[0].shape)}, a {tuple(As[0].shape)}")
        PT = C.c_void_p * H
        wp, ap = PT(*[w.data_ptr() for w in Ws]), PT(*[v.data_ptr() for v in As])
        sp = PT(*[w.data_ptr() for w in Ss]) if skip else None

        def pack(Wcat, ldw, a_pad, st):
            check(lib.pygat_pack_params_heads(H, Fin, Fo, wp, ap, sp, Wcat.data_ptr(), ldw, a_pad.data_ptr(), st), "pack_params_heads")
        n = ctx.needs_input_grad
        need = (n[0], any(n[9:9 + H]), any(n[9 + H:9 + 2 * H]), skip and any(n[9 + 2 * H:9 + 3 * H]))
        ctx.H, ctx.skip = H, skip
        return _level_forward(ctx, need, x, H, Fo, skip, pack, graph, alpha, concat, None, pipeline, xs=xs, att=att)

    @staticmethod
    def backward(ctx, G, A=None):
        dx, dW, da, dWs = _level_backward(ctx, G, A)
        H = ctx.H
        if dx is not None and dx.dtype != ctx.in_dtype_x:
            dx = dx.to(ctx.in_dtype_x)
        outs = []
        for k in range(H):
            outs.append(None if dW is None else dW[k])
        for k in range(H):
            outs.append(None if da is None else da[k].reshape(ctx.param_shapes[H + k]))
        if ctx.skip:
            for k in range(H):
                outs.append(None if dWs is None else dWs[k])
        outs = [g_ if g_ is None or g_.dtype == dt else g_.to(dt) for g_, dt in zip(outs, ctx.param_dtypes)]
        return (dx, None, None, None, None, None, None, None, None) + tuple(outs)


def _level_forward(ctx, need, x, H, Fo, skip, pack, graph: CSRGraph, alpha: float, concat: bool, bwd_heads, pipeline, xs=None,
                   att=None):
    """Body of the level's forward, shared by GATLevelFn (stacked parameters) and GATLevelHeadsFn (one tensor per head).
    need = (x, W, a, Wskip) gradient flags; pack(Wcat, ldw, a_pad, stream) launches the parameter packing; xs: the
    SparseFeatures of x (features.py) -- projection and weight gradient on the non-zeros only -- or None.  att: an
    AttentionTarget the forward fills with the level's attention coefficients, or None."""
    if att is not None and pipeline is not None:
        raise ValueError("pygat_amd: return_attention does not take a pipeline")
    if att is not None and att.grad and bwd_heads is not None:
        raise ValueError("pygat_amd: return_attention=\"grad\" does not take a backward over a head range (head_parallel)")
    if x.dim() == 3 and not blocked_input_ok(x):
        raise ValueError(f"column-blocked input {tuple(x.shape)}: blocks must be a power of two >= 16 floats wide (float32, GPU)")
    L = _Level(x, H, Fo, skip)
    Fin = L.Fin
    if L.N != graph.n:
        raise ValueError(f"x has {L.N} rows but the graph has {graph.n} nodes")
    if L.blocks is not None:
        xs = None
    # a degree-ordered graph handed in directly (CSRGraph.degree_ordered: x in internal order) carries its row map: `out` is
    # written, G and the saved output are read at the caller's rows -- by every kernel of the level, the tail's included
    user_row = graph.user_row
    single_out = (not concat) and H == 1
    if user_row is not None and (pipeline is not None or not (concat or single_out)):
        raise ValueError("pygat_amd: a graph with a row map (CSRGraph.degree_ordered) takes neither a pipeline nor a mean over "
                         "several heads; pass CSRGraph.internal_view() and keep x and `out` in internal order instead")
    tail = None      # (first tail row, pygat_graph* of the slot prefix) when the self-loop-only tail goes through its own streams
    if (RENUMBER and not need[0] and xs is None and pipeline is None and x.dim() == 2 and (concat or single_out)
            and graph.user_row is None and not graph.degree_sorted and L.N * L.R * 4 >= min(RENUMBER_MIN_BYTES, RENUMBER_MIN_BYTES_TAIL)
            and not torch.cuda.is_current_stream_capturing()):     # (a captured graph would bake this epoch's permuted copy of x in)
        from .features import permuted_rows
        g_int, to_user, to_int = graph.degree_ordered()
        worth = L.N * L.R * 4 >= RENUMBER_MIN_BYTES
        if not worth and TAIL and concat and graph.symmetric:     # a narrower table: only with a self-loop-only tail to stream
            t = g_int.fwd.self_loop_tail(slot_edges_for(L.R, g_int.slot_edges))
            worth = t is not None and L.N - t[0] >= TAIL_MIN_SHARE * L.N
        xp = permuted_rows(x, to_user) if worth else None
        if xp is not None:
            x, graph, user_row = xp, g_int, to_user
            if att is not None:
                att.renumbered(to_int)
    L.ts = slot_edges_for(L.R, graph.slot_edges)
    L.mode = get_gemm_mode()     # this thread's product mode, fixed for the level: its backward (another thread) uses it too
    dev, f32 = x.device, torch.float32
    need_grad = any(need)
    ctx.need = need
    with torch.cuda.device(dev):
        st = _stream()
        Wcat = torch.empty(Fin, L.ldw, dtype=f32, device=dev)
        a_pad = torch.empty(H, 2, L.Fp, dtype=f32, device=dev)
        pack(Wcat, L.ldw, a_pad, st)
        # K1: [Wh | Sk | s | t] = x @ Wcat
        Wh = torch.empty(L.N, L.R, dtype=f32, device=dev)
        Sk = torch.empty(L.N, L.R, dtype=f32, device=dev) if skip else None
        s = torch.empty(L.N, H, dtype=f32, device=dev)
        ncols = L.R * (2 if skip else 1) + H
        tiles = -(-L.N // 128) * -(-ncols // 128)
        # few row tiles (Cora: 22): K slabs of >= 128 until ~1.5 work-groups per CU (PYGAT_K1_SPLIT_MIN_K: slab floor)
        split_k = max(1, min(-(-384 // tiles), Fin // _K1_SLAB)) if tiles < 256 else 1
        ws = torch.empty(lib.pygat_gemm_workspace_bytes(L.N, ncols, split_k) // 4, dtype=f32, device=dev) \
            if split_k > 1 else None
        if xs is not None and need[0]:
            xs = None                                   # a gradient into x: the dense path forms it
        flags = (_lib.F_ELU if concat else 0) | (_lib.F_SKIP if skip else 0)
        flavour = backward_flavour(L.R) if need_grad else None
        # (a degree-ordered pattern: reached through the renumbering above -- user_row maps `out` / G to the caller's rows -- or
        # handed in by a model that keeps ALL its node arrays in internal order, graph.InternalOrderView: no map)
        if (TAIL and graph.degree_sorted and concat and graph.symmetric
                and (not need_grad or (flavour == "rowlocal" and L.hg >= H and bwd_heads is None))):
            t = graph.fwd.self_loop_tail(L.ts)
            if t is not None and L.N - t[0] >= TAIL_MIN_SHARE * L.N:
                tail = (t[0], t[2], t[1])
        out = pipeline[2] if (pipeline is not None and len(pipeline) > 2 and concat) else None    # the caller's buffer (dist.py:
        if out is not None:                                                                           # the rank's block of the exchange)
            if tuple(out.shape) != (L.N, H * Fo) or out.dtype != f32 or not out.is_contiguous() or out.device != dev:
                raise ValueError(f"pipeline output buffer {tuple(out.shape)}: expected a contiguous float32 [{L.N}, {H * Fo}] on {dev}")
            # the buffer is the rank's block of a larger tensor whose OTHER blocks are received in place afterwards: alias its
            # memory with a tensor of its own (no view relation, own version counter), or autograd takes the peers' writes for
            # in-place changes of this output
            out = torch.empty(0, dtype=f32, device=dev).set_(out.untyped_storage(), out.storage_offset(), out.shape, out.stride())
        else:
            out = torch.empty(L.N, H * Fo if concat else Fo, dtype=f32, device=dev)
        # the tail's output straight from the projection's epilogue (TAIL_FUSED): its Wh rows are then never written, so
        # nothing may read them -- with a backward, the a-gradient has to come from the column pass (its fold reads the prefix)
        fuse_fwd = (TAIL_FUSED and tail is not None and not skip and L.Fo == L.Fp and xs is None and x.dim() == 2
                    and L.mode == "split-bf16"
                    and (not need_grad or (DA_IN_K4 and need[2] and L.N * L.R * 4 >= DA_MIN_BYTES
                                           and lib.pygat_gat_backward_col_da_bytes(tail[1], H, Fo, H) > 0)))
        with _span("k1_project"):
            if xs is not None:
                check(lib.pygat_project_sparse(L.N, Fin, H, Fo, xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(),
                                               Wcat.data_ptr(), L.ldw, 0.0, None, 0, None, Wh.data_ptr(), _ptr(Sk), s.data_ptr(),
                                               st), "project_sparse")
            elif fuse_fwd:
                check(lib.pygat_project_tail_blocked(L.N, Fin, H, Fo, x.data_ptr(), L.ldx, L.xb(), Wcat.data_ptr(), L.ldw,
                                                     a_pad.data_ptr(), Wh.data_ptr(), s.data_ptr(), split_k, _ptr(ws),
                                                     GEMM_MODES[L.mode], tail[0], _ptr(user_row), out.data_ptr(), flags, st),
                      "project_tail")
            else:
                check(lib.pygat_project_blocked(L.N, Fin, H, Fo, x.data_ptr(), L.ldx, L.xb(), Wcat.data_ptr(), L.ldw, a_pad.data_ptr(),
                                                Wh.data_ptr(), _ptr(Sk), s.data_ptr(), split_k, _ptr(ws), GEMM_MODES[L.mode], st),
                      "project")
        # K2
        # mean over ONE head = that head (Cora / Citeseer output level, train.py:55,66): K2 writes `out` itself (its epilogue
        # adds the skip rows, no ELU), no head-mean launch; hattn is then only kept for the backward
        single = (not concat) and H == 1
        hattn = torch.empty(L.N, L.R, dtype=f32, device=dev) if (not concat and (need_grad or not single)) else None
        # (K2 picks its instantiation by aneg, not by m: asking for the attention changes no output bit)
        m = torch.empty(L.N, H, dtype=f32, device=dev) if (need_grad or att is not None) else None
        Z = torch.empty(L.N, H, dtype=f32, device=dev) if (need_grad or att is not None) else None
        aneg = torch.empty(L.N, L.R, dtype=f32, device=dev) if flavour == "rowlocal" else None
        qneg = torch.empty(L.N, H, dtype=f32, device=dev) if flavour == "rowlocal" else None
        part = torch.empty(lib.pygat_partials_bytes(graph.nnz, L.ts, H, L.Fp) // 4, dtype=f32,
                           device=dev)
        # (fuse_fwd: the tail's rows of m, Z and qneg stay unwritten -- nothing reads them.  K3a runs on the rows before the
        # tail (no skip projection: fused_tail in the backward), K4 and its fix-up take m / Z from the GR rows of the prefix
        # nodes they gather, the a-gradient fold reads Wh / ds / dt of cut rows, and K13 / K14 skip rows of one edge.)
        chunks = [(graph.fwd.ref(L.ts) if tail is None else tail[1], 0, L.N if tail is None else tail[0])]
        if pipeline is not None and concat and pipeline[0] > 1:
            chunks = (graph.fwd.row_chunks(int(pipeline[0]), L.ts) if tail is None
                      else graph.fwd.row_chunks(int(pipeline[0]), L.ts, nslots=tail[2], row_end=tail[0]))
        # a pipelined level: chunk c's fix-up launch (a few thousand cut rows, latency-bound: 25-30 us at config 5) and the
        # caller's hand-off of the chunk run on a SIDE stream beside chunk c + 1's main launch (the partial records are per
        # slot: chunks share none) -- in line they cost the step ~70 us per chunk border
        phases = len(chunks) > 1 and TIMER is None and bool(lib.pygat_gat_forward_phases_ok(L.N, H, Fo))
        if phases:
            main_s, side_s = torch.cuda.current_stream(dev), _side_stream(dev)

        def k2(gref, fl, stream):
            check(lib.pygat_gat_forward(gref, H, Fo, float(alpha), fl, Wh.data_ptr(), s.data_ptr(),
                                        a_pad.data_ptr(), _ptr(Sk), None, out.data_ptr() if (concat or single) else None,
                                        _ptr(hattn), _ptr(m), _ptr(Z), _ptr(aneg), _ptr(qneg), part.data_ptr(), stream),
                  "gat_forward")
        for c, (gref, r0, r1) in enumerate(chunks):
            if phases:
                k2(gref, flags | _lib.F_MAIN_ONLY, st)
                side_s.wait_stream(main_s)
                with torch.cuda.stream(side_s):
                    k2(gref, flags | _lib.F_FIXUP_ONLY, side_s.cuda_stream)
                    pipeline[1](c, r0, r1, out)        # (a collective issued here waits for the side stream = for this chunk only)
                continue
            with _span("k2_forward"):
                k2(gref, flags, st)
                if tail is not None and c == len(chunks) - 1 and not fuse_fwd:   # the self-loop-only rows: out = ELU(Wh (+ skip))
                    check(lib.pygat_gat_forward_tail(tail[0], L.N - tail[0], H, Fo, flags, Wh.data_ptr(), 0, _ptr(Sk), out.data_ptr(),
                                                     _ptr(user_row), _ptr(m), _ptr(Z), _ptr(qneg), st), "gat_forward_tail")
            if pipeline is not None and concat:
                pipeline[1](c, r0, r1 if not (tail is not None and c == len(chunks) - 1) else L.N, out)
        if phases:
            main_s.wait_stream(side_s)
            if tail is not None:       # (pipelined chunks: the tail is one more hand-off, after the last chunk's)
                if not fuse_fwd:
                    check(lib.pygat_gat_forward_tail(tail[0], L.N - tail[0], H, Fo, flags, Wh.data_ptr(), 0, _ptr(Sk), out.data_ptr(),
                                                     _ptr(user_row), _ptr(m), _ptr(Z), _ptr(qneg), st), "gat_forward_tail")
                pipeline[1](len(chunks), tail[0], L.N, out)
        if att is not None:      # (the tail's rows have one edge each: alpha = 1, their t, Wh, m, Z rows are not read)
            with _span("k13_attention"):
                att.launch_v1(H, Fo, alpha, Wh, L.R, s, a_pad, m, Z, L.N if tail is None else tail[0], st)
        if not concat and not single:
            check(lib.pygat_head_mean(L.N, H, Fo, hattn.data_ptr(), _ptr(Sk), out.data_ptr(), st), "head_mean")
    if need_grad:
        # concat: the backward recovers hattn from `out` (no second [N,R] table is written)
        ctx.save_for_backward(x, Wcat, a_pad, Wh, s, Sk, out if concat else hattn, m, Z, aneg, qneg)
        ctx.graph, ctx.L, ctx.alpha, ctx.concat, ctx.flags = graph, L, float(alpha), concat, flags
        ctx.user_row = user_row
        ctx.tail = tail
        ctx.tail_fwd_fused = fuse_fwd
        ctx.xs = xs
        ctx.flavour = flavour
        ctx.bwd_heads = None
        if bwd_heads is not None:
            hb, hr = int(bwd_heads[0]), int(bwd_heads[1])
            if not (0 <= hb and 0 < hr and hb + hr <= H):
                raise ValueError(f"bwd_heads {bwd_heads} outside the {H} heads of the level")
            if skip or need[0]:
                raise ValueError("pygat_amd: bwd_heads supports neither a skip projection nor a gradient into x")
            ctx.bwd_heads = (hb, hr)
    if att is not None and att.grad:
        # alpha is a second output of the node: an absent gradient stays None (a loss on `out` alone launches nothing new)
        ctx.set_materialize_grads(False)
        if need_grad:
            ctx.att_bwd, ctx.out_shape = att.backward_state(), tuple(out.shape)
        return out, att.alpha
    return out

def _level_backward(ctx, G, A=None):
    """Body of the level's backward: -> (dx | None, dW [H,Fin,F'] | None, da [H,2F'] | None, dWskip | None).
    A: dL/d alpha [E, H] of a level that returned its coefficients as a differentiable output (return_attention="grad"), or None."""
    x, Wcat, a_pad, Wh, s, Sk, y, m, Z, aneg, qneg = ctx.saved_tensors
    graph, L, H, Fo = ctx.graph, ctx.L, ctx.L.H, ctx.L.Fo
    dev, f32 = x.device, torch.float32
    if G is None:        # (only a level in "grad" mode sees this: the loss reaches it through alpha alone)
        G = torch.zeros(ctx.out_shape, dtype=f32, device=dev)
    G = G.contiguous().float()
    ranged = ctx.bwd_heads is not None
    hb, hr = ctx.bwd_heads if ranged else (0, 0)       # (0, 0) = all heads in the C ABI
    Hb = hr if ranged else H                            # heads this backward covers
    with torch.cuda.device(dev):
        st = _stream()
        RW = Hb * (L.Fp + 4)                            # GR is compact for the covered heads
        GR = torch.empty(L.N, RW, dtype=f32, device=dev)      # per head window: [Gp | (s, m, 1/Z, D) per head]
        ds = torch.empty(L.N, H, dtype=f32, device=dev)
        dt = torch.empty(L.N, H, dtype=f32, device=dev)
        dWh = torch.empty(L.N, L.R, dtype=f32, device=dev)
        part = torch.empty(lib.pygat_partials_bytes(graph.nnz, L.ts, H, L.Fp) // 4, dtype=f32,
                           device=dev)
        rowlocal = ctx.flavour == "rowlocal"
        # heads per window: the level's choice for all its heads, or the library default for the range a ranged backward covers
        hgw = lib.pygat_head_group(L.N, Hb, Fo) if (ranged and BWD_WINDOW_FLOATS is None) else (min(L.hg, Hb) if not ranged else head_group(L.N, Hb, Fo))
        # (symmetric pattern with a self-loop-only tail in internal order: the column pass and its fold run on the slot prefix)
        tail = getattr(ctx, "tail", None)
        gT = graph.bwd.ref(L.ts) if tail is None else tail[1]
        # da along with the column pass (no separate stream over Wh, ds, dt), when the pass can and the table is large
        da_part = None
        if DA_IN_K4 and not ranged and ctx.flavour != "rowsum" and ctx.need[2] and L.N * L.R * 4 >= DA_MIN_BYTES:
            nb = lib.pygat_gat_backward_col_da_bytes(gT, H, Fo, hgw)
            if nb:
                da_part = torch.empty(nb // 4, dtype=f32, device=dev)
        # no skip projection: nothing but the column pass reads the tail's Gp -- its whole backward is one stream from G / out
        # (pygat_gat_backward_tail) and K3a runs on the rows before it
        fused_tail = tail is not None and not L.skip
        with _span("k3a_prepare"):
            check(lib.pygat_gat_backward_prepare(tail[0] if fused_tail else L.N, H, Fo, ctx.flags, 0 if ctx.concat else 1, G.data_ptr(),
                                                 y.data_ptr(), _ptr(Sk), s.data_ptr(), m.data_ptr(), Z.data_ptr(),
                                                 GR.data_ptr(), _ptr(aneg), _ptr(qneg), ctx.alpha,
                                                 ds.data_ptr() if rowlocal else None, hb, hr, hgw, _ptr(getattr(ctx, "user_row", None)), st),
                      "gat_backward_prepare")
        two_gather = ctx.flavour == "two-gather"
        # no tail stream at all (TAIL_WGRAD_MIN_BYTES): the weight gradient forms the tail's dWh rows itself, where it is the
        # only reader of the tail's dWh, ds and dt rows -- no input gradient, da folded in the column pass (cut rows only, all
        # before the tail), dense x, no loss through alpha
        tail_wgrad = (rowlocal and fused_tail and not ranged and L.N * L.R * 4 >= TAIL_WGRAD_MIN_BYTES and ctx.need[1]
                      and not ctx.need[0] and da_part is not None and A is None and getattr(ctx, "xs", None) is None)
        # the tail's stream in the launch of the column pass's fix-up (COL_FINISH_MIN_BYTES)
        col_finish = (rowlocal and fused_tail and not ranged and not tail_wgrad and L.N * L.R * 4 >= COL_FINISH_MIN_BYTES
                      and lib.pygat_gat_backward_col_phases_ok(gT, H, Fo, hgw) == 1)
        if col_finish:
            with _span("k4_backward_col"):
                check(lib.pygat_gat_backward_col_phase(gT, None, H, Fo, ctx.alpha, Wh.data_ptr(),
                                                       a_pad.data_ptr(), GR.data_ptr(), None, ds.data_ptr(),
                                                       dWh.data_ptr(), dt.data_ptr(), None, part.data_ptr(), _ptr(da_part), hb, hr, hgw,
                                                       _lib.F_MAIN_ONLY, st), "gat_backward_col_phase")
                check(lib.pygat_gat_backward_col_finish(gT, H, Fo, a_pad.data_ptr(), ds.data_ptr(), dWh.data_ptr(), dt.data_ptr(),
                                                        part.data_ptr(), hgw, tail[0], L.N - tail[0], ctx.flags, G.data_ptr(),
                                                        y.data_ptr(), _ptr(getattr(ctx, "user_row", None)), st),
                      "gat_backward_col_finish")
        elif rowlocal:        # ds is known: the column pass finishes dWh on its own
            with _span("k4_backward_col"):
                check(lib.pygat_gat_backward_col(gT, None, H, Fo, ctx.alpha, Wh.data_ptr(),
                                                 a_pad.data_ptr(), GR.data_ptr(), None, ds.data_ptr(),
                                                 dWh.data_ptr(), dt.data_ptr(), None, part.data_ptr(), _ptr(da_part), hb, hr, hgw, st),
                      "gat_backward_col")
                if tail_wgrad:           # the self-loop-only rows: formed inside the weight gradient (pygat_wgrad_tail_blocked)
                    pass
                elif fused_tail:         # ... dWh_j = G_u ELU'(out_u), ds_j = dt_j = 0 (csrc/k12_tail.hip)
                    check(lib.pygat_gat_backward_tail(tail[0], L.N - tail[0], H, Fo, ctx.flags, G.data_ptr(), y.data_ptr(),
                                                      _ptr(getattr(ctx, "user_row", None)), dWh.data_ptr(), 0, 0, ds.data_ptr(), dt.data_ptr(), st),
                          "gat_backward_tail")
                elif tail is not None:   # ... with a skip projection (its weight gradient reads every row's Gp): dWh_j = Gp_j, dt_j = 0
                    check(lib.pygat_gat_backward_col_tail(tail[0], L.N - tail[0], H, Fo, GR.data_ptr(), dWh.data_ptr(), dt.data_ptr(), st),
                          "gat_backward_col_tail")
        elif two_gather:
            with _span("k3b_row"):
                check(lib.pygat_gat_backward_row(graph.fwd.ref(L.ts), H, Fo, ctx.alpha, Wh.data_ptr(),
                                                 a_pad.data_ptr(), GR.data_ptr(), None, ds.data_ptr(),
                                                 part.data_ptr(), hb, hr, hgw, st), "gat_backward_row")
            with _span("k4_backward_col"):
                check(lib.pygat_gat_backward_col(graph.bwd.ref(L.ts), None, H, Fo, ctx.alpha, Wh.data_ptr(),
                                                 a_pad.data_ptr(), GR.data_ptr(), None, ds.data_ptr(),
                                                 dWh.data_ptr(), dt.data_ptr(), None, part.data_ptr(), _ptr(da_part), hb, hr, hgw, st),
                      "gat_backward_col")
        else:
            dz_t = torch.empty(graph.nnz, H, dtype=f32, device=dev)
            with _span("k4_backward_col"):
                check(lib.pygat_gat_backward_col(graph.bwd.ref(L.ts), None, H, Fo, ctx.alpha, Wh.data_ptr(),
                                                 a_pad.data_ptr(), GR.data_ptr(), None, None,
                                                 dWh.data_ptr(), dt.data_ptr(), dz_t.data_ptr(), part.data_ptr(), None, hb, hr, hgw, st),
                      "gat_backward_col")
            with _span("k3c_rowsum"):
                check(lib.pygat_gat_backward_rowsum(graph.fwd.ref(L.ts), graph.perm_f.data_ptr(), H, Fo,
                                                    dz_t.data_ptr(), ds.data_ptr(), part.data_ptr(), hb, hr, st),
                      "gat_backward_rowsum")
        # da; after the row-sum flavour the same stream also finishes dWh_i += ds_i a_src
        da = (torch.zeros if ranged else torch.empty)(H, 2 * Fo, dtype=f32, device=dev)
        ws = torch.empty(lib.pygat_agrad_workspace_bytes(H, Fo) // 4, dtype=f32, device=dev)
        # ... unless nothing but the weight-gradient GEMM consumes dWh: there ds rides along as extra columns
        # (pygat_wgrad) and dWh is never rewritten
        rowsum = ctx.flavour == "rowsum"
        xs = getattr(ctx, "xs", None)
        sparse_w = xs is not None and not ranged and (not L.skip or L.hg >= H)    # weight gradients on the non-zeros of x
        fold_ds = (rowsum and ctx.need[1] and not ctx.need[0] and not sparse_w
                   and (Hb * L.Fp) % 32 == 0 and L.N >= 4096)   # the streamed-K GEMM takes [dWh | ds] in one pass
        finish = rowsum and not fold_ds
        # when a_grad does not rewrite dWh, nothing downstream depends on it: run it on the side stream,
        # beside the weight-gradient GEMM (TIMER spans stay on the main stream: no fork while timing kernels)
        fork = OVERLAP_BACKWARD and not finish and TIMER is None and ctx.need[1] and A is None
        if fork:
            main, side = torch.cuda.current_stream(), _side_stream(dev)
            side.wait_stream(main)      # the tensors it touches stay referenced until the join below
        if da_part is not None:      # the column pass left one record per work-group: fold them (and the cut rows) in a fixed order
            with _span("k5_afold"):
                check(lib.pygat_a_grad_fold(gT, H, Fo, Wh.data_ptr(), ds.data_ptr(), dt.data_ptr(),
                                            da_part.data_ptr(), da.data_ptr(), ws.data_ptr(), hgw,
                                            side.cuda_stream if fork else st), "a_grad_fold")
        else:
            with _span("k5_agrad"):
                check(lib.pygat_a_grad(L.N, H, Fo, Wh.data_ptr(), ds.data_ptr(), dt.data_ptr(), da.data_ptr(),
                                       ws.data_ptr(), a_pad.data_ptr() if finish else None,
                                       dWh.data_ptr() if finish else None, None, hb, hr,
                                       side.cuda_stream if fork else st), "a_grad")
        if A is not None:
            # the loss through alpha: (ds', dt') from the row and column passes of K14; their rank-one terms go into dWh and da
            # here, before the weight and input gradients consume them -- everything above is as for a loss on `out` alone.  The
            # self-loop-only tail contributes nothing (alpha = 1) and its Wh rows may be unwritten: the rows before it only.
            live = L.N if tail is None else tail[0]
            ds2, dt2 = ctx.att_bwd.scores(A, s, m, Z, ctx.alpha, st)
            with _span("k14_alpha_apply"):
                check(lib.pygat_alpha_grad_apply(live, H, Fo, a_pad.data_ptr(), ds2.data_ptr(), dt2.data_ptr(), dWh.data_ptr(), st),
                      "alpha_grad_apply")
                if ctx.need[2]:
                    da2 = torch.empty(H, 2 * Fo, dtype=f32, device=dev)
                    ws2 = torch.empty_like(ws)
                    check(lib.pygat_a_grad(live, H, Fo, Wh.data_ptr(), ds2.data_ptr(), dt2.data_ptr(), da2.data_ptr(), ws2.data_ptr(),
                                           None, None, None, 0, 0, st), "a_grad")
                    da += da2
        # dW = x^T dWh (split-K over the nodes), dWskip = x^T Gp
        dW = dWs = dx = None
        if sparse_w and (ctx.need[1] or (L.skip and ctx.need[3])):
            dW = torch.empty(H, L.Fin, Fo, dtype=f32, device=dev)
            want_s = L.skip and ctx.need[3]
            dWs = torch.empty(H, L.Fin, Fo, dtype=f32, device=dev) if want_s else None
            wss = torch.empty(lib.pygat_wgrad_sparse_workspace_bytes(xs.nseg, H, Fo, int(want_s)) // 4 + 4, dtype=f32, device=dev)
            with _span("k5_wgrad"):
                check(lib.pygat_wgrad_sparse(L.N, L.Fin, H, Fo, xs.nseg, xs.colseg.data_ptr(), xs.seg_col.data_ptr(),
                                             xs.seg_begin.data_ptr(), xs.seg_end.data_ptr(), xs.trow.data_ptr(), xs.tval.data_ptr(),
                                             0.0, None, 0, None, dWh.data_ptr(), GR.data_ptr() if want_s else None, RW,
                                             wss.data_ptr(), dW.data_ptr(), _ptr(dWs), st), "wgrad_sparse")
        elif ctx.need[1]:
            split_k = _split_k(L.Fin, Hb * L.Fp + (Hb if fold_ds else 0), L.N, streamed_k=True, mode=L.mode)
            wsw = torch.empty(lib.pygat_wgrad_workspace_bytes(L.Fin, H, Fo, split_k) // 4, dtype=f32, device=dev)
            dW = (torch.zeros if ranged else torch.empty)(H, L.Fin, Fo, dtype=f32, device=dev)
            with _span("k5_wgrad"):
                if tail_wgrad:
                    rc = lib.pygat_wgrad_tail_blocked(L.N, L.Fin, H, Fo, x.data_ptr(), L.ldx, L.xb(), dWh.data_ptr(), dW.data_ptr(),
                                                      split_k, wsw.data_ptr(), tail[0], ctx.flags, G.data_ptr(), y.data_ptr(),
                                                      _ptr(getattr(ctx, "user_row", None)), GEMM_MODES[L.mode], st)
                    if rc == 1:          # not taken (product mode, blocked x, F' != Fp, ...): the stream after all, then the plain GEMM
                        check(lib.pygat_gat_backward_tail(tail[0], L.N - tail[0], H, Fo, ctx.flags, G.data_ptr(), y.data_ptr(),
                                                          _ptr(getattr(ctx, "user_row", None)), dWh.data_ptr(), 0, 0, ds.data_ptr(), dt.data_ptr(), st),
                              "gat_backward_tail")
                    else:
                        check(rc, "wgrad_tail")
                if not tail_wgrad or rc == 1:
                    check(lib.pygat_wgrad_blocked(L.N, L.Fin, H, Fo, x.data_ptr(), L.ldx, L.xb(), dWh.data_ptr(),
                                                  ds.data_ptr() if fold_ds else None, a_pad.data_ptr(), dW.data_ptr(), split_k,
                                                  wsw.data_ptr(), hb, hr, GEMM_MODES[L.mode], st), "wgrad")
        if L.skip and ctx.need[3] and not sparse_w:
            dSc = torch.empty(L.Fin, L.R, dtype=f32, device=dev)
            for c0, w, g0 in L.gp_windows():
                gemm(True, False, L.Fin, w, L.N, x, L.ldx, GR[:, g0:], RW, [(w, dSc[:, c0:], L.R)], mode=L.mode, a_blocks=L.blocks)
            dWs = torch.empty(H, L.Fin, Fo, dtype=f32, device=dev)
            check(lib.pygat_unpack_wgrad(H, L.Fin, Fo, dSc.data_ptr(), L.R, 0, dWs.data_ptr(), st), "unpack")
        # dx = dWh Wcat[:, :R]^T (+ Gp Wcat[:, R:2R]^T)
        if ctx.need[0]:
            # (a column-blocked x: its gradient is written in the same blocks -- what the reduce-scatter of the exchange sends)
            dx = torch.empty(x.shape, dtype=f32, device=dev)
            with _span("k5_xgrad"):
                gemm(False, True, L.N, L.Fin, L.R, dWh, L.R, Wcat, L.ldw, [(L.Fin, dx, L.ldx)], mode=L.mode, c_blocks=L.blocks)
                if L.skip:
                    for c0, w, g0 in L.gp_windows():
                        gemm(False, True, L.N, L.Fin, w, GR[:, g0:], RW, Wcat[:, L.R + c0:], L.ldw,
                             [(L.Fin, dx, L.ldx)], accumulate=True, split_k=1, mode=L.mode, c_blocks=L.blocks)
        if fork:
            main.wait_stream(side)
    return dx, dW, (da if ctx.need[2] else None), dWs


class AttentionTarget:
    """Where a level writes its attention coefficients (return_attention): alpha [E, H] float32, not differentiable, row k =
    edge k of the CALLER's pattern (graph.fwd: rowptr, edge_rc).
    grad=True (return_attention="grad"): the level returns alpha as a second, differentiable output.  The target then keeps `t`,
    the pattern and the node map for the level's backward (AlphaGradState); at most MAX_GRAD_HEADS heads.  The level's tables may be in another node order: `to_internal`
    (caller node -> table row) is set when the level renumbers by itself (ops._level_forward, GATv2LevelFn), or given as
    order = (caller graph, to_internal) by a caller that hands the level an InternalOrderView of its graph (GAT.forward)."""

    MAX_GRAD_HEADS = 64      # csrc/k14_alpha_grad.hip: a wave's lanes cover the heads

    def __init__(self, graph, H: int, device, order=None, grad: bool = False):
        if grad and H > self.MAX_GRAD_HEADS:
            raise ValueError(f"pygat_amd: return_attention=\"grad\" takes at most {self.MAX_GRAD_HEADS} heads per level, not {H}; "
                             "return_attention=True gives the detached coefficients")
        g, self.to_internal = (graph, None) if order is None else order
        self.pattern = g.fwd
        self.grad, self.t, self._graph = bool(grad), None, g
        self.alpha = torch.empty(g.nnz, H, dtype=torch.float32, device=device)
        if self.pattern.n != graph.n or g.nnz != graph.nnz:
            raise ValueError(f"pygat_amd: attention_order: a graph of {self.pattern.n} nodes / {g.nnz} edges for a level on "
                             f"{graph.n} / {graph.nnz}")

    def renumbered(self, to_internal: torch.Tensor) -> None:
        self.to_internal = to_internal

    def _pattern_args(self):
        p = self.pattern
        return (p.n, p.nnz, p.rowptr.data_ptr(), p.edge_rc.data_ptr(), _ptr(self.to_internal))

    def launch_v1(self, H, Fo, slope, Wh, ldwh, s, a_pad, m, Z, t_rows, st):
        t = torch.empty(self.pattern.n, H, dtype=torch.float32, device=Wh.device)      # t_q = Wh_q . a_dst, rows < t_rows
        check(lib.pygat_gat_attention(*self._pattern_args(), H, Fo, float(slope), Wh.data_ptr(), ldwh, s.data_ptr(),
                                      a_pad.data_ptr(), m.data_ptr(), Z.data_ptr(), int(t_rows), t.data_ptr(),
                                      self.alpha.data_ptr(), st), "gat_attention")
        if self.grad:
            self.t, self.Fo = t, int(Fo)

    def backward_state(self) -> "AlphaGradState":
        """What the backward of a "grad" level needs (NOT alpha itself: the node's own output would keep the node alive)."""
        if self.t is None:
            raise ValueError("pygat_amd: return_attention=\"grad\" covers the GAT (v1) level only")
        return AlphaGradState(self._graph, self.t, self.to_internal, self.Fo)

    def launch_v2(self, H, Fo, slope, WW, a2, m, Z, st):
        check(lib.pygat_gatv2_attention(*self._pattern_args(), H, Fo, float(slope), WW.data_ptr(), a2.data_ptr(), m.data_ptr(),
                                        Z.data_ptr(), self.alpha.data_ptr(), st), "gatv2_attention")


class AlphaGradState:
    """The caller's pattern (forward and transposed, with perm_t), the node map and the t table of a level whose attention
    coefficients are a differentiable output: scores() runs the row and the column pass of csrc/k14_alpha_grad.hip."""

    def __init__(self, graph, t: torch.Tensor, to_internal: Optional[torch.Tensor], Fo: int):
        self.graph, self.t, self.to_internal, self.Fo = graph, t, to_internal, Fo

    def scores(self, A: torch.Tensor, s, m, Z, slope: float, st: int):
        """A [E, H] = dL/d alpha in the caller's edge order -> (ds', dt') [N, H] in the level's node order."""
        g, t = self.graph, self.t
        n, H = t.shape
        if tuple(A.shape) != (g.nnz, H):
            raise ValueError(f"pygat_amd: gradient of alpha {tuple(A.shape)}: expected {(g.nnz, H)}")
        A = A.contiguous().float()
        dev, f32 = t.device, torch.float32
        rec = torch.empty(n, H, 4, dtype=f32, device=dev)
        part = torch.empty(_lib.alpha_grad_workspace_bytes(g.nnz, H) // 4, dtype=f32, device=dev)
        ds2 = torch.empty(n, H, dtype=f32, device=dev)
        dt2 = torch.empty(n, H, dtype=f32, device=dev)
        f, b = g.fwd, g.bwd
        with _span("k14_alpha_rows"):
            check(lib.pygat_alpha_grad_rows(f.n, f.nnz, f.rowptr.data_ptr(), f.edge_rc.data_ptr(), _ptr(self.to_internal), H, self.Fo,
                                            float(slope), s.data_ptr(), t.data_ptr(), m.data_ptr(), Z.data_ptr(), A.data_ptr(),
                                            rec.data_ptr(), ds2.data_ptr(), part.data_ptr(), st), "alpha_grad_rows")
        with _span("k14_alpha_cols"):
            check(lib.pygat_alpha_grad_cols(b.n, b.nnz, b.rowptr.data_ptr(), b.edge_rc.data_ptr(), g.perm_t.data_ptr(),
                                            _ptr(self.to_internal), H, self.Fo, float(slope), t.data_ptr(), rec.data_ptr(), A.data_ptr(),
                                            dt2.data_ptr(), part.data_ptr(), st), "alpha_grad_cols")
        return ds2, dt2


def alpha_grad_scores(graph: CSRGraph, s, t, m, Z, A, slope: float, Fo: int, to_internal=None):
    """Just the two passes of csrc/k14_alpha_grad.hip: node tables s, t, m, Z [N, H] (float32, the level's node order), A [E, H] =
    dL/d alpha in the edge order of `graph` -> (ds', dt') [N, H], the score gradients a loss on alpha adds to a level's backward."""
    with torch.cuda.device(t.device):
        return AlphaGradState(graph, t.contiguous(), to_internal, Fo).scores(A, s.contiguous(), m.contiguous(), Z.contiguous(), slope,
                                                                         _stream())


class StackHeads(torch.autograd.Function):
    """(W [H,Fin,F'], a [H,2F'], Wskip [H,Fin,F'] | None) from the per-head parameter tensors in ONE launch (torch.stack: a
    cat launch per parameter kind); backward: views of the stacked gradients.  forward(H, skip, rows, *Ws, *As[, *Wskips]);
    rows > Fin: W and Wskip come out as [H, rows, F'] with zero rows appended (gat_level on padded input columns)."""

    @staticmethod
    def forward(ctx, H: int, skip: bool, rows: int, *params):
        Ws, As = params[:H], params[H:2 * H]
        Ss = params[2 * H:3 * H] if skip else ()
        dev, f32 = Ws[0].device, torch.float32
        ctx.shapes = [tuple(p.shape) for p in params]
        ctx.H, ctx.skip = H, skip
        ok = Ws[0].is_cuda and H <= MAX_HEAD_TABLE and all(p.dtype == f32 and p.is_contiguous() for p in params)
        pad = rows > 0 and rows != Ws[0].shape[0]
        if not ok:
            grow = (lambda t: torch.nn.functional.pad(t, (0, 0, 0, rows - t.shape[0]))) if pad else (lambda t: t)   # noqa: E731
            return (torch.stack([grow(w) for w in Ws], 0), torch.stack([q.reshape(-1) for q in As], 0),
                    torch.stack([grow(w) for w in Ss], 0) if skip else None)
        wshape = (rows, *Ws[0].shape[1:]) if pad else tuple(Ws[0].shape)
        W = torch.empty(H, *wshape, dtype=f32, device=dev)
        a = torch.empty(H, As[0].numel(), dtype=f32, device=dev)
        S = None
        if skip:                                                                        # (GATv2: W is [2 Fin, F'], the skip [Fin, F'])
            S = torch.empty(H, *((rows, *Ss[0].shape[1:]) if pad else Ss[0].shape), dtype=f32, device=dev)
        PT = C.c_void_p * H
        with torch.cuda.device(dev):
            check(lib.pygat_stack_heads_padded(H, Ws[0].numel(), W[0].numel(), As[0].numel(), Ss[0].numel() if skip else 0,
                                               S[0].numel() if skip else 0, PT(*[w.data_ptr() for w in Ws]),
                                               PT(*[v.data_ptr() for v in As]), PT(*[w.data_ptr() for w in Ss]) if skip else None,
                                               W.data_ptr(), a.data_ptr(), _ptr(S), _stream()), "stack_heads")
        return W, a, S

    @staticmethod
    def backward(ctx, dW, da, dS):
        H = ctx.H
        rows_w = ctx.shapes[0][0]
        outs = [None if dW is None else dW[k][:rows_w] for k in range(H)]               # (a view: the first Fin rows are contiguous)
        outs += [None if da is None else da[k].reshape(ctx.shapes[H + k]) for k in range(H)]
        if ctx.skip:
            rows_s = ctx.shapes[2 * H][0]
            outs += [None if dS is None else dS[k][:rows_s] for k in range(H)]
        return (None, None, None) + tuple(outs)


def stack_heads(Ws, As, Wskips):
    """-> (W, a, Wskip) stacked; one launch."""
    return StackHeads.apply(len(Ws), Wskips is not None, 0, *Ws, *As, *(Wskips if Wskips is not None else ()))


def gat_level(x: torch.Tensor, graph: CSRGraph, Ws: Sequence[torch.Tensor], As: Sequence[torch.Tensor],
              Wskips: Optional[Sequence[torch.Tensor]], alpha: float, concat: bool, pipeline=None, xs=None,
              return_attention=False, attention_order=None, edge_logit=None, table_dtype=None):
    """All heads of one level. Ws: H tensors [Fin,F']; As: H tensors with 2F' elements
    ([2F',1] as in GraphAttentionLayer, layers.py:23, or [1,2F'] as in SpGraphAttentionLayer,
    layers.py:114); Wskips: H tensors [Fin,F'] or None.  pipeline: see GATLevelFn.  xs: features.SparseFeatures of x
    (a first level on sparse input features) or None.
    return_attention: -> (out, alpha), alpha [E, H] float32 (detached) = the softmax coefficient of every edge and head, in
    the edge order of `graph` (graph.edge_index()); attention_order: see AttentionTarget.
    return_attention="grad": the same alpha as a second DIFFERENTIABLE output of the level -- a loss may use out, alpha or both
    (csrc/k14_alpha_grad.hip); a loss on `out` alone runs the backward it runs without it.
    edge_logit: u [E, H] (or [E] / [E, 1], the same term for every head) added to the score of every edge in front of the
    LeakyReLU, z_ij = s_i + t_j + u_ij, row k = edge k of graph.edge_index() (csrc/k15_edge_logit.hip).  Differentiable:
    its gradient is dz_ij (summed over the heads for the broadcast forms).  A row with one edge has alpha = 1 and never reads
    its u.  The edge-logit level runs in the caller's node order on a dense 2-D x and takes neither a pipeline, sparse xs, an
    attention_order, return_attention="grad", a column-blocked x nor a graph with a row map / an InternalOrderView (ValueError);
    return_attention=True is supported.  None: the level takes exactly the path it takes without the argument.
    table_dtype: None (the fp32 tables: exactly the path without the argument) or torch.bfloat16 -- the INFERENCE forward on a
    bf16 feature table (csrc/k16_bf16_forward.hip): the level is the fp32 level applied to Whq = bf16(x W) (round to nearest
    even, once per element; s and t from the rounded rows; softmax, sums, skip term, ELU and output fp32), its gathers move
    2 instead of 4 bytes per table element.  No backward: ValueError when autograd is on and x or a parameter requires grad,
    and for a pipeline, sparse xs, return_attention, attention_order, edge_logit, a column-blocked x or a row-map graph."""
    H = len(Ws)
    if table_dtype is not None:
        return _bf16_level(x, graph, Ws, As, Wskips, alpha, concat, table_dtype, return_attention, pipeline, xs, attention_order,
                           edge_logit)
    if edge_logit is not None:
        return _edge_logit_level(x, graph, Ws, As, Wskips, alpha, concat, edge_logit, return_attention, pipeline, xs, attention_order)
    if return_attention and pipeline is not None:
        raise ValueError("pygat_amd: return_attention does not take a pipeline")
    grad = attention_mode(return_attention)
    att = AttentionTarget(graph, H, x.device, attention_order, grad=grad) if return_attention else None
    out = _gat_level(x, graph, Ws, As, Wskips, alpha, concat, pipeline, xs, att)
    if grad:
        return out           # (out, alpha): both outputs of the level's autograd node
    return (out, att.alpha) if return_attention else out


def no_edge_logit(edge_logit, what: str) -> None:
    """The entry points the edge-logit term (gat_level(..., edge_logit=u), csrc/k15_edge_logit.hip) does not cover."""
    if edge_logit is not None:
        raise ValueError(f"pygat_amd: {what} does not take edge_logit: the per-edge logit term covers the plain GAT (v1) level "
                         "(ops.gat_level) only")


def attention_mode(return_attention) -> bool:
    """return_attention: False / True (detached coefficients) / "grad" (differentiable) -> is it "grad"?"""
    if isinstance(return_attention, str):
        if return_attention != "grad":
            raise ValueError(f"pygat_amd: return_attention={return_attention!r}: expected False, True or \"grad\"")
        return True
    return False


def _gat_level(x, graph, Ws, As, Wskips, alpha, concat, pipeline, xs, att):
    H = len(Ws)
    Fin = x.shape[1]
    if (xs is None and PAD_K and Fin % 16 and 16 < Fin <= 1024 and x.is_cuda and not x.requires_grad and x.dim() == 2
            and H <= MAX_HEAD_TABLE and Ws[0].dim() == 2 and Ws[0].is_cuda):
        # input columns zero-padded to a multiple of 16 (cached with x, like the sparse pattern) and zero rows appended to the
        # weights while they are stacked: the split-bf16 kernels take K in steps of 16; on PPI's 50 input features the fp32
        # fallback ran the projection at 45 us and the two weight gradients at 60-67 us, against 12 / 10 us on 64
        from .features import padded_columns
        xp = padded_columns(x, 16)
        W, a, Wskip = StackHeads.apply(H, Wskips is not None, xp.shape[1], *Ws, *As, *(Wskips if Wskips is not None else ()))
        return GATLevelFn.apply(xp, W, a, Wskip, graph, alpha, concat, None, pipeline, att)
    if H <= MAX_HEAD_TABLE:        # parameters read in place through a pointer table: no torch.stack launches
        return GATLevelHeadsFn.apply(x, graph, alpha, concat, pipeline, H, Wskips is not None, xs, att, *Ws, *As,
                                     *(Wskips if Wskips is not None else ()))
    W = torch.stack(list(Ws), 0)
    a = torch.stack([p.reshape(-1) for p in As], 0)
    Wskip = torch.stack(list(Wskips), 0) if Wskips is not None else None
    return GATLevelFn.apply(x, W, a, Wskip, graph, alpha, concat, None, pipeline, att)
