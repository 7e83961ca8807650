/*
 * pygat_amd.h -- C ABI of the MI355X (gfx950) GAT attention-layer hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.  The
 * reference (ArielleRosinski/pyGAT) is pure Python and owns no FFI; the entry
 * points below replace the ATen call sequences of its layer/op boundary:
 *
 *   GraphAttentionLayer.forward          layers.py:32-53   (dense N x N path)
 *   _prepare_attentional_mechanism_input layers.py:55-64   (s_i + t_j split)
 *   SpecialSpmmFunction.forward/backward layers.py:72-90   (COO spmm + its grads)
 *   SpGraphAttentionLayer.forward        layers.py:125-173 (edge-list path)
 *   GAT.forward head concat / head mean  models.py:29-35
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; the caller owns all
 *     memory including workspaces; nothing here allocates, frees or synchronises.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); kernels
 *     are only enqueued, never waited for.
 *   - return 0 on success, a negative PYGAT_E* code otherwise; the message of the
 *     last error on the calling thread is at pygat_last_error().  Nothing throws.
 *   - floats are fp32, indices int32.  Feature tables are row-major and PADDED:
 *     a level with H heads of F' outputs uses Fp = pygat_padded_width(F') columns
 *     per head and R = H*Fp floats per node row ("head-interleaved row").
 *   - graph = CSR pattern of the adjacency: row i lists the j with adj[i][j] != 0
 *     (layers.py:129: edge[0] = i = softmax row, edge[1] = j = gathered node).
 *   - no mutable library state besides the thread-local error string, and (since ABI 13) no environment variable is
 *     read while the library runs: two process-level defaults are read ONCE when it is loaded -- PYGAT_GEMM_F32=1
 *     (what PYGAT_GEMM_DEFAULT means, see the GEMM section) and PYGAT_NARROW=0 (pygat_dropout_narrow answers 0) --
 *     and every layout choice a caller can see (head windows of the backward, slot length, GEMM product mode, split-K)
 *     is an ARGUMENT.
 */
#ifndef PYGAT_AMD_H
#define PYGAT_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYGAT_ABI_VERSION 16

enum {
  PYGAT_OK = 0,
  PYGAT_EINVAL = -1,   /* bad argument (null pointer, size, alignment, unsupported width) */
  PYGAT_EHIP = -2,     /* a HIP launch failed; message holds hipGetErrorString */
  PYGAT_ENODEV = -3    /* no gfx950 device / code object not loadable */
};

/* flags for pygat_gat_forward / pygat_gat_backward */
enum {
  PYGAT_F_ELU = 1,      /* apply ELU to (attention + skip): concat=True, layers.py:50-51,168-170 */
  PYGAT_F_SKIP = 2,     /* add the skip projection rows `sk` (layers.py:47-48,165-166) */
  /* pygat_gat_forward only (ABI 14): run ONE phase of the pass over the graph's slot range -- the main launch (rows that lie
   * inside a slot are final after it) or the fix-up launch (finishes the rows a slot border cuts, from the main launch's
   * partial records).  A row-chunk pipeline puts chunk c's fix-up on a second stream beside chunk c + 1's main launch.
   * Needs the level in one head window: pygat_gat_forward_phases_ok(n, H, F') == 1. */
  PYGAT_F_MAIN_ONLY = 4,
  PYGAT_F_FIXUP_ONLY = 8
};

int pygat_abi_version(void);
const char* pygat_last_error(void);
/* Fp for a head width F' (power of two >= 4, <= 256); 0 if unsupported. */
int pygat_padded_width(int f_out);
/* number of HIP devices visible / name of the current one (host buffers). */
int pygat_device_count(void);
int pygat_device_name(char* host_buf, int len);
/* Registers per lane and scratch bytes per lane of a tuned kernel as the LOADED code object reports them (hipFuncGetAttributes):
 * "k2_headline" (fused forward, 8 heads x 16, training), "k4_headline_da" (column pass with the a-gradient sums), "tn_x3w"
 * (streamed-K weight gradient), "x3gw" (general split-bf16 GEMM), "k1_x3_tail" (the headline projection with the
 * self-loop-only tail's output folded in, ABI 15), "tn_x3w_tail" (the weight gradient that forms the tail's dWh rows).  The attention kernels were tuned at four waves per SIMD
 * without scratch; `amdgpu_waves_per_eu` makes the compiler spill rather than fail, so tests/test_gpu_properties.py asks. */
int pygat_kernel_footprint(const char* kernel, int* num_regs, int* scratch_bytes);

/* How the fp32 GEMMs of a level (the projection `mm(h, W)`, layers.py:35,134, its weight and input gradients) form
 * their products.  Operands, accumulators and results are fp32 in both modes.
 *   PYGAT_GEMM_SPLIT_BF16: each operand is cut EXACTLY into three bf16 pieces (8 + 8 + 8 significant bits) and all
 *     nine piece products are summed into fp32 accumulators by v_mfma_f32_32x32x16_bf16 -- no operand bit is dropped,
 *     the fp32 additions happen in another order than below; 288 instead of 512 MFMA cycles per 32 x 32 x 16 block.
 *     Shapes the split kernels do not take use the fp32 kernels.  Caveats: the cut is exact for finite operands whose
 *     mid and low pieces stay normal bf16 numbers (|x| >= 2^-110 or x == 0; smaller magnitudes lose their low bits,
 *     i.e. are treated as fp32 denormal-range values); a NON-FINITE operand gives NaN where the fp32 kernels give
 *     +-inf (inf - inf inside the cut).
 *   PYGAT_GEMM_FP32_MFMA: v_mfma_f32_32x32x2_f32 throughout.
 *   PYGAT_GEMM_DEFAULT: the process default -- split-bf16, or fp32 MFMA with PYGAT_GEMM_F32=1 in the environment
 *     (read once when the library is loaded; pygat_default_gemm_mode() reports it).
 * The mode is an ARGUMENT (`gemm_mode`) of every entry point that runs a GEMM: the library holds no mutable state
 * besides the thread-local error string, so two threads / two models may use different modes at the same time. */
enum { PYGAT_GEMM_DEFAULT = -1, PYGAT_GEMM_SPLIT_BF16 = 0, PYGAT_GEMM_FP32_MFMA = 1 };
int pygat_default_gemm_mode(void);

/* ------------------------------------------------------------------ K0: graph
 * Replaces `adj.nonzero().t()` (layers.py:129), run ONCE per graph instead of
 * once per head per forward, and the `adj > 0` mask of layers.py:41.
 * mode 0: pattern = (adj != 0) (sparse layer), mode 1: pattern = (adj > 0) (dense layer).
 */
/* counts[i] = nnz of row i of the dense n x n matrix (ld = row stride in floats). */
int pygat_dense_row_counts(const float* adj, int n, int64_t ld, int mode,
                           int32_t* counts, void* stream);
/* exclusive scan: out[0] = 0, out[i+1] = sum(in[0..i]); in/out length n / n+1.
 * ws: >= pygat_scan_workspace_bytes(n) bytes. */
size_t pygat_scan_workspace_bytes(int64_t n);
int pygat_exclusive_scan_i32(const int32_t* in, int64_t n, int32_t* out, void* ws, void* stream);
/* col[rowptr[i] ...] = sorted column indices of row i's pattern. */
int pygat_dense_fill_cols(const float* adj, int n, int64_t ld, int mode,
                          const int32_t* rowptr, int32_t* col, void* stream);
/* For a structurally symmetric CSR with sorted rows: perm[k] = position of edge
 * (j,i) for the edge k = (i,j); flags[0] is set to 1 if some edge has no mirror
 * (pattern not symmetric), flags[1] to 1 if some row is empty. flags must be zeroed. */
int pygat_csr_symmetric_perm(int n, const int32_t* rowptr, const int32_t* col,
                             int32_t* perm, int32_t* flags, void* stream);

/* ------------------------------------------------------------ K1: projection
 * Replaces torch.mm(h, W) per head (layers.py:35,134), the skip torch.mm
 * (layers.py:48,166) and the two a-halves matmuls (layers.py:60-61):
 *   C[M x N] = op(A) * op(B) (+ C if accumulate), fp32 MFMA, row-major.
 * Output columns can be routed to up to PYGAT_MAX_SEGMENTS destination tables (seg_*): columns
 * [seg_col[s], seg_col[s+1]) of C go to seg_ptr[s] with row stride seg_ld[s] (the projection's Wh | Sk | s
 * tables; the per-rank column blocks of a head-parallel level's input gradient, pygat_amd/dist.py).
 */
#define PYGAT_MAX_SEGMENTS 4
typedef struct {
  int nseg;                                       /* 1..PYGAT_MAX_SEGMENTS */
  int32_t col_start[PYGAT_MAX_SEGMENTS + 1];      /* col_start[0] = 0, col_start[nseg] = N */
  float* ptr[PYGAT_MAX_SEGMENTS];
  int64_t ld[PYGAT_MAX_SEGMENTS];
} pygat_out_segments;

/* transA: A is stored [K x M]; transB: B is stored [N x K]. split_k >= 1: when >1 the
 * K range is cut in split_k slabs whose partial products go to `ws`
 * (>= pygat_gemm_workspace_bytes) and are then summed in slab order (deterministic). */
size_t pygat_gemm_workspace_bytes(int M, int N, int split_k);
int pygat_gemm_f32(int transA, int transB, int M, int N, int64_t K,
                   const float* A, int64_t lda, const float* B, int64_t ldb,
                   const pygat_out_segments* out, int accumulate,
                   int split_k, void* ws, int gemm_mode, void* stream);

/* Column-blocked matrices (ABI 14): the activation of a head-parallel hidden level as the exchange over xGMI delivers it
 * (pygat_amd/dist.py; replaces torch.cat([...], dim=1), models.py:32, WITHOUT the concatenating copy).  A logical
 * [rows x cols] row-major matrix is stored as cols / w BLOCKS of [rows x w], block b (= rank b's heads, all rows) at
 * base + b * stride floats, row stride ld inside a block:
 *      element (r, c)  at  base + (c / w) * stride + r * ld + (c % w)
 * w: a power of two >= 16 dividing cols (w = 0, or a NULL descriptor: an ordinary matrix); stride, ld, base: multiples
 * of 4 floats / 16-byte aligned.  `a_blk` describes the STORED matrix of operand A along its contiguous dimension (the
 * K columns of a plain A, the M columns of a transA one: in both cases X [nodes x features] blocked by features);
 * `c_blk` the output C along its N columns (then `out` has ONE segment: ptr[0] = base, ld[0] = row stride, and
 * split_k must be 1) -- an input gradient written straight into the layout the reduce-scatter sends.
 * Blocked operands run on the general kernels of either product mode (no streamed fast path takes them). */
typedef struct {
  int w;             /* columns per block; 0 = not blocked */
  int64_t stride;    /* floats between block b and block b + 1 */
} pygat_col_blocks;
int pygat_gemm_f32_blocked(int transA, int transB, int M, int N, int64_t K,
                           const float* A, int64_t lda, const pygat_col_blocks* a_blk, const float* B, int64_t ldb,
                           const pygat_out_segments* out, const pygat_col_blocks* c_blk, int accumulate,
                           int split_k, void* ws, int gemm_mode, void* stream);

/* Pack the per-head parameters of one level into the projection operand
 *   Wcat [Fin x ldw], columns: [0,R) W heads (padded to Fp), [R,2R) skip heads if
 *   w_skip != NULL, then H columns W_h a_src_h and H columns W_h a_dst_h (so the
 *   projection also yields s and t), zero padded up to ldw (multiple of 4);
 *   a_pad [H x 2 x Fp]: a_src then a_dst per head, zero padded.
 * W [H x Fin x F'], a [H x 2F'] (a[:F'] = a_src multiplies Wh_i, layers.py:60),
 * w_skip [H x Fin x F'] or NULL. */
int pygat_pack_params(int H, int Fin, int Fo, const float* W, const float* a,
                      const float* w_skip, float* Wcat, int64_t ldw, float* a_pad,
                      void* stream);
/* The same with the parameters where the reference keeps them: one W [Fin x F'], a (2F' values) and skip_projection
 * [Fin x F'] tensor PER HEAD module (layers.py:21-28,111-119; models.py:15-27).  W, a, w_skip (or NULL): HOST arrays of H
 * device pointers, H <= PYGAT_MAX_HEADS_TABLE (they travel as kernel arguments) -- no stacking copy before the level. */
#define PYGAT_MAX_HEADS_TABLE 16
int pygat_pack_params_heads(int H, int Fin, int Fo, const float* const* W, const float* const* a,
                            const float* const* w_skip, float* Wcat, int64_t ldw, float* a_pad, void* stream);
/* torch.stack of the per-head parameters in ONE launch: W_out [H x nW], a_out [H x nA], skip_out [H x nS] (or NULL) from host
 * arrays of H device pointers (the level flavours that take stacked parameters: dropout, GATv2). */
int pygat_stack_heads(int H, int64_t nW, int nA, int64_t nS, const float* const* W, const float* const* a,
                      const float* const* w_skip, float* W_out, float* a_out, float* skip_out, void* stream);
/* The same with output blocks of nW_out >= nW (nS_out >= nS) elements per head, the tail zero: [Fin, F'] weights with zero
 * rows appended, for a level whose Fin is not a multiple of 16 run on zero-padded input columns (PPI: 50 -> 64; the split-
 * bf16 kernels take K in steps of 16, the fp32 fallback ran that level's three products at a sixth of their speed). */
int pygat_stack_heads_padded(int H, int64_t nW, int64_t nW_out, int nA, int64_t nS, int64_t nS_out, const float* const* W,
                             const float* const* a, const float* const* w_skip, float* W_out, float* a_out, float* skip_out,
                             void* stream);
/* Projection of one level in one GEMM: [Wh | Sk | s] = X * Wcat[:, :R (+R) + H]; the H columns behind the
 * heads are W_h a_src_h (pygat_pack_params), so s_i = Wh_i . a_src (layers.py:60) comes out of the same pass.
 * a_pad (pygat_pack_params; may be NULL): lets the kernel form s from the Wh accumulators themselves -- the
 * reference's own order, Wh_i . a_src -- where a head is 8 or 16 columns wide and Fin is 64 or 128.
 * Sk may be NULL (no skip).  split_k / ws as pygat_gemm_f32. */
int pygat_project(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const float* Wcat, int64_t ldw, const float* a_pad,
                  float* Wh, float* Sk, float* s, int split_k, void* ws, int gemm_mode, void* stream);
/* The same with X column-blocked (x_blk as in pygat_gemm_f32_blocked; NULL / w = 0: pygat_project). */
int pygat_project_blocked(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const pygat_col_blocks* x_blk,
                          const float* Wcat, int64_t ldw, const float* a_pad, float* Wh, float* Sk, float* s, int split_k,
                          void* ws, int gemm_mode, void* stream);
/* s[n x H], t[n x H] (t may be NULL) from the masked Wh table: s_ih = Wh_ih . a_src_h, t_ih = Wh_ih . a_dst_h
 * (layers.py:60-61 after the Wh dropout of layers.py:37,136).  wh_mask [n x R] (pre-scaled) non-NULL: that dropout is
 * applied HERE, in place (Wh *= wh_mask), instead of by a launch of its own; NULL: Wh is taken as it is.
 * a_pad as written by pygat_pack_params. */
int pygat_attn_scores(int n, int H, int Fo, float* Wh, const float* wh_mask, const float* a_pad,
                      float* s, float* t, void* stream);
/* Inverse for gradients: dW[H x Fin x F'] (+)= columns of dWcat [Fin x ld]. */
int pygat_unpack_wgrad(int H, int Fin, int Fo, const float* dWcat, int64_t ld,
                       int col_offset, float* dW, void* stream);

/* ---------------------------------------------- K2: fused edge-softmax + aggregate
 * Replaces layers.py:141-170 (and 40-51): per row i and head h
 *   e_ij = LeakyReLU(s_i + t_j), m_i = max_j e_ij, p_ij = exp(e_ij - m_i),
 *   Z_i = sum_j p_ij, hattn_i = (sum_j p_ij Wh_j) / Z_i,
 *   out_i = [ELU](hattn_i [+ sk_i]).
 * Work is split by EDGES, not rows ("nnz split"): the CSR edge list is cut into
 * slots of `slot_edges` consecutive edges; a slot walks its edges with the
 * online-softmax recurrence and finishes every row that lies wholly inside it.
 * Rows cut by a slot border leave partial (m, Z, acc) records in `part`, merged in
 * slot order by a second small launch (deterministic, no atomics).
 */
typedef struct {
  int n;                     /* nodes */
  int64_t nnz;               /* edges */
  const int32_t* rowptr;     /* [n+1] */
  const int32_t* edge_rc;    /* [nnz][2]: (row i, column j) of every edge, CSR order (pygat_edge_pairs) */
  int slot_edges;            /* nominal edges per slot: multiple of 4, >= 4 */
  const int32_t* slot_begin; /* NULL: slot k = edges [k*slot_edges, (k+1)*slot_edges); else [n_slots+1]
                                row-snapped borders from pygat_slot_bounds (fewer rows are cut) */
  const int32_t* cut_rows;   /* NULL, or [n_cut][3] = (first slot k, row, number of pieces) of every row that a
                                slot border cuts, sorted by pieces descending: lets the fix-up launches go
                                straight to the cut rows instead of screening every slot */
  int n_cut;
  int n_cut_wide;            /* leading entries with more than 32 pieces (merged by a whole work-group) */
  /* pygat_gat_forward only: work on the slots [slot_first, slot_first + slot_count) -- a range of whole rows (its
     first slot starts a row, the slot after its last one too); cut_rows then lists the cut rows of that range alone.
     slot_count = 0: all slots.  Lets a caller pipeline row chunks of a level (pygat_amd/dist.py: chunk k's head
     outputs travel over xGMI while chunk k+1 is computed).  Every other entry point needs 0, 0. */
  int64_t slot_first;
  int64_t slot_count;
  /* NULL, or [n_slots][4] = (first edge, end edge, row of the first edge, flags) of every slot, flags bit 0: the slot's
     first row began in an earlier slot, bit 1: its last row continues in a later one (pygat_slot_meta).  One 16-byte load
     then replaces the slot's start-up chain slot_begin -> edge_rc -> rowptr and the rowptr load at its end: what a slot
     costs in DEPENDENT memory round trips is what bounds the attention kernels on small graphs and on narrow rows. */
  const int32_t* slot_meta;
  /* NULL, or [n_slots] a permutation of the slot ids (ABI 14): the MAIN launches of pygat_gat_forward and
     pygat_gat_backward_col hand slot slot_order[q] to grid position q (work-groups are dispatched in grid order, eight
     lane groups of consecutive q each), i.e. the ORDER in which slots are walked -- and with it which rows' gathers are in
     flight together -- without renumbering a node or moving a table row.  Results do not depend on it (partial records
     and fix-up launches go by the slot id).  Needs slot_count = 0. */
  const int32_t* slot_order;
  /* NULL, or [n] (ABI 14): this pattern is an INTERNAL renumbering of the caller's graph (pygat_amd/graph.py, degree order) and
     user_row[i] is the caller's row of internal node i.  Every node table the kernels exchange among themselves is in internal
     order; the caller-facing ones are addressed through this map: pygat_gat_forward writes row user_row[i] of `out`
     (pygat_gat_backward_prepare takes the same map as an argument for G and the saved output). */
  const int32_t* user_row;
} pygat_graph;

/* edge_rc[k] = (i, col[k]) for rowptr[i] <= k < rowptr[i+1] */
int pygat_edge_pairs(int n, const int32_t* rowptr, const int32_t* col, int32_t* edge_rc, void* stream);

/* slot_begin[k] = k*slot_edges, moved forward to the next row start when that is less than
 * slot_edges/2 edges away (so most slot borders fall between rows and only rows longer than
 * slot_edges/2 are ever cut); slot_begin[n_slots] = nnz, n_slots = ceil(nnz / slot_edges). */
int pygat_slot_bounds(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int slot_edges,
                      int32_t* slot_begin, void* stream);
/* slot_meta[k] = (first edge, end edge, row of the first edge, flags) for the slots of `slot_begin` (NULL: uniform
 * slots of slot_edges) -- see pygat_graph.slot_meta.  slot_meta: [n_slots][4] int32, 16-byte aligned. */
int pygat_slot_meta(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int slot_edges,
                    const int32_t* slot_begin, int32_t* slot_meta, void* stream);

/* bytes of `part` workspace needed by forward / column backward for this graph and row width */
size_t pygat_partials_bytes(int64_t nnz, int slot_edges, int H, int Fp);

/* Heads per backward kernel pass ("head window").  The attention entry points take the level's
 * full-width tables.  The forward walks rows of up to 1024 floats per pass; the two backward passes of
 * a LARGE graph (gathered table beyond the 256 MiB Infinity Cache) with rows wider than 512 floats walk
 * the heads in windows of at most 256 floats (one 16-byte chunk per lane of a wave64): window w covers
 * heads [w*hg, min(H, (w+1)*hg)), hg = pygat_head_group(n, H, F').  Callers only need it to find Gp
 * inside GR (see K3a below).  Returns H when the backward takes the whole row in one pass, 0 on bad
 * arguments.  It is a pure function of its arguments and only the DEFAULT: prepare / row / col take `head_group`
 * (heads per window; 0 = this default; any value whose windows are at most 1024 floats wide) as an argument, and
 * the caller passes the SAME value to all three and lays GR out accordingly.  (Until ABI 12 an environment
 * variable read on every call moved the threshold: process state deciding a layout the caller allocates.) */
int pygat_head_group(int n, int H, int Fo);

/* Wh [n x R], s,t [n x H], sk [n x R] or NULL.
 * out [n x H*F'] compact (may be NULL), hattn [n x R] padded (may be NULL; needed for the
 * head mean), m,Z [n x H] (may be NULL together in eval).
 * aneg [n x R], qneg [n x H] (NULL together; need m,Z): the training forward also leaves the share of each row
 * sum that went through the alpha branch of the LeakyReLU,
 *     aneg_i = sum_{j: s_i+t_j <= 0} alpha_ij mask_ij Wh_j,     qneg_i = sum_{j: s_i+t_j <= 0} alpha_ij,
 * from which pygat_gat_backward_prepare takes the row sums ds_i = sum_j dz_ij without touching an edge again
 * (sum_j de_ij = 0, so ds_i = -(1 - alpha)(Gp_i . aneg_i - D_i qneg_i)). */
int pygat_gat_forward_phases_ok(int n, int H, int Fo);   /* 1: PYGAT_F_MAIN_ONLY / PYGAT_F_FIXUP_ONLY may be used */
int pygat_gat_forward(const pygat_graph* g, int H, int Fo, float alpha, int flags,
                      const float* Wh, const float* s, const float* a_pad, const float* sk,
                      const float* att_mask,
                      float* out, float* hattn, float* m, float* Z, float* aneg, float* qneg,
                      void* part, void* stream);

/* models.py:34: out[n x F'] = mean over heads of (hattn [+ sk]) (padded inputs). */
int pygat_head_mean(int n, int H, int Fo, const float* hattn, const float* sk,
                    float* out, void* stream);

/* ------------------------------------------------ K3/K4: backward, no N x N, no atomics
 * Replaces SpecialSpmmFunction.backward (layers.py:81-90) and the autograd of
 * layers.py:141-170.
 *   K3a prepare (per row):  Gp_i = G_i * ELU'(.), D_i = Gp_i . hattn_i,
 *        GR_i = [ Gp_i (R floats) | (s_i, m_i, 1/Z_i, D_i) per head (4H floats) ]   -> GR [n x (R+4H)]
 *        With more than one head window (pygat_head_group(n,H,F') < H) the row is laid out window by
 *        window, each [ Gp of its heads | their 4-float records ], window w starting at float
 *        w*hg*(Fp+4): head h's Gp slice is at  (h/hg)*hg*(Fp+4) + (h%hg)*Fp.
 *        mean_mode 0: G is [n x H*F'] and y is the forward OUTPUT out [n x H*F'] (hattn is
 *                     recovered from it: out > 0 ? out : log1p(out), minus sk);
 *        mean_mode 1: G is [n x F'] (every head receives G/H, models.py:34), y is hattn [n x R].
 *   K3b row pass (nnz split over the forward pattern g): per edge (i,j)
 *        alpha_ij = exp(LeakyReLU(s_i + t_j) - m_i)/Z_i, dz_ij = alpha_ij (mask_ij Gp_i.Wh_j - D_i) LeakyReLU'(.)
 *        ds_i = sum_j dz_ij            (GR_i row-local, Wh_j gathered; the layers.py:85 entry, per edge)
 *   K4 column pass (nnz split over the TRANSPOSED pattern gT, any pattern, symmetric or not):
 *        alpha_ij, dz_ij recomputed (GR_i gathered as one contiguous row, Wh_j row-local)
 *        dWh_j = sum_i alpha_ij mask_ij Gp_i + ds_j a_src + dt_j a_dst,  dt_j = sum_i dz_ij
 * Nothing per-edge is stored between the passes.  att_mask [nnz x H] (forward edge order) or NULL;
 * perm_t[k] = forward edge of gT's edge k, needed only to index att_mask (may be NULL without mask).
 * pygat_gat_backward_col takes EITHER ds (from the row pass; dz_t = NULL) OR dz_t (ds = NULL; see
 * pygat_gat_backward_rowsum below).
 * part: >= pygat_partials_bytes for both passes.
 *
 * Head range.  The backward entry points (prepare, row, col, rowsum, a_grad, wgrad) end in (h_first, h_count):
 * gradients are produced for the heads [h_first, h_first + h_count) of the level only; 0, 0 = all heads.  The
 * level's tables keep their full width (H heads) and are addressed with the level's strides; only GR, which
 * nothing but the backward touches, is then COMPACT for the range ([n x h_count*(Fp+4)], same layout rules with
 * h_count in place of H), and dW / da rows outside the range are left untouched.  Use: a rank of a head-parallel
 * run that ran the forward for all heads (cheaper than receiving them over one xGMI link) back-propagates its own.
 */
/* pygat_gat_backward_prepare: aneg, qneg (from the training forward) and ds non-NULL together: K3a also writes
 * ds [n x H] (LeakyReLU slope `alpha`), after which pygat_gat_backward_col is called WITH ds and neither the row
 * pass nor the row-sum pass runs -- the default backward.  All three NULL: GR only. */
int pygat_gat_backward_prepare(int n, int H, int Fo, int flags, int mean_mode,
                               const float* G, const float* y, const float* sk,
                               const float* s, const float* m, const float* Z,
                               float* GR, const float* aneg, const float* qneg, float alpha, float* ds,
                               int h_first, int h_count, int head_group, const int32_t* user_row, void* stream);
/* user_row (ABI 14; NULL = identity): the tables are in the INTERNAL node order of a renumbered pattern
 * (pygat_graph.user_row): G -- and, in concat mode, y = the level's saved output -- are the caller's arrays and are read at
 * row user_row[i] for internal node i; every other table is internal. */
int pygat_gat_backward_row(const pygat_graph* g, int H, int Fo, float alpha,
                           const float* Wh, const float* a_pad, const float* GR,
                           const float* att_mask, float* ds, void* part, int h_first, int h_count, int head_group,
                           void* stream);
/* da_part (or NULL): the column pass also takes the attention-vector gradient along (autograd of layers.py:60-61 /
 * a.mm(edge_h) layers.py:144): where row j finishes -- dt_j just formed, ds_j loaded for the dWh term, Wh_j in L1 from the
 * row's edges -- every lane adds ds_j Wh_j and dt_j Wh_j into two float4s of its own in LDS, and each work-group leaves ONE
 * record [2 R] = (sum ds_j Wh_j | sum dt_j Wh_j) over the rows it finished, lane groups added in a fixed order.  Rows cut by a
 * slot border are finished by the fix-up launch and are NOT in the records: pygat_a_grad_fold adds them from the cut-row
 * list.  Needs ds (row sums known), a level of 8 heads x 16 in one window (the instantiation that keeps four waves per
 * SIMD with the sums; the others lose a wave to them and more time than the a-gradient pass costs) and a graph with a cut-row
 * list: pygat_gat_backward_col_da_bytes returns the size of da_part, 0 when the pass does not do it (then pygat_a_grad).
 * What it replaces: a launch that streams Wh, ds and dt again (0.6 GB, 0.12 ms at config 5). */
size_t pygat_gat_backward_col_da_bytes(const pygat_graph* gT, int H, int Fo, int head_group);
int pygat_gat_backward_col(const pygat_graph* gT, const int32_t* perm_t, int H, int Fo, float alpha,
                           const float* Wh, const float* a_pad, const float* GR,
                           const float* att_mask, const float* ds,
                           float* dWh, float* dt, float* dz_t, void* part, float* da_part, int h_first, int h_count,
                           int head_group, void* stream);
/* The two launches of pygat_gat_backward_col one by one (additive under ABI 16): phase = 0 (both: pygat_gat_backward_col),
 * PYGAT_F_MAIN_ONLY (the walk over the slots: rows that lie inside a slot are final after it, the pieces of cut rows are in
 * `part`) or PYGAT_F_FIXUP_ONLY (finishes the cut rows from `part`).  A single phase needs the level in one head window with
 * a list-driven fix-up: pygat_gat_backward_col_phases_ok(gT, H, F', head_group) == 1 (a graph with a cut-row list and no
 * slot_order; 0: not supported, negative: a bad graph or shape).  Same arguments as pygat_gat_backward_col otherwise. */
int pygat_gat_backward_col_phases_ok(const pygat_graph* gT, int H, int Fo, int head_group);
int pygat_gat_backward_col_phase(const pygat_graph* gT, const int32_t* perm_t, int H, int Fo, float alpha,
                                 const float* Wh, const float* a_pad, const float* GR,
                                 const float* att_mask, const float* ds,
                                 float* dWh, float* dt, float* dz_t, void* part, float* da_part, int h_first, int h_count,
                                 int head_group, int phase, void* stream);
/* The fix-up phase and the backward stream of the self-loop-only tail (pygat_gat_backward_tail, below) in ONE launch, after
 * pygat_gat_backward_col_phase(..., PYGAT_F_MAIN_ONLY) over the slot prefix gT: the leading work-groups finish the cut rows
 * from `part` (dWh_j, dt_j; ds is read for the ds_j a_src term), the ones behind them stream the rows [row_first, row_first +
 * n_rows): dWh_j = G_u ELU'(y_u) with u = user_row[j] (NULL: j), ds_j = dt_j = 0.  The two write disjoint rows (every cut row
 * lies before the tail) and neither reads what the other writes: no work-group waits for another, and each value is formed
 * exactly as by the two launches it replaces.  The fix-up is a few hundred latency-bound work-groups: resident beside the
 * stream they cost the step nothing, as a launch of their own they own a place in the sequence.  Needs
 * pygat_gat_backward_col_phases_ok == 1, a concat level without a skip projection, ds != NULL (the row-local backward);
 * flags: PYGAT_F_ELU or 0. */
int pygat_gat_backward_col_finish(const pygat_graph* gT, int H, int Fo, const float* a_pad, float* ds, float* dWh, float* dt,
                                  void* part, int head_group, int row_first, int n_rows, int flags, const float* G,
                                  const float* y, const int32_t* user_row, void* stream);
/* da [H x 2F'] from the records of a column pass that ran with da_part, plus the rows of gT's cut-row list (their ds, dt
 * and Wh rows are read here).  Same gT / head_group as that pass; ws >= pygat_agrad_workspace_bytes(H, F').  Fixed
 * summation order, no atomics: bitwise reproducible. */
int pygat_a_grad_fold(const pygat_graph* gT, int H, int Fo, const float* Wh, const float* ds, const float* dt,
                      const float* da_part, float* da, void* ws, int head_group, void* stream);
/* Row sums without the row pass.  The column pass computes every dz_ij anyway (for dt_j): called with ds = NULL
 * and dz_t [nnz x H] it writes them out per TRANSPOSED edge and leaves the ds_j a_src term out of dWh_j; then
 *   pygat_gat_backward_rowsum   ds_i = sum over the forward edges k of row i of dz_t[perm_f[k]]
 * replaces pygat_gat_backward_row: 4H-byte records per edge instead of a gathered Wh row (a quarter less HBM
 * traffic for the whole backward at 8 heads x 16), fixed summation order, still no atomics; and pygat_a_grad,
 * which streams Wh, ds, dt anyway, finishes dWh_i += ds_i a_src when given dWh.
 * g = forward pattern, perm_f[k] = position of forward edge k in gT.  part >= pygat_partials_bytes. */
int pygat_gat_backward_rowsum(const pygat_graph* g, const int32_t* perm_f, int H, int Fo, const float* dz_t,
                              float* ds, void* part, int h_first, int h_count, void* stream);
/* da[H x 2F'] : da_src = sum_i ds_i Wh_i, da_dst = sum_j dt_j Wh_j (per head).
 * ws >= pygat_agrad_workspace_bytes(H, Fo).  dWh (with a_pad) non-NULL: also dWh_i += ds_i a_src, see above. */
size_t pygat_agrad_workspace_bytes(int H, int Fo);
/* dwh_mask [n x R] (pre-scaled; needs dWh): dWh is also taken back through the Wh dropout of layers.py:37,136 in the same
 * pass (after the finishing term), instead of by a launch of its own. */
int pygat_a_grad(int n, int H, int Fo, const float* Wh, const float* ds, const float* dt,
                 float* da, void* ws, const float* a_pad, float* dWh, const float* dwh_mask, int h_first, int h_count,
                 void* stream);

/* Weight gradient of one level, the backward counterpart of pygat_project (autograd of layers.py:35,134):
 *   dW[h] = X^T dWh[:, head h]                       dW [H x Fin x F'], X [n x Fin], dWh [n x R]
 * With ds [n x H] (and a_pad) the dWh passed in still lacks its ds_i a_src term (pygat_gat_backward_col with
 * dz_t): X^T(dWh' + ds (x) a_src) = X^T dWh' + (X^T ds) (x) a_src, so ds rides along as H extra columns of the
 * same GEMM and the rank-1 terms are added while unpacking -- dWh is not read-modified-written for it (then
 * pygat_a_grad is called WITHOUT dWh).  ds = NULL: plain X^T dWh.
 * ws >= pygat_wgrad_workspace_bytes(Fin, H, F', split_k); split_k as in pygat_gemm_f32. */
size_t pygat_wgrad_workspace_bytes(int Fin, int H, int Fo, int split_k);
int pygat_wgrad(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const float* dWh, const float* ds,
                const float* a_pad, float* dW, int split_k, void* ws, int h_first, int h_count, int gemm_mode, void* stream);

/* The same with X column-blocked (pygat_col_blocks; NULL / w = 0: pygat_wgrad). */
int pygat_wgrad_blocked(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const pygat_col_blocks* x_blk,
                        const float* dWh, const float* ds, const float* a_pad, float* dW, int split_k, void* ws,
                        int h_first, int h_count, int gemm_mode, void* stream);

/* The weight gradient of a level whose self-loop-only tail [row_first, n) has NO dWh rows (additive under ABI 16): the streamed-K
 * split kernel reads dWh for the rows before row_first and forms the tail's rows itself, dWh_k = G_u ELU'(y_u) with u =
 * user_row[k] (NULL: k) -- pygat_gat_backward_tail's value, by the same single multiply; flags: PYGAT_F_ELU or 0 -- so the tail's
 * rows of dWh are neither written nor read (they may hold anything).  Same slabs, products and reduce as pygat_wgrad_blocked:
 * dW has the bits of pygat_gat_backward_tail + pygat_wgrad_blocked.  Workspace and split_k as there (no ds, all heads).
 * Returns 0 when it ran, 1 when NOT TAKEN -- nothing was launched, the caller runs that pair instead: whenever
 * pygat_wgrad_blocked would not run the streamed-K split kernel with its dW-writing reduce (fp32-mfma mode, a column-blocked X,
 * split_k <= 1, n < 4096, Fin or H F' <= 64 or not multiples of 4, operands or rows not 16-byte aligned), F' != Fp,
 * PYGAT_F_SKIP in flags, or a slab of more rows than the kernel's row-id table holds (about 16 000).  Negative: an error. */
int pygat_wgrad_tail_blocked(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const pygat_col_blocks* x_blk,
                             const float* dWh, float* dW, int split_k, void* ws, int row_first, int flags, const float* G,
                             const float* y, const int32_t* user_row, int gemm_mode, void* stream);

/* Self-loop-only nodes (ABI 14; csrc/k12_tail.hip).  A node whose only neighbour is itself has alpha_ii = 1: its forward is
 * h'_i = ELU(Wh_i (+ skip_i)), its backward dWh_i = Gp_i, ds_i = dt_i = 0 (layers.py:146-170 / 81-90 with one edge).  In a
 * degree-ordered pattern (pygat_graph.user_row != NULL) these nodes are the rows [row_first, row_first + n_rows) at the END of the
 * row range and their slots a suffix of the slot list: the caller runs pygat_gat_forward / pygat_gat_backward_col /
 * pygat_a_grad_fold on the slot PREFIX before them (pygat_graph.slot_first = 0, slot_count = the first tail slot; same struct for
 * all three) and these two streams on the tail.  Concat levels (out only), GR in ONE head window ([Gp R | records 4H] per row).
 * forward_tail also writes m = 0, Z = 1 (and qneg = 0) for the tail rows when given, so that pygat_gat_backward_prepare finds
 * finite records there. */
int pygat_gat_forward_tail(int row_first, int n_rows, int H, int Fo, int flags, const float* Wh, int64_t ldwh, const float* sk,
                           float* out, const int32_t* user_row, float* m, float* Z, float* qneg, void* stream);
/* (ldwh: row stride of Wh in floats, 0 = H*Fp; GATv2 passes its [Whi | Whj] table with 2 H Fp: h'_i = ELU(Whi_i (+ skip_i)),
 *  layers.py:296 with one edge) */
int pygat_gat_backward_col_tail(int row_first, int n_rows, int H, int Fo, const float* GR, float* dWh, float* dt, void* stream);
/* The tail's whole backward in one stream, for levels WITHOUT a skip projection (nothing else reads the tail's Gp): dWh_j =
 * G_u ELU'(out_u) with u = user_row[j], ds_j = dt_j = 0 (ds may be NULL); pygat_gat_backward_prepare is then called with
 * n = row_first (the rows before the tail) and the tail's rows of GR stay untouched.  Concat levels (y = the saved output). */
int pygat_gat_backward_tail(int row_first, int n_rows, int H, int Fo, int flags, const float* G, const float* y,
                            const int32_t* user_row, float* dWh, int64_t ld_dwh, int zero_cols, float* ds, float* dt, void* stream);
/* (ld_dwh: row stride of dWh, 0 = H*Fp; zero_cols: columns behind the H*Fp gradient columns of a row to clear -- GATv2: dWW_i =
 *  [Gp_i | 0] with ld_dwh = 2 H Fp, zero_cols = H Fp; ds, dt may be NULL) */

/* The tail's forward folded into the projection (ABI 15), for levels without a skip projection: pygat_project_blocked (Sk =
 * NULL) for the rows before row_first; for the rows [row_first, n) it writes out[user_row ? user_row[i] : i] = ELU(Wh_i) (flags:
 * PYGAT_F_ELU or 0) -- pygat_gat_forward_tail's output; m / Z / qneg are not touched -- and leaves Wh_i unspecified: on the
 * split-bf16 projection with s from the accumulators (F' = Fp of 8 / 16) the epilogue stores the output instead of Wh; any
 * other call projects every row and runs the tail stream after it.  Bitwise the same output either way. */
int pygat_project_tail_blocked(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const pygat_col_blocks* x_blk,
                               const float* Wcat, int64_t ldw, const float* a_pad, float* Wh, float* s, int split_k, void* ws,
                               int gemm_mode, int row_first, const int32_t* user_row, float* out, int flags, void* stream);

/* ------------------------------------------------ GATv2 (next row of the scope table)
 * The reference's SpGraphAttentionLayerV2 (layers.py:258-313): per head
 *   e_ij = a . LeakyReLU(Whi_i + Whj_j), alpha = row softmax, h'_i = sum_j alpha_ij Whi_j  (Whi is aggregated,
 *   layers.py:296).  WW [n x 2R] holds [Whi | Whj] rows (one projection GEMM with W[:Fin] and W[Fin:]),
 *   a2 [H x Fp] the zero-padded attention vectors.  Same outputs / flags / part as pygat_gat_forward.
 *   Limits: F' <= 256 per head as everywhere, and R = H * Fp <= 1024 (a [Whi | Whj] row of at most 2048 floats, never
 *   split into head windows); pygat_gatv2_forward / _backward return an error above that; GATv2LevelFn raises ValueError first.
 * (GraphAttentionLayerV2, layers.py:204-230, broadcasts one logit per ROW and is therefore a neighbour mean:
 *  it maps onto pygat_gat_forward with s = 0 and a = 0.)
 */
int pygat_gatv2_forward(const pygat_graph* g, int H, int Fo, float alpha, int flags,
                        const float* WW, const float* a2, const float* sk, const float* att_mask,
                        float* out, float* hattn, float* m, float* Z, void* part, void* stream);
/* GRW [n x (2R+4H)] = [Gp | (., m, 1/Z, D) per head | Whi]; G, y, sk, mean_mode as pygat_gat_backward_prepare. */
int pygat_gatv2_backward_prepare(int n, int H, int Fo, int flags, int mean_mode,
                                 const float* G, const float* y, const float* sk,
                                 const float* m, const float* Z, const float* WW, float* GRW, const int32_t* user_row,
                                 void* stream);   /* user_row: as in pygat_gat_backward_prepare */
/* Column pass over gT, then row pass over g:
 *   dWW [n x 2R] = [dWhi | dWhj], da [H x F'].  perm_t (transposed position -> forward edge) only indexes att_mask and may
 *   be NULL without one; perm_f (forward edge -> transposed position; the same array for a symmetric pattern) lets the row
 *   pass fetch the de_ij the column pass left per transposed edge.  ws >= pygat_gatv2_workspace_bytes. */
size_t pygat_gatv2_workspace_bytes(int64_t nnz, int slot_edges, int H, int Fo);
int pygat_gatv2_backward(const pygat_graph* g, const pygat_graph* gT, const int32_t* perm_t, const int32_t* perm_f,
                         int H, int Fo, float alpha, const float* WW, const float* a2, const float* GRW,
                         const float* att_mask, float* dWW, float* da, void* ws, void* stream);

/* ------------------------------------------------ K13: attention coefficients (ABI 16, csrc/k13_attention.hip)
 * att [nnz x H] fp32, head-contiguous per edge: att[k*H + h] = exp(e_ij - m_i) / Z_i for edge k = (i, j) of the CALLER's
 * pattern (rowptr [n+1], edge_rc [nnz][2] = (row, col) per edge, 8-byte aligned), the coefficient the forward normalised by,
 * taken after the x / Wh dropout masks (the tables carry them) and before the attention mask.
 *   v1:    e_ij = LeakyReLU(s_i + t_j),  t_j = Wh_j . a_dst  (a_pad [H][2][Fp] as for pygat_gat_forward);
 *   GATv2: e_ij = a . LeakyReLU(Whi_i + Whj_j),  WW [n x 2R] = [Whi | Whj], a2 [H x Fp]  (R = H * Fp <= 1024).
 * The tables (Wh / WW, s, m, Z) are the level's, as its forward left them, with n rows each; to_internal (NULL: identity)
 * maps a caller node to its table row when the level ran in an internal node order (CSRGraph.degree_ordered).  m, Z: the
 * row maxima and sums pygat_gat_forward / pygat_gatv2_forward wrote.  A row with exactly one edge gets exactly 1.0 and none
 * of its table rows is read (the self-loop-only tail: unwritten Wh rows with PYGAT_F_ELU fused into the projection, m / Z
 * fill values).  v1 scratch: t [n x H] floats; t is formed for the table rows [0, t_rows) only -- rows at and after t_rows
 * must be self-loop-only rows that no other row gathers (the tail of a symmetric degree-ordered pattern).  Edge-parallel,
 * no atomics, bitwise reproducible.  Memory is the caller's; alpha = the LeakyReLU slope. */
int pygat_gat_attention(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                        int H, int Fo, float alpha, const float* Wh, int64_t ldwh, const float* s, const float* a_pad,
                        const float* m, const float* Z, int t_rows, float* t, float* att, void* stream);
int pygat_gatv2_attention(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                          int H, int Fo, float alpha, const float* WW, const float* a2, const float* m, const float* Z,
                          float* att, void* stream);

/* ------------------------------------------------ K14: gradient through the attention coefficients (csrc/k14_alpha_grad.hip)
 * Additive under ABI 16 (no existing entry point changes).  A [nnz x H] = dL/d att of pygat_gat_attention, in the CALLER's edge
 * order; z_ij = s_i + t_j, l_ij = (z_ij > 0 ? 1 : alpha), att_ij recomputed from (s_i, t_j, m_i, Z_i) as K13 forms it:
 *   rows:  c_i = sum_k att_ik A_ik,  ds2_i = sum_j l_ij att_ij (A_ij - c_i)        over the forward pattern (rowptr, edge_rc);
 *          rec [n x H x 4] = (s_i, m_i, Z_i, c_i) per node and head, Z = 0 marking a row of at most one edge
 *   cols:  dt2_j = sum_i l_ij att_ij (A_ij - c_i)                                   over the transposed pattern (rowptr_t,
 *          edge_rc_t = (j, i) per transposed edge; a symmetric pattern passes its forward arrays), A of transposed edge k at row
 *          perm_t[k]; reads the rec the row pass left
 *   apply: dWh_q += ds2_q a_src + dt2_q a_dst for the table rows q < n_rows (a_pad [H][2][Fp], dWh [n_rows x H*Fp]).
 * The caller adds da through pygat_a_grad(ds2, dt2).  Tables (s, t, m, Z, rec, ds2, dt2) have n rows in the level's node order,
 * to_internal (NULL: identity) maps a caller node to its table row; t is the [n x H] table pygat_gat_attention left.  A row of
 * exactly one edge has att = 1, a constant: it contributes exactly zero, and neither its table rows nor its rows of A are read.
 * H <= 64.  Fo is only validated (1..256, as every entry point of a level does): the passes work on the per-head score tables and
 * never touch an F'-wide row.  Scratch, the caller's: rec n*H*4 floats (16-byte aligned); part >= the size
 * pygat_alpha_grad_workspace_bytes reports (both passes may share it): the partial records of the long rows (csrc/long_rows.h).
 * No float atomics, fixed summation order: bitwise reproducible.  alpha = the LeakyReLU slope. */
int pygat_alpha_grad_workspace_bytes(int64_t nnz, int H, size_t* bytes);   /* an error code like the launchers; additive under ABI 16 */
int pygat_alpha_grad_rows(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                          int H, int Fo, float alpha, const float* s, const float* t, const float* m, const float* Z,
                          const float* A, float* rec, float* ds2, float* part, void* stream);
int pygat_alpha_grad_cols(int n, int64_t nnz, const int32_t* rowptr_t, const int32_t* edge_rc_t, const int32_t* perm_t,
                          const int32_t* to_internal, int H, int Fo, float alpha, const float* t, const float* rec,
                          const float* A, float* dt2, float* part, void* stream);
int pygat_alpha_grad_apply(int n_rows, int H, int Fo, const float* a_pad, const float* ds2, const float* dt2, float* dWh,
                           void* stream);

/* ------------------------------------------------ K15: a per-edge logit term for the GAT level (csrc/k15_edge_logit.hip)
 * Additive under ABI 16 (no existing entry point changes).  u [nnz x H] in the CALLER's edge order (row k = edge k of
 * rowptr / edge_rc) enters the score in front of the LeakyReLU:
 *   z_ij = (s_i + t_j) + u_ij,  att_ij = softmax_j LeakyReLU(z_ij),  h'_i = sum_j att_ij Wh_j.
 *   forward   hattn [n x R] = h' (padded heads, pad columns 0), m, Z [n x H]; with PYGAT_F_ELU (a concat level) also
 *             out [n x H*F'] = ELU(h' (+ sk with PYGAT_F_SKIP)); a head-mean level runs pygat_head_mean(hattn, sk) afterwards.
 *             Online softmax in edge order.  A row of at most one edge gets (m, Z) = (0, 0): the mark every later pass tests.
 *   attention att [nnz x H] from (s, t, m, Z, u), one coefficient per edge and head; a marked row gets exactly 1.0.
 *   rows      Gp [n x R] = dL/d(h' + skip) (through the ELU from the saved output y with PYGAT_F_ELU, else G [n x F'] / H),
 *             D_i = Gp_i . h'_i, du_ij = l_ij att_ij (Gp_i . Wh_j - D_i) [nnz x H] = dL/du, ds_i = sum_j du_ij [n x H].
 *   cols      over the transposed pattern (rowptr_t, edge_rc_t = (j, i) per transposed edge, whose u / du row is perm_t[k]; a
 *             symmetric pattern passes its forward arrays): dt_j = sum_i du_ij, dWh_j = sum_i att_ij Gp_i + ds_j a_src + dt_j a_dst.
 * s, t [n x H] = Wh . a_src, Wh . a_dst (pygat_attn_scores); Wh [n x R] as the projection left it; all tables in the caller's node
 * order.  A row of exactly one edge has att = 1: its rows of u are never read and its du is exactly 0.  u_rows = rows of u (and
 * of att / du): it must equal nnz.  R = H * padded F' <= 1024.  ws >= the size pygat_gat_edge_workspace_bytes reports, 16-byte
 * aligned, the caller's (the three walking passes may share it): the partial records of the long rows (columns), merged in chunk
 * order (csrc/long_rows.h).  No float atomics: bitwise reproducible.  alpha = the LeakyReLU slope. */
int pygat_gat_edge_workspace_bytes(int64_t nnz, int H, int Fo, size_t* bytes);   /* an error code like the launchers: bad sizes are refused */
int pygat_gat_edge_forward(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo, float alpha,
                           int flags, const float* Wh, const float* s, const float* t, const float* sk, const float* u,
                           int64_t u_rows, float* out, float* hattn, float* m, float* Z, void* ws, void* stream);
int pygat_gat_edge_alpha(int n, int64_t nnz, const int32_t* edge_rc, int H, float alpha, const float* s, const float* t,
                             const float* m, const float* Z, const float* u, int64_t u_rows, float* att, void* stream);
int pygat_gat_edge_backward_rows(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo, float alpha,
                                 int flags, const float* Wh, const float* s, const float* t, const float* m, const float* Z,
                                 const float* u, int64_t u_rows, const float* G, const float* y, const float* hattn,
                                 float* Gp, float* du, float* ds, void* ws, void* stream);
int pygat_gat_edge_backward_cols(int n, int64_t nnz, const int32_t* rowptr_t, const int32_t* edge_rc_t, const int32_t* perm_t,
                                 int H, int Fo, float alpha, const float* s, const float* t, const float* m, const float* Z,
                                 const float* u, int64_t u_rows, const float* Gp, const float* du, const float* ds,
                                 const float* a_pad, float* dt, float* dWh, void* ws, void* stream);

/* ------------------------------------------------ K16: the inference forward on a bf16 feature table (csrc/k16_bf16_forward.hip)
 * Additive under ABI 16 (no existing entry point changes).  With Q = round-to-nearest-even from fp32 to bf16 the level is exactly
 * the fp32 level applied to the table Whq = Q(Wh): s_i = Whq_i . a_src and t_j = Whq_j . a_dst from the ROUNDED rows, logits,
 * LeakyReLU, online softmax, the weighted sum, skip and ELU in fp32, fp32 outputs.  Forward only (no backward exists).
 *   pack      Whq [n x R] (uint16 bf16 bit patterns, row stride R = H * padded F', padded columns 0, 16-byte aligned) and
 *             s [n x H] from the fp32 projection Wh (row stride ldwh >= R floats) and a_pad (pygat_pack_params).
 *   forward   the nnz split of pygat_gat_forward on the slots / slot_meta / cut_rows of g, a lane gathering 8 table elements
 *             (16 bytes; 4 at padded F' = 4): out [n x H*F'] = epilogue(h' (+ sk with PYGAT_F_SKIP)), ELU with PYGAT_F_ELU,
 *             and / or hattn [n x R] = h' (a head-mean level runs pygat_head_mean(hattn, sk) afterwards).  flags: PYGAT_F_ELU |
 *             PYGAT_F_SKIP only.  g must carry neither user_row (the pass writes row i) nor a slot range.  head_group: heads per
 *             pass, 0 = as many as a pass takes (rows of 1024 floats; 64 heads at padded F' = 4); more than that is refused.
 *             part >= the size pygat_gat_bf16_workspace_bytes reports for g's nnz and slot_edges, 16-byte aligned: two fp32
 *             records per slot for the rows a slot border cuts, merged in slot order.  No float atomics: bitwise reproducible. */
int pygat_gat_bf16_workspace_bytes(int64_t nnz, int slot_edges, int H, int Fo, size_t* bytes);   /* an error code like the launchers */
int pygat_gat_pack_bf16(int n, int H, int Fo, const float* Wh, int64_t ldwh, const float* a_pad, void* Whq, float* s, void* stream);
int pygat_gat_forward_bf16(const pygat_graph* g, int H, int Fo, float alpha, int flags, const void* Whq, const float* s,
                           const float* a_pad, const float* sk, float* out, float* hattn, int head_group, void* part, void* stream);

/* ------------------------------------------------ K17: the sparse-region SpMM as an op of its own (csrc/k17_spmm.hip)
 * Additive under ABI 16 (no existing entry point changes).  The reference's SpecialSpmmFunction (layers.py:70-95) for H heads:
 *   forward      out[i, h, f] = sum_{k in row i} val[perm[k], h] * b[col[k], h, f]  over a CSR pattern (rowptr [n_rows + 1], col
 *                [nnz]); perm[k] = the caller's entry index of CSR position k (NULL: k itself), val [nnz x H] in the CALLER's entry
 *                order.  Entries of a row are added in CSR order; repeated (row, col) pairs are separate entries and add.  A row
 *                without entries gets exact zeros.  The gradient with respect to b is this call on the transposed pattern (rowptr_t,
 *                row_t, perm_t) with G in place of b and n_cols in place of n_rows.
 *   grad_values  dval[k, h] = sum_f G[row_k, h, f] * b[col_k, h, f] for every entry k of edge_rc [nnz][2] = (row, col), the caller's
 *                order (8-byte aligned).  No pattern, no workspace.
 * Rows of b / out / G are H*F floats (heads side by side, NOT padded) with row strides ldb / ldo / ldg >= H*F.  16-byte loads are used
 * where F % 4 == 0 and the tables and their strides are 16-byte multiples, single floats otherwise: any F >= 1 is taken.  Limits,
 * refused with PYGAT_EINVAL: 1 <= H <= 64, F >= 1, H*F <= 1024, 0 <= nnz < 2^31 (n_rows, n_cols are ints).  col / edge_rc are NOT
 * range-checked: the caller validates its pattern once.  ws >= the size pygat_spmm_workspace_bytes reports, 16-byte aligned, the
 * caller's: the partial records of the long rows, added in chunk order (csrc/long_rows.h).  fp32, no float atomics, fixed summation
 * order: bitwise reproducible.  Nothing allocates or synchronises. */
int pygat_spmm_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes);   /* an error code like the launchers */
int pygat_spmm_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                       int H, int F, const float* val, const float* b, int64_t ldb, float* out, int64_t ldo,
                       void* ws, void* stream);
int pygat_spmm_grad_values(int64_t nnz, const int32_t* edge_rc, int H, int F, const float* G, int64_t ldg,
                           const float* b, int64_t ldb, float* dval, void* stream);

/* ------------------------------------------------ K18: a row softmax over per-entry logits as an op of its own (csrc/k18_edge_softmax.hip)
 * Additive under ABI 16 (no existing entry point changes).  The reference's layers.py:145-150,160 (attention dropout off) for H heads:
 * with i_k the group of entry k -- its row (side 0) or its column (side 1) --
 *   rows        m[i, h] = max_{k in group i} l[k, h],  Z[i, h] = sum_{k in group i} exp(l[k, h] - m[i, h])
 *   apply       alpha[k, h] = exp(l[k, h] - m[i_k, h]) / Z[i_k, h]
 *   grad_rows   c[i, h] = sum_{k in group i} alpha[k, h] G[k, h]
 *   grad_apply  dl[k, h] = alpha[k, h] (G[k, h] - c[i_k, h])
 * logits, alpha, G, dlogits are [nnz x H] in the CALLER's entry order.  rowptr [n_rows + 1] and perm [nnz] are the CSR of the grouping
 * side: perm[k] = the caller's entry index of CSR position k (NULL: k itself); pass the column-sorted pattern and its n_cols to group by
 * column.  The entry-parallel passes read the group of entry k from half `side` of edge_rc [nnz][2] = (row, col).  m, Z, c are
 * [n_rows x H]; a group without entries gets m = Z = c = 0.  A group of one entry gets alpha = 1.0 and dl = 0.0 exactly.  Logits are
 * finite floats of any magnitude.  Limits, refused with PYGAT_EINVAL: 1 <= H <= 64, 0 <= nnz < 2^31, side 0 or 1, n_rows < 0 or
 * n_rows == 0 with entries, null pointers (perm excepted; the message names the pointer); nnz == 0 is a successful no-op.  perm / edge_rc are NOT range-checked: the caller validates its pattern once.
 * ws >= the size pygat_edge_softmax_workspace_bytes reports = 5 records of 2 H floats per 2048-entry chunk, 16-byte aligned, the caller's
 * (both group passes may share it): the partial (m, Z) or c records of the long rows, merged in chunk order (csrc/long_rows.h).  fp32, no
 * float atomics, fixed summation order: bitwise reproducible.  Nothing allocates or synchronises. */
int pygat_edge_softmax_workspace_bytes(int64_t nnz, int H, size_t* bytes);   /* an error code like the launchers */
int pygat_edge_softmax_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* perm, int H,
                            const float* logits, float* m, float* Z, void* ws, void* stream);
int pygat_edge_softmax_apply(int64_t nnz, const int32_t* edge_rc, int side, int H, const float* logits,
                             const float* m, const float* Z, float* alpha, void* stream);
int pygat_edge_softmax_grad_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* perm, int H,
                                 const float* alpha, const float* G, float* c, void* ws, void* stream);
int pygat_edge_softmax_grad_apply(int64_t nnz, const int32_t* edge_rc, int side, int H, const float* alpha,
                                  const float* G, const float* c, float* dlogits, void* stream);

/* ------------------------------------------------ K19: fused dot-product attention over an edge pattern (csrc/k19_dot_attention.hip)
 * Additive under ABI 16 (no existing entry point changes).  For H heads, over a CSR pattern (rowptr [n_rows + 1], col [nnz]):
 *   forward        s[e, h] = scale <q[i, h], k[j, h]> for entry e = (i, j);  out[i, h, :] = sum_{e in row i} softmax_row(s)[e, h] v[j, h, :]
 *                  in one pass (an online softmax: nothing per entry is written);  m[i, h] = max_e s[e, h],  Z[i, h] = sum_e exp(s[e, h] -
 *                  m[i, h]), [n_rows x H], always written: with out they are all backward_rows needs.
 *   backward_rows  D[i, h] = <G[i, h], out[i, h]>,  p = exp(s - m[i, h]) / Z[i, h],  ds = scale p (<G[i, h], v[j, h]> - D[i, h]);
 *                  dq[i, h, :] = sum_{e in row i} ds k[j, h, :];  P[e, h] = p and S[e, h] = ds, [nnz x H] in the CALLER's entry order
 *                  (perm[k] = the caller's entry index of CSR position k, NULL: k itself).  The column side is K17 on the transposed
 *                  pattern: dk = pygat_spmm_forward(val = S, b = q), dv = pygat_spmm_forward(val = P, b = G).
 * Rows of q / out / G / dq (n_rows of them) and of k / v are H*F floats, heads side by side, NOT padded, 16-byte aligned, with row
 * strides >= H*F that are multiples of 4 floats.  Repeated (row, col) pairs are separate entries.  A row without entries gets out = m = Z
 * = dq = 0 exactly and its G row is not read; a row of one entry (i, j) gets out_i = v_j bit for bit, p = 1 and ds = dq_i = 0 exactly.
 * Limits, refused with PYGAT_EINVAL before anything is launched: 1 <= H <= 64, F a power of two in 4..256 (zero-padding the columns of
 * q, k and v to the next allowed F leaves the first F columns of the result unchanged), H*F <= 1024, 0 <= nnz < 2^31, null or misaligned
 * tables (the message names the argument), short strides.  col / perm are NOT range-checked: the caller validates its pattern once.
 * ws >= the size pygat_dot_attn_workspace_bytes reports = 5 records of H*F + 2 H floats (rounded up to 4) per 2048-entry chunk,
 * 16-byte aligned, the caller's (both launchers may share it): the partial (acc, m, Z) or dq records of the long rows, merged in chunk
 * order (csrc/long_rows.h).  fp32, no float atomics, fixed summation order: bitwise reproducible.  Nothing allocates or synchronises. */
int pygat_dot_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes);   /* an error code like the launchers */
int pygat_dot_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F, float scale,
                                const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_dot_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                      int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                      const float* v, int64_t ldv, const float* out, int64_t ldo, const float* m, const float* Z,
                                      const float* G, int64_t ldg, float* dq, int64_t lddq, float* P, float* S, void* ws,
                                      void* stream);
/* The same two with a per-entry term on the score (the BIAS instantiations of the K19 kernels), additive under ABI 16:
 *   s[e, h] = scale <q[i, h], k[j, h]> + bias[c(e) * (bias_head_stride ? H : 1) + h * bias_head_stride],
 * c(e) the CALLER's entry index of CSR position e (perm[e]; perm may be null: the position itself), as P and S are addressed.
 * bias_head_stride 1: bias [nnz x H]; 0: bias [nnz], one value per entry shared by the heads.  Both launchers take the softmax's
 * difference as (scale <q, k>) - (m - bias), the expression of the pair above with the bias on the maximum's side: under a bias of zeros
 * out, dq, P and S are theirs bit for bit.  m and Z are those of the biased scores.  bias is read with 4-byte loads (no alignment beyond 4
 * bytes), must be finite and is not checked; a large negative finite value (-9e15) masks an entry exactly -- p = 0, no share of out,
 * exact zeros in dq, P, S and dbias -- while its row keeps an unmasked entry.  backward_rows also forms dbias[c(e), h] = p (<G[i, h],
 * v[j, h]> - D[i, h]), always [nnz x H] (the gradient of a [nnz] bias is its sum over h, the caller's), stored only where dbias is not
 * null; dq, P and S keep their formulas and, under a bias of zeros, their bits.  Refusals as above after the launcher's own name;
 * besides: a null bias with nnz > 0, a bias_head_stride other than 0 or 1.  The workspace and its size query are unchanged. */
int pygat_dot_attn_bias_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                     int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                     int64_t ldv, const float* bias, int bias_head_stride, float* out, int64_t ldo, float* m,
                                     float* Z, void* ws, void* stream);
int pygat_dot_attn_bias_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                           int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                           const float* v, int64_t ldv, const float* bias, int bias_head_stride, const float* out,
                                           int64_t ldo, const float* m, const float* Z, const float* G, int64_t ldg, float* dq,
                                           int64_t lddq, float* P, float* S, float* dbias, void* ws, void* stream);
/* The forward on bf16 k and v tables, for inference (the bf16-table instantiations of the two K19 forward kernels), additive under
 * ABI 16.  k and v are rows of H*F bf16 values, 8-byte aligned, ldk and ldv in ELEMENTS, >= H*F and multiples of 4; q, out and ws as
 * above (fp32, 16 bytes).  A lane's chunk is the same 4 row elements as in the fp32 kernels, one 8-byte load widened in registers, and
 * everything after the load is theirs: out is pygat_dot_attn_forward's (pygat_dot_attn_bias_forward's) on the widened tables bit for
 * bit, at 4 H*F + 4 gathered bytes per entry instead of 8 H*F + 4.  bias may be null: no bias, perm and bias_head_stride are then
 * not looked at; otherwise as in pygat_dot_attn_bias_forward.  m and Z are not written: there is no backward on bf16 tables.
 * Refusals as above after the launcher's own name.  The workspace and its size query are unchanged. */
int pygat_dot_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                     int F, float scale, const float* q, int64_t ldq, const void* k, int64_t ldk, const void* v,
                                     int64_t ldv, const float* bias, int bias_head_stride, float* out, int64_t ldo, void* ws,
                                     void* stream);
/* The bias pair with seeded dropout of the softmax coefficients, for training (the DROP instantiations of the four fp32 K19 kernels),
 * additive under ABI 16:
 *   out[i, h, :] = sum_{e in row i} alpha[e, h] mask[c(e), h] v[j, h, :],   alpha = softmax_row(scale <q, k> + bias) over ALL entries of
 * the row -- a dropped entry stays in the denominator; m and Z are the undropped softmax's -- mask in {0, 1 / (1 - p)}, c(e) the CALLER's
 * entry index (perm[e]; perm may be null: the position itself).  mask[c, h] is element idx = c H + h of the flat layout of
 * pygat_dropout_mask: word (idx & 3) of Philox-4x32-10(counter = (idx >> 2 low word, idx >> 2 high word, stream_id, 0xFFFFFFFF), key =
 * *seed), kept iff word < the threshold of p; pygat_dropout_mask(nnz H, p, seed, stream_id, ...) writes the same table.  The decision is
 * drawn in registers in the forward and again in backward_rows: no mask is stored.  seed is a uint64 in DEVICE memory, read by the
 * kernels (nothing is read back; a captured graph replays with the seed found there).  backward_rows: D = <G, out>, ds = scale p (mask
 * <G, v> - D), dbias = p (mask <G, v> - D), P := p mask and S := ds, so dk = pygat_spmm_forward(val = S, b = q) and dv =
 * pygat_spmm_forward(val = P, b = G) as above.  bias may be null: no bias, bias_head_stride is then not looked at (dbias is not
 * written).  A row of one entry gets out_i = mask v_j bit for bit; a row whose entries are all dropped, and every row at p = 1, exact
 * zeros.  Refusals as for the bias pair after the launcher's own name; besides: a null or misaligned (8 bytes) seed, p outside [0, 1]
 * (a NaN included).  Both launchers must be given the same p, seed value and stream_id.  The workspace and its size query are unchanged. */
int pygat_dot_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                   int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                   int64_t ldv, const float* bias, int bias_head_stride, float p, const void* seed,
                                   uint32_t stream_id, float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_dot_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                         int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                         const float* v, int64_t ldv, const float* bias, int bias_head_stride, float p,
                                         const void* seed, uint32_t stream_id, const float* out, int64_t ldo, const float* m,
                                         const float* Z, const float* G, int64_t ldg, float* dq, int64_t lddq, float* P, float* S,
                                         float* dbias, void* ws, void* stream);
/* The bias pair with a feature row per entry on the key and the value side (the EDGE instantiations of the four fp32 K19 kernels),
 * additive under ABI 16:
 *   s[e, h] = scale <q[i, h], k[j, h] + ee[c(e), h]> + bias,   out[i, h, :] = sum_{e in row i} softmax_row(s)[e, h] (v[j, h, :] + ee[c(e), h, :]),
 * ee = the argument e, [nnz x H*F] floats, a row table like k and v (16-byte aligned, lde >= H*F and a multiple of 4), c(e) the CALLER's
 * entry index of CSR position e (perm[e]; perm may be null: the position itself).  A lane reads its 16 bytes of the entry's row with the
 * k and v rows of the entry.  kk = k_j + ee_c and vv = v_j + ee_c are one rounded add per element, formed the same way by both
 * launchers, and everything after sees kk and vv where the pairs above see k_j and v_j: with ee = 0, out, dq, P and S have their
 * values.  backward_rows: dp = <G_i, vv>, D = <G_i, out_i>, ds = scale p (dp - D), dq_i = sum_e ds kk, P := p and S := ds, so dk =
 * pygat_spmm_forward(val = S, b = q) and dv = pygat_spmm_forward(val = P, b = G) as above, and the gradient of ee, row-local:
 * de[c(e), h, :] = ds q[i, h, :] + p G[i, h, :], [nnz x H*F] with row stride ldde, a row table like e.  Every row of de is written
 * exactly once (an entry belongs to one row, in a long row to one piece): nothing is zeroed or accumulated.  de may be null: not asked
 * for, ldde is then not looked at.  bias may be null: no bias, bias_head_stride is then not looked at (dbias is not written);
 * otherwise as in the bias pair, dbias = p (dp - D).  A row of one entry (i, j) gets out_i = v_j + ee_c and de_c = G_i bit for bit, p
 * = 1 and ds = dq_i = 0 exactly; a masked entry (bias -9e15) gets an all-zero row of de.  Refusals as for the bias pair after the
 * launcher's own name; besides: a null e with nnz > 0, a misaligned e or de, a short or odd lde or ldde.  The workspace and its size
 * query are unchanged. */
int pygat_dot_attn_edge_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                int64_t ldv, const float* e, int64_t lde, const float* bias, int bias_head_stride, float* out,
                                int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_dot_attn_edge_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                      int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                      const float* v, int64_t ldv, const float* e, int64_t lde, const float* bias,
                                      int bias_head_stride, const float* out, int64_t ldo, const float* m, const float* Z,
                                      const float* G, int64_t ldg, float* dq, int64_t lddq, float* P, float* S, float* de,
                                      int64_t ldde, float* dbias, void* ws, void* stream);

/* ------------------------------------------------ K20: the GAT score fused over an edge pattern (csrc/k20_additive_attention.hip)
 * Additive under ABI 16 (no existing entry point changes).  For H heads, over a CSR pattern (rowptr [n_rows + 1], col [nnz]) whose row
 * side and column side are different tables, s_dst [n_rows x H] and s_src [n_cols x H] (dense, 4-byte loads) and v [n_cols x H*F]:
 *   forward        z[e, h] = s_dst[i, h] + s_src[j, h] for entry e = (i, j), one rounded add;  with edge_logit: z = (s_dst[i, h] +
 *                  s_src[j, h]) + edge_logit[c(e) * (logit_head_stride ? H : 1) + h * logit_head_stride], two rounded adds in this
 *                  order, c(e) the CALLER's entry index of CSR position e (perm[e]; perm may be null: the position itself);
 *                  l = z > 0 ? z : negative_slope z;  out[i, h, :] = sum_{e in row i} softmax_row(l)[e, h] v[j, h, :] in one pass (an
 *                  online softmax: nothing per entry is written);  m[i, h] = max_e l[e, h],  Z[i, h] = sum_e exp(l[e, h] - m[i, h]),
 *                  [n_rows x H], always written: with out they are all backward_rows needs.
 *   backward_rows  D[i, h] = <G[i, h], out[i, h]>,  p = exp(l - m[i, h]) / Z[i, h],  dz = p (<G[i, h], v[j, h]> - D[i, h]) (z > 0 ? 1 :
 *                  negative_slope);  ds_dst[i, h] = sum_{e in row i} dz, [n_rows x H];  P[c(e), h] = p and S[c(e), h] = dz, [nnz x H] in
 *                  the CALLER's entry order.  S is the gradient of edge_logit ([nnz x H]; of a [nnz] one its sum over h, the
 *                  caller's).  The column side is K17 on the transposed pattern: dv = pygat_spmm_forward(val = P, b = G), ds_src =
 *                  pygat_spmm_forward(val = S, b = ones [n_rows x H x 1]).
 * edge_logit == NULL selects the kernels without the term: they carry no entry index through their walk, the forward does not read
 * perm, and logit_head_stride is not looked at; perm may be null then, and for a pattern in CSR order.  logit_head_stride 1:
 * edge_logit [nnz x H]; 0: [nnz], one value per entry shared by the heads.  An edge_logit of zeros changes no bit of out, ds_dst, P or S.
 * Its values must be finite and are not checked; a large negative finite one (-9e15) masks an entry exactly -- p = 0, no share of out,
 * exact zeros in P and S -- while its row keeps another entry and negative_slope > 0 (at slope 0, l = 0: no mask).
 * Rows of v / out / G are H*F floats, heads side by side, NOT padded, 16-byte aligned, with row strides >= H*F that are multiples of 4
 * floats.  Repeated (row, col) pairs are separate entries.  A row without entries gets out = m = Z = ds_dst = 0 exactly and its G row is
 * not read; a row of one entry (i, j) gets out_i = v_j bit for bit and dz = 0 exactly.  Limits, refused with PYGAT_EINVAL before
 * anything is launched: 1 <= H <= 64, F a power of two in 4..256 (zero-padding the columns of v to the next allowed F leaves the
 * first F columns of the result unchanged), H*F <= 1024, 0 <= nnz < 2^31, a negative_slope that is not finite, null or misaligned
 * tables (the message names the argument), short strides, a logit_head_stride other than 0 or 1.  col / perm are NOT range-checked.
 * ws >= the size pygat_add_attn_workspace_bytes reports = 5 records of H*F + 2 H floats (rounded up to 4) per 2048-entry chunk,
 * 16-byte aligned, the caller's (both launchers may share it): the partial (acc, m, Z) records, or the H sums of dz, of the long rows,
 * merged in chunk order (csrc/long_rows.h).  fp32, no float atomics, fixed summation order: bitwise reproducible.  Nothing allocates or
 * synchronises. */
int pygat_add_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes);   /* an error code like the launchers */
int pygat_add_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H, int F,
                           float negative_slope, const float* s_dst, const float* s_src, const float* v, int64_t ldv,
                           const float* edge_logit, int logit_head_stride, float* out, int64_t ldo, float* m, float* Z, void* ws,
                           void* stream);
int pygat_add_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                 int F, float negative_slope, const float* s_dst, const float* s_src, const float* v, int64_t ldv,
                                 const float* edge_logit, int logit_head_stride, const float* out, int64_t ldo, const float* m,
                                 const float* Z, const float* G, int64_t ldg, float* ds_dst, float* P, float* S, void* ws,
                                 void* stream);
/* The K20 pair with seeded dropout of the softmax coefficients, for training (the DROP instantiations of the four K20 kernels), additive
 * under ABI 16:
 *   out[i, h, :] = sum_{e in row i} alpha[e, h] mask[c(e), h] v[j, h, :],   alpha = softmax_row(l) over ALL entries of the row -- a
 * dropped entry stays in the denominator; m and Z are the undropped softmax's -- mask in {0, 1 / (1 - p)}, c(e) the CALLER's entry index
 * (perm[e]; perm may be null: the position itself).  The mask is pygat_dot_attn_dropout_forward's: mask[c, h] is element idx = c H + h
 * of the flat layout of pygat_dropout_mask, word (idx & 3) of Philox-4x32-10(counter = (idx >> 2 low word, idx >> 2 high word,
 * stream_id, 0xFFFFFFFF), key = *seed), kept iff word < the threshold of p; pygat_dropout_mask(nnz H, p, seed, stream_id, ...) writes
 * the same table, and one seed gives the same mask in K19, K20 and K21.  The decision is drawn in registers in the forward and again in
 * backward_rows: no mask is stored.  Under dropout the walk carries the entry index in both passes, so the forward reads perm whether or
 * not there is an edge_logit; without one it loads no logit.  seed is a uint64 in DEVICE memory, read by the kernels (nothing is read
 * back; a captured graph replays with the seed found there).  backward_rows: D = <G, out>, dp = mask <G, v>, dz = p (dp - D) (z > 0 ?
 * 1 : negative_slope), ds_dst = sum dz, P := p mask and S := dz, so dv = pygat_spmm_forward(val = P, b = G), ds_src =
 * pygat_spmm_forward(val = S, b = ones) and S is the gradient of edge_logit as above.  edge_logit may be null: no term,
 * logit_head_stride is then not looked at; an edge_logit of zeros changes no bit against the DROP kernels without it.  A row of one
 * entry gets out_i = mask v_j bit for bit; its dz is an exact zero where the entry is dropped and where mask is a power of two (p =
 * 0.5: mask dp and D are then the same bits), and otherwise the difference of two roundings, mask <G, v> against <G, mask v>: a few
 * ulps of dp, not zero.  A row whose entries are all dropped, and every row at p = 1, get exact zeros in out.  Refusals as for the
 * K20 pair after the launcher's own name; besides: a null or misaligned (8 bytes) seed, p outside [0, 1] (a NaN included).  Both
 * launchers must be given the same p, seed value and stream_id.  The workspace is pygat_add_attn_workspace_bytes'. */
int pygat_add_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                   int F, float negative_slope, const float* s_dst, const float* s_src, const float* v, int64_t ldv,
                                   const float* edge_logit, int logit_head_stride, float p, const void* seed, uint32_t stream_id,
                                   float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_add_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                         int H, int F, float negative_slope, const float* s_dst, const float* s_src, const float* v,
                                         int64_t ldv, const float* edge_logit, int logit_head_stride, float p, const void* seed,
                                         uint32_t stream_id, const float* out, int64_t ldo, const float* m, const float* Z,
                                         const float* G, int64_t ldg, float* ds_dst, float* P, float* S, void* ws, void* stream);
/* The K20 forward on a bf16 v table, for inference (the BF16 instantiations of the two K20 forward kernels), additive under ABI 16.  v is
 * rows of H*F bf16 values, 8-byte aligned, ldv in ELEMENTS, >= H*F and a multiple of 4; s_dst, s_src, edge_logit, out and ws as in
 * pygat_add_attn_forward (fp32; out and ws 16 bytes).  A lane's chunk is the same 4 row elements as in the fp32 kernels, one 8-byte load
 * widened in registers, and everything after the load is theirs: out is pygat_add_attn_forward's on the widened table bit for bit, at
 * 2 H*F + 4 H + 4 gathered bytes per entry instead of 4 H*F + 4 H + 4.  edge_logit may be null: the kernels without the term, perm and
 * logit_head_stride are then not looked at; otherwise as in pygat_add_attn_forward.  m and Z are neither taken nor written: there is no
 * backward on a bf16 table.  Refusals as for pygat_add_attn_forward after the launcher's own name (v: 8-byte aligned).  The workspace
 * is pygat_add_attn_workspace_bytes'. */
int pygat_add_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H, int F,
                                float negative_slope, const float* s_dst, const float* s_src, const void* v, int64_t ldv,
                                const float* edge_logit, int logit_head_stride, float* out, int64_t ldo, void* ws, void* stream);

/* ------------------------------------------------ K21: the GATv2 score fused over an edge pattern (csrc/k21_gatv2_attention.hip)
 * Additive under ABI 16 (no existing entry point changes).  For H heads, over a CSR pattern (rowptr [n_rows + 1], col [nnz]) whose row
 * side and column side are different tables, x_dst [n_rows x H*F] and x_src [n_cols x H*F], an attention vector a [H x F] (dense)
 * and a value table v [n_cols x H*F]; v == NULL: v is x_src, the gathered row serves the score and the sum (one gather per entry):
 *   forward        t[f] = x_dst[i, h, f] + x_src[j, h, f] for entry e = (i, j), one rounded add;  g[f] = t[f] > 0 ? t[f] :
 *                  negative_slope t[f];  s[e, h] = sum_f a[h, f] g[f] in a fixed order;  out[i, h, :] = sum_{e in row i}
 *                  softmax_row(s)[e, h] v[j, h, :] in one pass (an online softmax: nothing per entry is written);  m[i, h] = max_e
 *                  s[e, h],  Z[i, h] = sum_e exp(s[e, h] - m[i, h]), [n_rows x H], always written: with out they are all the backward needs.
 *   backward_rows  D[i, h] = <G[i, h], out[i, h]>,  p = exp(s - m[i, h]) / Z[i, h],  S = p (<G[i, h], v[j, h]> - D[i, h]);
 *                  dx_dst[i, h, f] = sum_{e in row i} S a[h, f] (t[f] > 0 ? 1 : negative_slope);  P[c(e), h] = p and S[c(e), h] = S,
 *                  [nnz x H] in the CALLER's entry order, c(e) = perm[e] (perm may be null: the position itself).
 *   backward_cols  on the transposed pattern (rowptr_t [n_cols + 1], row_t [nnz], perm_t [nnz] | null), S as backward_rows left it:
 *                  dx_src[j, h, f] = sum_{e in column j} S[c(e), h] a[h, f] (t[f] > 0 ? 1 : negative_slope);  da[h, f] = sum over
 *                  ALL entries of S[c(e), h] g[f], reduced from per-wave records in a fixed order.  Both are always written.
 *   dv = pygat_spmm_forward(val = P, b = G) on the transposed pattern (K17), the caller's launch; with v == NULL the caller adds it
 *   to dx_src.
 * Rows of x_dst / x_src / v / out / G / dx_dst / dx_src are H*F floats, heads side by side, NOT padded, 16-byte aligned, with row
 * strides >= H*F that are multiples of 4 floats; a and da are 16-byte aligned.  Repeated (row, col) pairs are separate entries.  A
 * row without entries gets out = m = Z = dx_dst = 0 exactly and its G row is not read; a column without entries gets dx_src = 0; a
 * row of one entry (i, j) gets out_i = v_j bit for bit and S = 0 exactly.  Limits, refused with PYGAT_EINVAL before anything is
 * launched: 1 <= H <= 64, F a power of two in 4..256 (zero-padding the columns of x_dst, x_src, a and v to the next allowed F leaves
 * the first F columns of the result unchanged: zero columns of a add nothing to a score), H*F <= 1024, 0 <= nnz < 2^31, a
 * negative_slope that is not finite, null or misaligned tables (the message names the argument), short strides.  col / perm are NOT
 * range-checked.  ws >= the size pygat_v2_attn_workspace_bytes reports, 16-byte aligned, the caller's (the three launchers may share
 * it): 5 records of H*F + 2 H floats (rounded up to 4) per 2048-entry chunk -- the partial (acc, m, Z) records, or the H*F sums of
 * dx, of the long rows and long columns, merged in chunk order (csrc/long_rows.h) -- and the da records of backward_cols: H*F floats,
 * five per 2048-entry chunk (one of the long-column kernel, four of the column kernel, whose work-groups take a chunk's columns
 * each; four for a pattern without entries) and one per partial sum of the reduce (128).  fp32, no float
 * atomics, no LDS, fixed summation order: bitwise reproducible.  Nothing allocates or synchronises. */
int pygat_v2_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes);   /* an error code like the launchers */
int pygat_v2_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F, float negative_slope,
                          const float* x_dst, int64_t ldd, const float* x_src, int64_t lds, const float* a, const float* v,
                          int64_t ldv, float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_v2_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds,
                                const float* a, const float* v, int64_t ldv, const float* out, int64_t ldo, const float* m,
                                const float* Z, const float* G, int64_t ldg, float* dx_dst, int64_t lddx, float* P, float* S,
                                void* ws, void* stream);
int pygat_v2_attn_backward_cols(int n_cols, int64_t nnz, const int32_t* rowptr_t, const int32_t* row_t, const int32_t* perm_t,
                                int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                int64_t lds, const float* a, const float* S, float* dx_src, int64_t lddx, float* da, void* ws,
                                void* stream);
/* The two K21 row passes with seeded dropout of the softmax coefficients, for training (the DROP instantiations of the forward and
 * backward_rows kernels), additive under ABI 16:
 *   out[i, h, :] = sum_{e in row i} alpha[e, h] mask[c(e), h] v[j, h, :],   alpha = softmax_row(s) over ALL entries of the row -- a
 * dropped entry stays in the denominator; m and Z are the undropped softmax's -- mask in {0, 1 / (1 - p)}, the mask of
 * pygat_dot_attn_dropout_forward and pygat_add_attn_dropout_forward: element c(e) H + h of the flat layout
 * pygat_dropout_mask(nnz H, p, seed, stream_id, ...) writes, drawn in registers in the forward and again in backward_rows; no mask is
 * stored.  c(e) is the CALLER's entry index, so the forward takes perm (after col; it may be null: the position itself), which
 * pygat_v2_attn_forward never reads.  seed is a uint64 in DEVICE memory, read by the kernels.  backward_rows: D = <G, out>, S = p (mask
 * <G, v> - D), dx_dst from S as above, P := p mask, so dv = pygat_spmm_forward(val = P, b = G).  pygat_v2_attn_backward_cols reads S
 * alone: it is launched as it is and has no dropout variant.  v == NULL as above.  A row of one entry gets out_i = mask v_j bit for
 * bit; its S is an exact zero where the entry is dropped and where mask is a power of two (p = 0.5), and otherwise the difference of
 * two roundings, mask <G, v> against <G, mask v>: a few ulps of dp, not zero.  A row whose entries are all dropped, and every row at
 * p = 1, get exact zeros in out.  Refusals as for the K21 launchers after the launcher's own name; besides: a null or misaligned (8
 * bytes) seed, p outside [0, 1] (a NaN included).  Both launchers must be given the same p, seed value and stream_id.  The workspace
 * is pygat_v2_attn_workspace_bytes'. */
int pygat_v2_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                  int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds,
                                  const float* a, const float* v, int64_t ldv, float p, const void* seed, uint32_t stream_id,
                                  float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream);
int pygat_v2_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                        int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                        int64_t lds, const float* a, const float* v, int64_t ldv, float p, const void* seed,
                                        uint32_t stream_id, const float* out, int64_t ldo, const float* m, const float* Z,
                                        const float* G, int64_t ldg, float* dx_dst, int64_t lddx, float* P, float* S, void* ws,
                                        void* stream);
/* The three K21 passes with a feature row per entry inside the score (the EDGE instantiations of the K21 kernels), additive under ABI
 * 16:
 *   t[f] = (x_dst[i, h, f] + x_src[j, h, f]) + ee[c(e), h, f], two rounded adds in this order, the same bits in all three launchers;
 *   g, s, m, Z and out from t as above: ee enters the score alone, out stays the sum over v (PyG's GATv2Conv with edge_dim).
 * ee = the argument e, [nnz x H*F] floats, a row table like x_src (16-byte aligned, lde >= H*F and a multiple of 4), c(e) the CALLER's
 * entry index of CSR position e, so the forward takes perm (after col; it may be null: the position itself).  A lane reads its 16
 * bytes of the entry's row with the gathered rows of the entry.  backward_rows: D, S, P and dx_dst as above, and the gradient of ee,
 * row-local: de[c(e), h, f] = S a[h, f] (t[f] > 0 ? 1 : negative_slope), the term dx_dst sums over the row, [nnz x H*F] with row
 * stride ldde, a row table like e.  Every row of de is written exactly once (an entry belongs to one row, in a long row to one
 * piece): nothing is zeroed or accumulated, no atomics.  de may be null: not asked for, ldde is then not looked at.  backward_cols
 * takes e beside S (perm_t places both) and forms dx_src and da from the same t; it does not write de.  v == NULL as above.  With ee =
 * 0 every output has the bits of the launchers without it.  A row of one entry (i, j) gets out_i = v_j bit for bit, S = 0 exactly and
 * an all-zero row of de.  There is no dropout variant.  Refusals as for the K21 launchers after the launcher's own name; besides: a
 * null e with nnz > 0, a misaligned e or de, a short or odd lde or ldde, in the words of pygat_dot_attn_edge_forward.  The workspace
 * and its size query are unchanged. */
int pygat_v2_attn_edge_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H, int F,
                               float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds, const float* a,
                               const float* v, int64_t ldv, const float* e, int64_t lde, float* out, int64_t ldo, float* m, float* Z,
                               void* ws, void* stream);
int pygat_v2_attn_edge_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                     int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds,
                                     const float* a, const float* v, int64_t ldv, const float* e, int64_t lde, const float* out,
                                     int64_t ldo, const float* m, const float* Z, const float* G, int64_t ldg, float* dx_dst,
                                     int64_t lddx, float* P, float* S, float* de, int64_t ldde, void* ws, void* stream);
int pygat_v2_attn_edge_backward_cols(int n_cols, int64_t nnz, const int32_t* rowptr_t, const int32_t* row_t, const int32_t* perm_t,
                                     int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                     int64_t lds, const float* a, const float* e, int64_t lde, const float* S, float* dx_src,
                                     int64_t lddx, float* da, void* ws, void* stream);
/* The K21 forwards on bf16 tables, for inference (the BF16 instantiations of the two K21 forward kernels, without and with EDGE),
 * additive under ABI 16.  x_src, v and (the edge launcher) e are rows of H*F bf16 values, 8-byte aligned, lds, ldv and lde in ELEMENTS,
 * >= H*F and multiples of 4; x_dst, a, out and ws as in pygat_v2_attn_forward (fp32, 16 bytes).  v == NULL: v is x_src, the one gathered
 * row, widened once, serves the score and the sum.  A lane's chunk is the same 4 row elements as in the fp32 kernels, one 8-byte load
 * widened in registers, and everything after the load is theirs: out is pygat_v2_attn_forward's (pygat_v2_attn_edge_forward's) on the
 * widened tables bit for bit, at half the gathered and per-entry row bytes.  pygat_v2_attn_bf16_forward takes no perm, as
 * pygat_v2_attn_forward; the edge launcher takes it (it may be null: the position itself): the entry index places the rows of e.  m
 * and Z are neither taken nor written: there is no backward on bf16 tables, and no dropout variant.  Refusals as for the fp32 forward
 * launchers after the launcher's own name (x_src, v, e: 8-byte aligned).  The workspace is pygat_v2_attn_workspace_bytes'. */
int pygat_v2_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F, float negative_slope,
                               const float* x_dst, int64_t ldd, const void* x_src, int64_t lds, const float* a, const void* v,
                               int64_t ldv, float* out, int64_t ldo, void* ws, void* stream);
int pygat_v2_attn_edge_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                    int F, float negative_slope, const float* x_dst, int64_t ldd, const void* x_src, int64_t lds,
                                    const float* a, const void* v, int64_t ldv, const void* e, int64_t lde, float* out, int64_t ldo,
                                    void* ws, void* stream);

/* ------------------------------------------------ K22: seeded neighbour sampling of a block (csrc/k22_sample.hip), additive under ABI 16
 * The block the pattern ops above are fed with: n_dst destination nodes of the graph (n, nnz, rowptr, col: columns strictly increasing
 * inside a row) x their sampled sources, written as a CSR directly -- no sort, all arithmetic integer, two runs give the same bits.
 *   key(p) of the entry at CSR position p = word (p & 3) of Philox-4x32-10(counter (p >> 2, hop, 4, 0), key (seed lo, seed hi)); *seed
 *     is a uint64 in DEVICE memory.  The key depends on the position only: not on dst, not on fanout.
 *   row r = node dst[r] with positions [b, e): all of them if e - b <= fanout, else the fanout entries smallest in (key, p); kept
 *     positions are stored ascending.  (fanout = INT32_MAX keeps whole rows.)
 *   src_nodes = dst in the caller's order, then every other kept column once, ascending; an entry's local column is its index there.
 * Outputs, all sized by the CALLER's upper bounds (nothing is read back in between): blk_rowptr [n_dst + 1]; blk_col [cap] local
 * columns; edge_rc [cap x 2] (row, local column); edge_ids [cap] the graph's CSR position of every entry; src_nodes [src_cap];
 * info [4] = (entries E, sources n_src, 1 if some dst[r] lies outside [0, n), 1 if some id repeats in dst).  cap >= min(n_dst *
 * fanout, nnz) and src_cap >= n_dst + min(cap, n) hold every valid result; a row that would pass cap and a source that would pass
 * src_cap are not written.  An id outside [0, n) is never used as an index: its row is empty.  With a flag raised the other outputs
 * are not meaningful (after a repeat nothing is selected at all).
 * ws >= pygat_sample_workspace_bytes(n, n_dst) bytes, 16-byte aligned, contents irrelevant: two n-sized int32 tables (the marker of
 * the dst nodes, the marks of the kept columns), their scan, the per-row counts and the list of the long rows.
 * Rows whose positions span at most 64 Philox calls (253 entries at any alignment) are selected by one wave with the keys in
 * registers, longer ones by a work-group with a four-pass radix select (256-bin LDS histograms, keys recomputed per pass). */
int pygat_sample_workspace_bytes(int n, int n_dst, size_t* bytes);
int pygat_sample_block(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int n_dst, const int64_t* dst, int fanout,
                       const void* seed, uint32_t hop, int64_t cap, int64_t src_cap, int32_t* blk_rowptr, int32_t* blk_col,
                       int32_t* edge_rc, int64_t* edge_ids, int64_t* src_nodes, int32_t* info, void* ws, void* stream);
/* The same block sampled WEIGHTED BY EDGE, without replacement (Efraimidis-Spirakis / exponential clocks; the WEIGHTED instantiations
 * of the K22 kernels), additive under ABI 16: pygat_sample_block's arguments plus weight, nnz floats (4-byte aligned), one per entry at
 * its CSR position.  For the entry at position p with the Philox word k = key(p) above and w = weight[p]:
 *   w == 0: never sampled.  w > 0, finite or +inf: its clock is c(p) = E(k) / w with E(k) = -ln(1 - (k + 0.5) / 2^32) a unit exponential
 *     variate; a row keeps its fanout entries smallest in (c, p) among those with w > 0, and all of them if they number at most fanout.
 *     w = +inf gives c = 0: the entry is always kept (a self loop, say); of more than fanout such entries the first fanout by position.
 *   w < 0 or NaN in a row of dst: info[4] = 1 and the entry is never selected.  Rows that dst does not name are not looked at.
 *   The clock is fp32 throughout: E = -log1pf(-u), u = ((float)k + 0.5f) 2^-32 for k < 2^31, else E = -logf(v), v = ((float)(~k) + 0.5f)
 *     2^-32 (accurate logarithms; a few ulps from the exact value at every k); the key that is ordered is the bit pattern of E / w.  It
 *     depends on (seed, hop, p, w) only, so the sample at a smaller fanout is a subset of the one at a larger fanout.  tests/
 *     sampler_weighted_ref.py restates it in fp64.  No float is summed across lanes: two runs give the same bits.
 * Everything else -- kept positions ascending, src_nodes, the outputs and their bounds, ws (pygat_sample_workspace_bytes: the weighted
 * passes need no more) and the refusals, each after `weighted_block: ` -- is pygat_sample_block's; info has FIVE words: (entries,
 * sources, id outside, id repeated, bad weight).  The rows' counts are their numbers of positive weights: the long rows are listed
 * before the counts are scanned and counted by a work-group each, so no single thread walks a hub's weights. */
int pygat_weighted_block(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int n_dst, const int64_t* dst, int fanout,
                         const float* weight, const void* seed, uint32_t hop, int64_t cap, int64_t src_cap, int32_t* blk_rowptr,
                         int32_t* blk_col, int32_t* edge_rc, int64_t* edge_ids, int64_t* src_nodes, int32_t* info, void* ws,
                         void* stream);

/* ------------------------------------------------ K23: the induced subgraph of a node set and seeded random walks
 * (csrc/k23_subgraph.hip), additive under ABI 16.  The square sub-pattern of the graph (n, nnz, rowptr, col: columns strictly
 * increasing inside a row) on the SET of the n_in ids in `nodes` (int64, any order, repeats allowed; 1 <= n_in < 2^31), written as a
 * CSR directly -- no sort, all arithmetic integer, no atomics, two runs give the same bits:
 *   local ids are ranks in ascending global id: sub_nodes [n_sub] = the distinct ids ascending, index[i] = the local id of nodes[i]
 *     (sub_nodes[index[i]] == nodes[i]; -1 for an id outside [0, n)).  The relabelling is monotone, so
 *   row r holds, in ascending position, the positions p of graph row sub_nodes[r] whose col[p] is in the set, with local column
 *     rank(col[p]): strictly ascending.  edge_ids = those positions, strictly increasing over the whole sub-pattern.
 * Two calls with ONE host read between them, so that the entry tables are allocated at their exact size:
 *   pygat_subgraph_count writes sub_nodes and sub_rowptr (room for m and m + 1 words, m = min(n_in, n): valid up to n_sub and n_sub + 1),
 *     index [n_in] and info [4] = (rows n_sub, entries, 1 if some id lies outside [0, n), rows without an entry); nothing is read
 *     back inside it.  An id outside [0, n) is never used as an index: it is not part of the set.
 *   pygat_subgraph_fill takes n_sub = info[0] and sub_nnz = info[1] as read by the caller (both >= 1), the SAME n_in, sub_nodes,
 *     sub_rowptr and workspace with its contents intact (the marks, their ranks and the list of long rows), and writes sub_col
 *     [sub_nnz], edge_rc [sub_nnz x 2] (row, local column) and edge_ids [sub_nnz].  Every store is bounded by the row's range in
 *     sub_rowptr and by sub_nnz, whatever the workspace holds.
 * ws >= pygat_subgraph_workspace_bytes(n, n_in) bytes, 16-byte aligned: an n-sized int32 mark table, its scan, the per-row counts
 * and the list of the long rows.  Rows of at most 64 entries are counted and filled by one thread, rows of at most 256 by one wave
 * (64 positions per round), longer ones by a work-group each (1024 positions per round).  Each refusal names its entry point:
 * `subgraph_workspace_bytes: `, `subgraph_count: `, `subgraph_fill: `. */
int pygat_subgraph_workspace_bytes(int n, int64_t n_in, size_t* bytes);
int pygat_subgraph_count(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_in, const int64_t* nodes,
                         int64_t* sub_nodes, int64_t* index, int32_t* sub_rowptr, int32_t* info, void* ws, void* stream);
int pygat_subgraph_fill(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_in, int n_sub, int64_t sub_nnz,
                        const int64_t* sub_nodes, const int32_t* sub_rowptr, int32_t* sub_col, int32_t* edge_rc, int64_t* edge_ids,
                        void* ws, void* stream);
/* Seeded uniform random walks: walks [n_walk x (length + 1)] int64, walks[w, 0] = start[w] (int64, repeats allowed), and for t = 1 ..
 * length, with cur = walks[w, t - 1], [b, e) its row and d = e - b:
 *   k = word (t & 3) of Philox-4x32-10(counter (w, hop, 5, t >> 2), key (seed lo, seed hi)); *seed is a uint64 in DEVICE memory;
 *   walks[w, t] = col[b + ((k * d) >> 32)] (the high word of the 64-bit product); a walker on a row without entries stays.
 * The pick is uniform up to d / 2^32; the same (seed, hop) gives the same walks bit for bit.  info [1] = 1 if some start[w] lies
 * outside [0, n): it is never used as an index (that walker stays where it is).  One thread per walker, one Philox call per four
 * steps; refusals after `random_walk: `. */
int pygat_random_walk(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_walk, const int64_t* start, int length,
                      const void* seed, uint32_t hop, int64_t* walks, int32_t* info, void* stream);

/* ------------------------------------------------ K24: link-prediction mini-batches -- the CSR position of (row, col) pairs and seeded
 * negative destinations per source node (csrc/k24_linkpred.hip), additive under ABI 16.  The graph is (n, nnz, rowptr, col) with the
 * columns strictly increasing inside a row; all arithmetic is integer, there are no atomics and no workspace, and two runs give the
 * same bits.
 * pygat_find_edges: for each of the n_pairs pairs (row[i], colq[i]) (int64; 1 <= n_pairs < 2^31), pos[i] (int64) = the position p
 *   with rowptr[row[i]] <= p < rowptr[row[i] + 1] and col[p] == colq[i], or -1 if the pair is no entry: the positions that
 *   pygat_sample_block and pygat_subgraph_fill write as edge_ids.  One thread per pair, one binary search over the row.  info [1] = 1
 *   if an id of some pair lies outside [0, n) on either side: it is never used as an index, and that pair gets -1.
 * pygat_draw_negatives: neg [n_src x num_neg] int64 -- for every source node src[w] (int64, repeats allowed; 1 <= n_src, num_neg >= 1,
 *   n_src * num_neg < 2^31) num_neg ids that are NOT its neighbours.  For the flat draw i = w * num_neg + s, with u = src[w]:
 *     the forbidden list c_0 < ... < c_{f-1} is the columns of row u, with u merged in at its sorted place if exclude_self == 1 and u is
 *       not already a column; m = n - f ids are left;
 *     k = word (i & 3) of Philox-4x32-10(counter (i >> 2, hop, 6, 0), key (seed lo, seed hi)); *seed is a uint64 in DEVICE memory;
 *     r = (k * m) >> 32 (the high word of the 64-bit product); t* = #{t : c_t - t <= r}; neg[i] = r + t*, the r-th smallest id outside
 *       the list.  c_t - t does not decrease with t, so t* is one upper-bound binary search over the row: there is no rejection loop.
 *   Each draw is uniform over the m candidates up to m / 2^32; the draws of a row are independent, so ids may repeat; the same (seed,
 *   hop) gives the same draws bit for bit.  info [2]: info[0] = 1 if some src[w] lies outside [0, n) -- it is never used as an index,
 *   and its draws are -1; info[1] = 1 if some row has no candidate (m == 0) -- its draws are -1.  One thread per draw.
 * Each refusal names its entry point: `find_edges: `, `draw_negatives: `. */
int pygat_find_edges(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_pairs, const int64_t* row,
                     const int64_t* colq, int64_t* pos, int32_t* info, void* stream);
int pygat_draw_negatives(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_src, const int64_t* src, int num_neg,
                         int exclude_self, const void* seed, uint32_t hop, int64_t* neg, int32_t* info, void* stream);

/* ------------------------------------------------ K7: train-mode dropout around the projection
 * The reference drops out inside every head, each head with its own masks (models.py:32,34 call the heads
 * one after another): the input (layers.py:34,132), Wh (layers.py:37,136), the attention (layers.py:43,153).
 * Masks are pre-scaled keep masks (0 or 1/(1-p)).  Either the caller passes one explicitly (`mask`,
 * [H x n x Fin]; tests) or it is drawn in-kernel: Philox-4x32-10, key = *seed (a uint64 in DEVICE memory, so
 * a captured HIP graph replays with fresh masks when the caller refreshes it), `stream_id` separating the
 * different masks drawn from one seed.
 *   pygat_dropout_mask      out[e] = mask, e < count                          (Wh and attention masks)
 *   pygat_dropout_expand    A'[i, h*Fin + k] = x[i,k] * m_h[i,k]   -> A' [n x H*Fin] (ldo >= H*Fin)
 *   pygat_pack_blockdiag    B'[h*Fin + k, :] = [ W_h[k,:] in head h's padded columns | same for Wskip ]
 *                           so that A' B' = [Wh | Sk] for all heads in ONE GEMM (K = H*Fin)
 *   pygat_unpack_blockdiag  dW[h,k,f] = dB'[h*Fin + k, col_offset + h*Fp + f]  (diagonal blocks of A'^T dWh)
 *   pygat_dropout_head_sum  dx[i,k] (+)= sum_h m_h[i,k] dxe[i, h*Fin + k]      (dxe = dWh B'^T; same mask/seed/
 *                           stream_id as the expand call)
 */
int pygat_dropout_mask(int64_t count, float p, const void* seed, uint32_t stream_id, float* out, void* stream);
/* two of them (a level's Wh and attention masks) in one launch */
int pygat_dropout_mask2(float p, const void* seed, int64_t count1, uint32_t stream1, float* out1, int64_t count2,
                        uint32_t stream2, float* out2, void* stream);
int pygat_dropout_expand(int n, int Fin, int H, const float* x, int64_t ldx, const float* mask, float p,
                         const void* seed, uint32_t stream_id, float* out, int64_t ldo, void* stream);
int pygat_dropout_head_sum(int n, int Fin, int H, const float* dxe, int64_t lde, const float* mask, float p,
                           const void* seed, uint32_t stream_id, float* dx, int64_t ldx, int accumulate,
                           void* stream);
int pygat_pack_blockdiag(int H, int Fin, int Fo, const float* W, const float* w_skip, float* Bp, int64_t ldb,
                         void* stream);
int pygat_unpack_blockdiag(int H, int Fin, int Fo, const float* dBp, int64_t ldb, int col_offset, float* dW,
                           void* stream);

/* Per-head input dropout WITHOUT the wide operand (default since ABI 9 where supported: H <= 8 and
 * (skip ? 2 : 1) * Fp <= 256, pygat_headmask_supported).  The decisions of all heads for x[i,k] are one byte,
 *   pygat_dropout_bits        bits[i,k] bit h = head h keeps x[i,k]   (word h & 3 of Philox counter (k, i, stream_id, h >> 2))
 * and the projection and its weight gradient run for ALL heads in one launch with X read once -- the A tile is staged
 * in LDS with its mask bytes and the heads are an inner loop over the MFMA fragments (a_h = bit_h ? x : 0):
 *   pygat_project_dropout     [Wh | Sk] = 1/(1-p) (X .* m_h) [W_h | Wskip_h]           Wcat from pygat_pack_params;
 *                             split_k K slabs over Fin for graphs with few 128-row tiles
 *   pygat_wgrad_dropout       dWc [Fin x R (+R)] = 1/(1-p) (X .* m_h)^T [dWh_h | Gp_h]  (then pygat_unpack_wgrad);
 *                             split_k K slabs over the nodes: a slab is ONE fp32 accumulator chain per output, so give
 *                             slabs of a few hundred rows (pygat_amd/dropout.py: >= 64 rows until the chip is full) when
 *                             the result should match a blocked CPU product to its last bits
 *   pygat_dropout_head_sum_bits  dx[i,k] (+)= 1/(1-p) sum_h bit_h[i,k] dxe[i, h*Fin + k]
 * Memory: N*Fin bytes instead of N*H*Fin*4 (Citeseer: 12 MB instead of 394 MB); no products with zero blocks.
 * X must be dense (ldx == Fin).  Explicit masks (tests) are packed into the same bytes by the caller. */
int pygat_headmask_supported(int H, int Fo, int skip);
int pygat_dropout_bits(int n, int Fin, int H, float p, const void* seed, int stream_id, unsigned char* bits, void* stream);
size_t pygat_project_dropout_workspace_bytes(int n, int H, int Fo, int skip, int split_k);
int pygat_project_dropout(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const unsigned char* bits, float p,
                          const float* Wcat, int64_t ldw, float* Wh, float* Sk, int split_k, void* ws, void* stream);
size_t pygat_wgrad_dropout_workspace_bytes(int Fin, int H, int Fo, int skip, int split_k);
int pygat_wgrad_dropout(int n, int Fin, int H, int Fo, const float* X, int64_t ldx, const unsigned char* bits, float p,
                        const float* dWh, const float* Gp, int64_t ldgp, float* dWc, int split_k, void* ws, void* stream);
int pygat_dropout_head_sum_bits(int n, int Fin, int H, const float* dxe, int64_t lde, const unsigned char* bits, float p,
                                float* dx, int64_t ldx, int accumulate, void* stream);
/* NARROW levels (Fin <= 128, H <= 8, (skip ? 2 : 1) H F'p <= 128 -- the second level of the citation models: 64 inputs,
 * 1 x 7 or 8 x 3 outputs; pygat_dropout_narrow says whether a shape qualifies): pygat_project_dropout and
 * pygat_wgrad_dropout then run on the vector ALUs with the weight table in registers (csrc/k10_narrow.hip) -- split_k of
 * the projection is ignored, split_k of the weight gradient is the number of row slabs (one wave each; a few rows per slab
 * on a small graph, 8-32 on a large one) and its workspace is always used -- and the gradient into the level's input is one
 * launch instead of a GEMM per head and a fold:
 *   pygat_dx_dropout   dx[i,k] (+)= 1/(1-p) sum_h bit_h(i,k) ( dWh_h[i,:] . W_h[k,:] + Gp_h[i,:] . Wskip_h[k,:] )
 * dWh [n x R], Gp rows of stride ldgp or NULL, Wcat from pygat_pack_params.  PYGAT_NARROW=0 (read when the library loads)
 * switches the narrow kernels off. */
int pygat_dropout_narrow(int Fin, int H, int Fo, int skip);
int pygat_dx_dropout(int n, int Fin, int H, int Fo, const float* dWh, const float* Gp, int64_t ldgp, const unsigned char* bits,
                     float p, const float* Wcat, int64_t ldw, float* dx, int64_t lddx, int accumulate, void* stream);

/* ------------------------------------------------ the citation scripts' training loss (next row 8(f)-2: fused epoch)
 * train.py:151-152,159: loss = nll_loss(log_softmax(elu(out), dim=1)[idx], labels[idx]), forward and backward as ONE
 * launch each (ATen: 17).  The index set is given as per-row weights: weight[r] = (multiplicity of r in idx) / len(idx),
 * label[r] the class of row r (any value where weight[r] == 0).
 *   forward:  loss[0] = sum_r weight[r] * -log_softmax(elu(out[r, :]))[label[r]]     (deterministic two-stage sum inside
 *             the launch; ws >= pygat_nll_workspace_bytes(n), ZEROED once by the caller, left zeroed by every launch)
 *   backward: dout[r, c] = gscale[0] * d loss / d out[r, c]   (every row written; gscale = the upstream gradient, on the device) */
size_t pygat_nll_workspace_bytes(int n);
int pygat_elu_logsoftmax_nll(int n, int C, const float* out, int64_t ldo, const int32_t* label, const float* weight,
                             void* ws, float* loss, void* stream);
int pygat_elu_logsoftmax_nll_backward(int n, int C, const float* out, int64_t ldo, const int32_t* label, const float* weight,
                                      const float* gscale, float* dout, int64_t ldd, void* stream);

/* ------------------------------------------------ sparse input features (level 1 of the citation configurations)
 * The reference densifies its bag-of-words features (utils.py:38-41,60) and multiplies the zeros (Cora: 98.7 % of X).
 * With the non-zero pattern of X extracted once -- CSR (rowptr, col, val) for the projection, its transpose (colptr, row,
 * val, cut into segments) for the weight gradient -- these two replace pygat_project / pygat_project_dropout and pygat_wgrad /
 * pygat_wgrad_dropout for a first level (no gradient into X is formed):
 *   pygat_project_sparse   [Wh | Sk | s] = scale * (X .* m_h) Wcat      Wcat from pygat_pack_params; Sk, s may be NULL
 *   pygat_wgrad_sparse     dW_h = scale * (X .* m_h)^T dWh_h, dWskip_h = ... Gp_h   written as [H x Fin x F'] directly
 * p = 0: no dropout (m = 1, scale = 1).  p > 0: per-head input dropout with the decisions of pygat_dropout_bits -- drawn
 * from (seed, stream_id) per non-zero, or read from explicit `bits` [n x Fin] (H <= 8) -- and scale = 1 / (1 - p); s must
 * be NULL then (scores come from the masked Wh, pygat_attn_scores).  p outside [0, 1] (NaN included) is refused.  At most
 * 512 output columns (2 R + H). */
int pygat_project_sparse(int n, int Fin, int H, int Fo, const int32_t* rowptr, const int32_t* col, const float* val,
                         const float* Wcat, int64_t ldw, float p, const void* seed, int stream_id, const unsigned char* bits,
                         float* Wh, float* Sk, float* s, void* stream);
/* The transpose is cut into nseg SEGMENTS of at most 128 entries, none crossing a feature column (a frequent word's column is
 * thousands of entries long): segment s covers entries [seg_begin[s], seg_end[s]) of (row, val) -- which are in column
 * order -- and belongs to column seg_col[s]; column k owns the segments [colseg[k], colseg[k+1]) (at least one each, so
 * nseg >= Fin).  One wave per segment, then one per column adds its segments in order.  ws >=
 * pygat_wgrad_sparse_workspace_bytes(nseg, H, F', skip). */
size_t pygat_wgrad_sparse_workspace_bytes(int nseg, int H, int Fo, int skip);
int pygat_wgrad_sparse(int n, int Fin, int H, int Fo, int nseg, const int32_t* colseg, const int32_t* seg_col,
                       const int32_t* seg_begin, const int32_t* seg_end, const int32_t* row, const float* val, float p,
                       const void* seed, int stream_id, const unsigned char* bits, const float* dWh, const float* Gp, int64_t ldg,
                       void* ws, float* dW, float* dWskip, void* stream);

/* train_ppi.py:114,157: nn.BCEWithLogitsLoss(reduction='mean') over `total` logits / targets (fp32, contiguous), one launch
 * each way: loss[0] = mean( max(x,0) - x y + log1p(exp(-|x|)) );  dlogits = gscale[0] / total * (sigmoid(x) - y).
 * ws >= pygat_bce_workspace_bytes(total), zero before the first call (the kernel leaves its counter at zero). */
size_t pygat_bce_workspace_bytes(int64_t total);
int pygat_bce_with_logits(int64_t total, const float* logits, const float* targets, void* ws, float* loss, void* stream);
int pygat_bce_with_logits_backward(int64_t total, const float* logits, const float* targets, const float* gscale, float* dlogits,
                                   void* stream);

/* ---------------------------------------------- K11: optimiser step (csrc/k11_adam.hip)
 * torch.optim.Adam's update (train.py:64-66,122: lr 0.005, weight_decay 5e-4; train_ppi.py:58-60) for up to
 * PYGAT_ADAM_MAX_TENSORS parameter tensors in ONE launch:
 *   g += wd p;  m += (g - m)(1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 * (hyper-parameters as doubles, like the Python floats torch holds: 1 - beta and the bias corrections are formed in double).
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of ntensors device pointers (fp32, contiguous), numel their sizes.
 * state: PYGAT_ADAM_STATE_BYTES of DEVICE memory, 8-byte aligned ({int32 t, uint32 scratch, double beta1^t, double beta2^t}),
 * zero before the first step; the kernel advances t itself, so a
 * captured HIP graph replays successive steps.  More tensors: several calls must not share one state (each would advance
 * it) -- give every group of 48 its own. */
#define PYGAT_ADAM_MAX_TENSORS 48
#define PYGAT_ADAM_STATE_BYTES 24
int pygat_adam_step(int ntensors, float* const* params, const float* const* grads, float* const* exp_avg,
                    float* const* exp_avg_sq, const int64_t* numel, double lr, double beta1, double beta2, double eps,
                    double weight_decay, void* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYGAT_AMD_H */
