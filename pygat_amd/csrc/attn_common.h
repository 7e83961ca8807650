// Lane mapping and nnz-split skeleton shared by the fused attention kernels K2 (forward), K3 (row
// backward), K4 (column backward), K6 (GATv2 backward) and K16 (bf16 forward): how a slot is opened (SlotView), which
// record a piece of a cut row lies in (piece_record), the screening loop of the fix-up kernels that have no cut-row list
// (screen_cut_rows) and the launch geometry of a pass (main_grid, fixup_grid).
//
// A node row is R = H*Fp floats (all local heads interleaved, each padded to
// Fp = power of two), i.e. NCH = R/4 float4 "chunks".  The CSR edge list is cut
// into SLOTS of `ts` consecutive edges; a lane group of LPR lanes owns one slot
// and walks its edges (nnz split: perfect balance whatever the degree skew):
//   LPR  lanes per gathered row  = pow2 >= NCH, capped at 64
//   EPW  = 64 / LPR slots per wave (independent lane groups, no shuffles between them)
//   VEC  chunks per lane (only when NCH > 64, LPR = 64): chunk c = c0 + 64*v
// Lane l: slot-in-wave = l / LPR, c0 = l % LPR.  A float4 never straddles heads
// (Fp % 4 == 0); the head of chunk c is (4c) / Fp and the LPH = Fp/4 lanes of a
// head are consecutive and aligned, so per-head reductions are DPP butterflies.
#pragma once
#include "common.h"

namespace pygat {

constexpr int FIX_LIST_WAVES = 16;  // waves per work-group of the list-driven fix-up kernels
// Cut rows one wave of a list-driven fix-up merges side by side (the entries behind the wide ones): a wave of 64 / LPR lane
// groups per row piece had most of them idle -- the config-5 graph has 21.7 k cut rows of 5 pieces on average at 64-edge slots,
// 57.9 k of 4.8 at 32 -- and the launch is latency per wave, not bytes.  The list is sorted by piece count, so the rows of a
// wave are alike.
__host__ __device__ constexpr int fix_rows_per_wave(int lpr) { return 64 / lpr >= 8 ? 4 : (64 / lpr >= 2 ? 2 : 1); }
constexpr int FIX_WIDE = 32;   // cut rows with more pieces are merged by a whole work-group
constexpr int FIX_SCREEN = 8;  // slots screened per wave by the fix-up kernels (owned rows are merged serially)
constexpr float NEG_BIG = -1.0e30f;  // running-max seed: exp(NEG_BIG - x) == 0, exp(NEG_BIG - NEG_BIG) == 1

struct RowShape {
  int H, Fo, Fp, R, NCH;  // heads of THIS kernel pass, true width, padded width, H*Fp, R/4
  int fp_shift;           // log2(Fp)
  int lph;                // lanes per head = Fp/4 (power of two, may exceed 64 only if Fp > 256: rejected)
  // A pass may cover a WINDOW of the level's heads (see head_group): the per-node tables keep the
  // level's full width, so rows are addressed with the level's strides and pointers pre-offset to the window.
  int Htot;               // heads of the level (mean mode divides by it)
  int64_t ldr;            // row stride of the R-wide tables (Wh, Sk, hattn, dWh) = Htot*Fp
  int64_t ldh;            // row stride of the per-head tables (s, m, Z, ds, dt, attention mask) = Htot
  int64_t ldo;            // row stride of out / G = Htot*Fo
};

static inline bool make_row_shape(int H, int Fo, RowShape* rs) {
  int Fp = padded_width(Fo);
  if (H <= 0 || Fp == 0) return false;
  rs->H = H; rs->Fo = Fo; rs->Fp = Fp; rs->R = H * Fp; rs->NCH = rs->R / 4;
  rs->fp_shift = ilog2(Fp); rs->lph = Fp / 4;
  rs->Htot = H; rs->ldr = rs->R; rs->ldh = H; rs->ldo = (int64_t)H * Fo;
  return rs->NCH <= 256;  // VEC <= 4
}

// Heads per kernel pass ("head window").
// A pass takes rows of at most 1024 floats (VEC <= 4 chunks of 16 B per lane); wider levels are walked
// window by window.  That is the only reason to window the forward: measured on MI355X (RMAT 1M/10.8M,
// 8 heads x 128) K2 is fastest on the full 4-KB rows (9.1 ms; 9.7 ms as 4 windows of 1 KB, whose
// gathers hit only a quarter of each row and load the HBM channels unevenly).
static inline int head_group_fwd(int H, int Fp) {
  if (H * Fp <= 1024) return H;
  const int g = 1024 / Fp;
  return g < 1 ? 1 : g;
}
// K2 on a cache-resident table (PPI: 3144 x 1024 floats): at VEC = 4 it holds 205 VGPRs = 2 waves per SIMD; two windows of
// 512 floats run 4 and finish sooner despite the second launch (PPI epoch 2.43 -> 2.40 ms).  Large tables keep whole rows
// (the gathered row is the HBM transaction; a window re-reads the edge structure: measured).
static inline int head_group_fwd_n(int64_t n, int H, int Fp) {
  constexpr int fwd_w = 512;   // floats per window on a cache-resident table
  const int64_t R = (int64_t)H * Fp;
  if (R > fwd_w && R <= 1024 && n * R * 4 < ((int64_t)256 << 20)) { const int g = fwd_w / Fp; return g < 1 ? 1 : g; }
  return head_group_fwd(H, Fp);
}
// The two backward passes hold two gathered/row-local rows per edge: at VEC >= 3 they need 170-250
// VGPRs, run 2 waves per SIMD and stop covering the HBM latency (same workload: K3b 11.0 -> 8.5 ms,
// K4 11.6 -> 9.9 ms as windows of 256 floats = one chunk per lane).  Windows cost extra launches, so
// they are used where the gathered table is far beyond the caches and rows are wider than 256 floats (8 heads x 64 on the
// config-5 graph: K4 5.14 -> 4.72 ms as two windows of 256, the step 13.6 -> 13.0); a cache-resident table wider than 512
// floats takes windows of 512 (VEC = 2, 150 VGPRs) instead of whole rows -- K4 at VEC = 4 holds 256 VGPRs + 16 AGPRs, ONE
// wave per SIMD (PPI epoch 2.55 -> 2.43 ms; windows of 256 there: 2.66).
// This is the DEFAULT (pygat_head_group): the backward entry points take the heads per window as an argument (0 = this
// default), because it is also the layout of a GR row, which the caller allocates and reads -- no environment variable
// decides it (rounds 1-3 read PYGAT_BWD_WINDOW_BYTES and three more on every call).
static inline int head_group_bwd(int64_t n, int H, int Fp) {
  const int64_t R = (int64_t)H * Fp;
  constexpr int64_t min_bytes = (int64_t)256 << 20;   // gathered table beyond the Infinity Cache
  if (R <= 256) return head_group_fwd(H, Fp);
  if (n * R * 4 < min_bytes) {   // cache-resident table: windows of 512 floats
    if (512 >= R) return head_group_fwd(H, Fp);
    const int g = 512 / Fp;
    return g < 1 ? 1 : g;
  }
  const int g = 256 / Fp;
  return g < 1 ? 1 : g;
}
// heads per window of a backward call: the caller's choice when it gave one (any window a kernel pass can take), else the default
static inline int head_group_arg(int head_group, int64_t n, int H, int Fp) {
  if (head_group <= 0) return head_group_bwd(n, H, Fp);
  const int cap = head_group_fwd(H, Fp);
  if (head_group > cap) return -1;                // rows of more than 1024 floats per pass
  return head_group < H ? head_group : H;
}
// narrow rows (a wave carries 8-64 slots, the whole grid is a few ten waves per SIMD): one-wave work-groups, so that a SIMD
// slot is refilled as soon as ITS wave ends instead of when the slowest of four does (measured against 128 / 256: DESIGN.md)
static inline unsigned narrow_block() { return 64u; }

// shape of the window [h0, h0+hc) of a level with Htot heads
static inline bool make_window_shape(int Htot, int Fo, int hc, RowShape* rs) {
  if (!make_row_shape(hc, Fo, rs)) return false;
  rs->Htot = Htot; rs->ldr = (int64_t)Htot * rs->Fp; rs->ldh = Htot; rs->ldo = (int64_t)Htot * Fo;
  return true;
}
// A backward call may cover only the heads [hb, hb+hr) of a level with H heads (h_count == 0: all of them):
// the level's tables (Wh, G, out, s, m, Z, ds, dt, dWh, dz_t, masks) keep their full width and are addressed with
// the level's strides, while GR -- written and read only by the backward -- is compact for the range.
struct HeadRange { int hb, hr; };
static inline bool make_head_range(int H, int h_first, int h_count, HeadRange* r) {
  if (h_count == 0 && h_first == 0) { r->hb = 0; r->hr = H; return H > 0; }
  if (h_first < 0 || h_count <= 0 || h_first + h_count > H) return false;
  r->hb = h_first; r->hr = h_count;
  return true;
}
// column offset of a window inside a GR row [Gp(window) | rowtab(window)] ... : h0 * (Fp + 4)
static inline int64_t gr_window_offset(int h0, int Fp) { return (int64_t)h0 * (Fp + 4); }

// (LPR, VEC) for a row shape
static inline void pick_lanes(const RowShape& rs, int* lpr, int* vec) {
  if (rs.NCH <= 64) {
    int l = 1;
    while (l < rs.NCH) l <<= 1;
    *lpr = l; *vec = 1;
  } else {
    *lpr = 64; *vec = (rs.NCH + 63) / 64;
  }
}

#define PYGAT_DISPATCH_LANES(LPRV, VECV, CALL)                      \
  do {                                                              \
    if ((VECV) == 1) {                                              \
      switch (LPRV) {                                               \
        case 1: { constexpr int LPR = 1, VEC = 1; CALL; } break;    \
        case 2: { constexpr int LPR = 2, VEC = 1; CALL; } break;    \
        case 4: { constexpr int LPR = 4, VEC = 1; CALL; } break;    \
        case 8: { constexpr int LPR = 8, VEC = 1; CALL; } break;    \
        case 16: { constexpr int LPR = 16, VEC = 1; CALL; } break;  \
        case 32: { constexpr int LPR = 32, VEC = 1; CALL; } break;  \
        default: { constexpr int LPR = 64, VEC = 1; CALL; } break;  \
      }                                                             \
    } else if ((VECV) == 2) { constexpr int LPR = 64, VEC = 2; CALL; \
    } else if ((VECV) == 3) { constexpr int LPR = 64, VEC = 3; CALL; \
    } else { constexpr int LPR = 64, VEC = 4; CALL; }               \
  } while (0)

struct GraphDev {  // device view of pygat_graph
  int n;
  int64_t nnz;
  const int32_t* rowptr;
  const int2* rc;   // (row, col) per edge
  int ts;           // nominal edges per slot
  const int32_t* sb;  // row-snapped slot borders [nslots+1] or nullptr (uniform slots)
  const int4* meta;   // [nslots] (e0, e1, first row, flags) or nullptr (pygat_graph.slot_meta)
  const int32_t* cut;  // [n_cut][3] (slot, row, pieces) or nullptr
  int n_cut, n_cut_wide;
  int64_t k0, kn;   // active slot range [k0, k0 + kn) (the forward can work on a range of whole rows)
  const int32_t* order;   // slot handed to grid position q (pygat_graph.slot_order) or nullptr: q itself
  const int32_t* urow;    // caller's row of internal node i (pygat_graph.user_row) or nullptr: i itself
};

// allow_slot_range: 0 none, 1 any range of whole rows (pygat_gat_forward), 2 a PREFIX [0, slot_count) (the column pass and the fold of
// its da records: the slots behind it are the self-loop-only tail of a degree-ordered pattern, pygat_gat_backward_col_tail)
static inline int check_graph(const pygat_graph* g, GraphDev* d, int allow_slot_range = 0) {
  if (!g || !g->rowptr || !g->edge_rc || g->n <= 0 || g->nnz <= 0) {
    set_error("graph: null or empty (n=%d nnz=%lld)", g ? g->n : -1, g ? (long long)g->nnz : -1LL);
    return PYGAT_EINVAL;
  }
  if (g->nnz >= (int64_t)1 << 31) {
    set_error("graph: nnz %lld exceeds int32 edge indexing", (long long)g->nnz);
    return PYGAT_EINVAL;
  }
  if (g->slot_edges < 4 || (g->slot_edges & 3)) {
    set_error("graph: slot_edges=%d must be a multiple of 4, >= 4", g->slot_edges);
    return PYGAT_EINVAL;
  }
  d->n = g->n; d->nnz = g->nnz; d->rowptr = g->rowptr; d->rc = reinterpret_cast<const int2*>(g->edge_rc);
  d->ts = g->slot_edges; d->sb = g->slot_begin; d->meta = reinterpret_cast<const int4*>(g->slot_meta);
  if (g->slot_meta && !aligned16(g->slot_meta)) {
    set_error("graph: slot_meta must be 16-byte aligned");
    return PYGAT_EINVAL;
  }
  d->cut = g->cut_rows; d->n_cut = g->cut_rows ? g->n_cut : 0; d->n_cut_wide = g->cut_rows ? g->n_cut_wide : 0;
  if (d->n_cut < 0 || d->n_cut_wide < 0 || d->n_cut_wide > d->n_cut) {
    set_error("graph: bad cut-row list (n_cut=%d n_cut_wide=%d)", g->n_cut, g->n_cut_wide);
    return PYGAT_EINVAL;
  }
  const int64_t total = (g->nnz + g->slot_edges - 1) / g->slot_edges;
  d->k0 = 0; d->kn = total;
  d->order = g->slot_order;
  d->urow = g->user_row;
  if (g->slot_order && g->slot_count != 0) {
    set_error("graph: slot_order needs the whole slot range (slot_count = 0)");
    return PYGAT_EINVAL;
  }
  if (g->slot_count != 0) {
    if (!allow_slot_range || g->slot_first < 0 || g->slot_count < 0 || g->slot_first + g->slot_count > total ||
        (allow_slot_range == 2 && g->slot_first != 0)) {
      set_error("graph: slot range [%lld, +%lld) of %lld %s", (long long)g->slot_first, (long long)g->slot_count,
                (long long)total, allow_slot_range ? "is out of bounds (or not a prefix, for the column pass)"
                                                   : "is not supported by this entry point");
      return PYGAT_EINVAL;
    }
    d->k0 = g->slot_first; d->kn = g->slot_count;
  }
  return PYGAT_OK;
}

#ifdef __HIPCC__
__host__ __device__
#endif
static inline int64_t num_slots(const GraphDev& g) { return (g.nnz + g.ts - 1) / g.ts; }
#ifdef __HIPCC__
// ELU: expm1 by a short series near 0 (where exp(x)-1 cancels), fast exp elsewhere (K2's epilogue and the self-loop-only tail)
__device__ __forceinline__ float elu1(float x) {
  if (x > 0.f) return x;
  if (x > -0.03125f) return x * (1.f + x * (0.5f + x * (0.16666667f + x * 0.041666668f)));
  return __expf(x) - 1.f;
}
// slot handed to grid position q of a main launch (q < num_slots): pygat_graph.slot_order, or q itself
__device__ __forceinline__ int64_t slot_at(const GraphDev& g, int64_t q) { return g.order ? (int64_t)g.order[q] : q; }
#endif

// Launch geometry of a pass over `nslots` slots.  Main launch: a wave carries 64 / lpr slots; narrow rows take one-wave
// work-groups (narrow_block), the others four waves.
struct MainGrid { unsigned bt, blocks; };
static inline MainGrid main_grid(int64_t nslots, int lpr, int vec) {
  MainGrid m;
  m.bt = (vec == 1 && lpr <= 8) ? narrow_block() : 256u;
  m.blocks = (unsigned)cdiv(cdiv(nslots, 64 / lpr), m.bt / 64);
  return m;
}
// Fix-up launch: driven by the graph's cut-row list (`listed`) -- one work-group of FIX_LIST_WAVES waves per wide entry, then
// fix_rows_per_wave(lpr) entries per wave -- or, without a list, one work-group of four waves per FIX_SCREEN slots.
// wave_rows (K16): four-wave work-groups whose waves work alone, on one list entry or on FIX_SCREEN slots each.
// blocks == 0: the list is empty, there is nothing to launch.
struct FixGrid { bool listed; unsigned blocks; int waves; };
static inline FixGrid fixup_grid(const GraphDev& g, int lpr, bool wave_rows = false) {
  FixGrid f;
  f.listed = g.cut != nullptr;
  f.waves = (f.listed && !wave_rows) ? FIX_LIST_WAVES : 4;
  if (wave_rows) f.blocks = (unsigned)cdiv(f.listed ? (int64_t)g.n_cut : cdiv(g.kn, FIX_SCREEN), 4);
  else if (!f.listed) f.blocks = (unsigned)cdiv(g.kn, FIX_SCREEN);
  else f.blocks = g.n_cut > 0 ? (unsigned)(g.n_cut_wide + cdiv(g.n_cut - g.n_cut_wide, FIX_LIST_WAVES * fix_rows_per_wave(lpr))) : 0u;
  return f;
}

// Work-groups of the column pass (pygat_gat_backward_col) over gT for a level of H heads = its da_part records, or 0 when the
// pass does not take the attention-vector gradient along: no cut-row list (the rows its fix-up finishes are folded in by
// pygat_a_grad_fold from that list), head windows (hg < H), or a row shape other than 8 heads x 16 -- the one
// instantiation that keeps its four waves per SIMD with the sums (128 VGPRs).  The others hold 130-138 VGPRs with them,
// three waves, and lose more than the a-gradient pass costs: measured at 1 / 2 / 4 heads of 16 on the config-5 graph, K4
// 0.275 -> 0.291, 0.413 -> 0.444, 0.71 -> 0.83 ms (profiles/r4m_as_rank_of.jsonl of the first build), so they are not built.
static inline int64_t col_da_blocks(const GraphDev& g, int H, int Fp, int hg, int* lpr_out) {
  RowShape rs;
  if (!g.cut || !make_window_shape(H, Fp, H, &rs)) return 0;   // (Fp as F': padded_width(Fp) == Fp)
  if (hg < H) return 0;
  int lpr, vec;
  pick_lanes(rs, &lpr, &vec);
  if (vec != 1 || H != 8 || Fp != 16) return 0;
  if (lpr_out) *lpr_out = lpr;
  return main_grid(g.kn, lpr, vec).blocks;   // (kn: the active slots -- all of them, or the prefix of the call)
}

#ifdef __HIPCC__
// edge range of slot k
__device__ __forceinline__ void slot_range(const GraphDev& g, int64_t k, int64_t* e0, int64_t* e1) {
  if (g.sb) {
    *e0 = g.sb[k];
    *e1 = g.sb[k + 1];
  } else {
    *e0 = k * g.ts;
    *e1 = (*e0 + g.ts < g.nnz) ? *e0 + g.ts : g.nnz;
  }
}
// slot that contains edge position pos
__device__ __forceinline__ int64_t slot_of(const GraphDev& g, int64_t pos) {
  int64_t k = pos / g.ts;
  if (g.sb && pos < g.sb[k]) --k;
  return k;
}

// A slot as its lane group sees it when it starts to walk: the edge range, the first row, whether that row began in an earlier
// slot (its state then goes to the head record 2k) and what is known up front of the last row.
struct SlotView {
  int64_t e0, e1;
  int r_first;
  bool head_partial;
  bool tail_known, tail_flag;   // slot_meta says whether the last row continues; without it rowptr does (slot_tail_partial)
};
// by the chain slot_begin -> edge_rc -> rowptr
__device__ __forceinline__ SlotView open_slot_chain(const GraphDev& g, int64_t k) {
  SlotView s;
  slot_range(g, k, &s.e0, &s.e1);
  s.r_first = g.rc[s.e0].x;
  s.head_partial = g.rowptr[s.r_first] < s.e0;
  s.tail_known = false; s.tail_flag = false;
  return s;
}
// from the slot's slot_meta record where the graph has them (wave-uniform branch), else by the chain
__device__ __forceinline__ SlotView open_slot(const GraphDev& g, int64_t k) {
  SlotView s;
  if (g.meta) {
    const int4 mt = g.meta[k];
    s.e0 = mt.x; s.e1 = mt.y; s.r_first = mt.z;
    s.head_partial = (mt.w & 1) != 0; s.tail_known = true; s.tail_flag = (mt.w & 2) != 0;
  } else {
    s = open_slot_chain(g, k);
  }
  return s;
}
// did `cur` begin in an earlier slot (only the slot's first row can: its state then goes to the head record 2k)
__device__ __forceinline__ bool slot_head_partial(const SlotView& s, int cur) { return cur == s.r_first && s.head_partial; }
// does `cur`, the last row of the slot, continue in the next slot (its state then goes to the tail record 2k + 1)
__device__ __forceinline__ bool slot_tail_partial(const GraphDev& g, const SlotView& s, int cur) {
  return s.tail_known ? s.tail_flag : g.rowptr[cur + 1] > s.e1;
}

// record of piece q of the cut row that slot k owns: tail(k), head(k + 1), head(k + 2), ...
__device__ __forceinline__ int64_t piece_record(int64_t k, int q) { return q == 0 ? 2 * k + 1 : 2 * (k + q); }

// Slot k OWNS a cut row if its last row starts inside k and continues beyond: that row and the end of its edges.
__device__ __forceinline__ bool slot_owns_cut_row(const GraphDev& g, int64_t k, int* r, int* row_end) {
  int64_t e0, e1;
  slot_range(g, k, &e0, &e1);
  *r = g.rc[e1 - 1].x;
  *row_end = g.rowptr[*r + 1];
  return (int64_t)*row_end > e1 && (int64_t)g.rowptr[*r] >= e0;
}
// Screening loop of the fix-up kernels that have no cut-row list: the calling wave screens the FIX_SCREEN slots from `kbase`
// (below `kend`), one per lane, and calls merge(k, row, npieces) for every cut row they own, in slot order.  The waves of a
// work-group that screen the same slots see the same rows in the same order, so `merge` may hold barriers.
template <typename Merge>
__device__ __forceinline__ void screen_cut_rows(const GraphDev& g, int64_t kbase, int64_t kend, Merge&& merge) {
  const int lane = threadIdx.x & 63;
  int my_r = 0, my_end = 0;
  bool owner = false;
  if (lane < FIX_SCREEN && kbase + lane < kend) owner = slot_owns_cut_row(g, kbase + lane, &my_r, &my_end);
  unsigned long long todo = __ballot(owner);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int64_t k = kbase + src;
    const int r = __shfl(my_r, src);
    const int64_t row_end = __shfl(my_end, src);
    merge(k, r, (int)(slot_of(g, row_end - 1) - k) + 1);
  }
}

template <int VEC>
struct LaneCols {
  int cofs[VEC];   // float offset of the lane's chunk inside a padded row (clamped when invalid)
  int head[VEC];
  bool valid[VEC];
};

template <int LPR, int VEC>
__device__ __forceinline__ LaneCols<VEC> lane_cols(const RowShape& rs) {
  LaneCols<VEC> lc;
  const int c0 = (threadIdx.x & 63) & (LPR - 1);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    int c = c0 + 64 * v;
    lc.valid[v] = c < rs.NCH;
    int cc = lc.valid[v] ? c : 0;
    lc.cofs[v] = 4 * cc;
    lc.head[v] = (4 * cc) >> rs.fp_shift;
  }
  return lc;
}

// sum / online-softmax merge across the EPW edge slots of a wave (lanes l and l^off, off >= LPR)
// "does any lane of my LPR-lane group say yes": a ballot, usable in divergent code as long as whole groups diverge
template <int LPR>
__device__ __forceinline__ bool row_any(bool p) {
  const unsigned long long b = __ballot(p);
  if constexpr (LPR >= 64) {
    return b != 0ull;
  } else if constexpr (LPR == 32) {   // one select between the two halves of the (scalar) ballot
    return (((threadIdx.x & 32) ? (uint32_t)(b >> 32) : (uint32_t)b)) != 0u;
  } else {
    const int sh = (threadIdx.x & 63) & ~(LPR - 1);
    return ((b >> sh) & ((1ull << LPR) - 1ull)) != 0ull;
  }
}

template <int LPR, int SPAN = 64>   // sum over the lane groups of every aligned SPAN-lane block
__device__ __forceinline__ float slot_sum(float x) {
#pragma unroll
  for (int off = LPR; off < SPAN; off <<= 1) x += __shfl_xor(x, off);
  return x;
}
template <int LPR, int SPAN = 64>
__device__ __forceinline__ float4 slot_sum4(float4 v) {
#pragma unroll
  for (int off = LPR; off < SPAN; off <<= 1) {
    v.x += __shfl_xor(v.x, off); v.y += __shfl_xor(v.y, off);
    v.z += __shfl_xor(v.z, off); v.w += __shfl_xor(v.w, off);
  }
  return v;
}
#endif

}  // namespace pygat
