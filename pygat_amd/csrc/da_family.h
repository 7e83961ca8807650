// The kernel skeleton and the launcher tail of the fused attention families over an edge pattern: K19 (k19_dot_attention.hip), K20
// (k20_additive_attention.hip) and K21 (k21_gatv2_attention.hip), on the lane mapping of da_lanes.h.  A pass is two kernels, a piece
// kernel for the long rows (one wave per chunk, the rule of long_rows.h) and a row kernel; their bodies are here once, templated on
// the family, a type (DaFam<variant>, AaFam<LOGIT, DROP, BF16>, V2Fam<SHARED, DROP, EDGE, BF16>) that says what a lane group holds of its row and how it
// walks it:
//   forward   Fam::Own<VEC>; Fam::load<VEC>(g, ln, row, own); Fam::KEEP_MZ
//   backward  Fam::Row<VEC>, a DaGrad<VEC> and the row's own operand; Fam::bwd_load<LPR, VEC>(g, ln, row, r);
//             Fam::lone(start, end) (the row is one entry and the family cares: K19 under EDGE)
//   both      Fam::walk<LPR, VEC, PASS>(g, ln, e0, e1, step, lone, key, own | r, st | dx): the entries e0, e0 + step, ... < e1 folded
//             in that order, PASS 0 forward, 1 backward;  Fam::key(g): what a kernel reads once for all its rows (K19: the key of
//             the draws under DROP, zeros without; K20 and K21: the same key under DROP (da_key, da_lanes.h), a DaNoKey without)
// The backward pair is that of the families whose row gradient is a row of H*F floats (K19's dq, K21's dx_dst); K20's, one scalar
// per head and a record of H floats, is its own and shares da_grad_load alone: a trait for the accumulator would have been as long
// as the two kernels it saves.
// Device code.  The kernels are templates, and not helpers called from per-family kernels, on purpose: of the 462 kernels of the three
// families 456 are instruction for instruction what they were when each family had its own copy, 6 the same instructions in another
// order (profiles/da_family_isa.txt); helpers did not keep that.  What a kernel calls is the family's walk itself where that could be
// had (K19, K21): with one forwarding function between the kernel and the walk, the backward kernels of both came out reordered.
// Host side: the shape check, the check of a DROP launcher's p and seed, the parser of the kernel names pygat_kernel_footprint takes,
// the grids and the launch of a pair.
#pragma once
#include "da_lanes.h"
#include <string.h>

namespace pygat {

struct DaNoKey {};

// ------------------------------------------------------------------------------------------------------------------------ forward
// launch 1: one wave per chunk; the piece of every long row inside the chunk -> one partial record (acc, m, Z)
template <typename Fam, int LPR, int VEC>
__global__ __launch_bounds__(64) void da_fwd_long_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const auto key = Fam::key(g);
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  const int HF = g.H * g.F;
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int row, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    typename Fam::template Own<VEC> r;
    Fam::template load<VEC>(g, ln, row, r);
    DaState<VEC> st;
    da_init<VEC>(st);
    Fam::template walk<LPR, VEC, 0>(g, ln, e0 + grp, e1, EPW, false, key, r, st);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {                            // lane groups of the wave: the maximum first, one rescale, a fixed butterfly
      float mx = st.m[v];
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      const float f = __expf(st.m[v] - mx);                    // (a lane group without entries: 0 x 0)
      st.z[v] *= f;
      da_scale(st.acc[v], f);
      st.m[v] = mx;
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1) {
        st.z[v] += __shfl_xor(st.z[v], off);
        da_add(st.acc[v], da_shfl_xor(st.acc[v], off));
      }
    }
    if (grp == 0) {
      float* p = g.part + long_record(blockIdx.x, slot) * g.pstride;
      da_store_row<VEC>(p, ln, st.acc);
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (ln.lead >> v & 1) { p[HF + ln.head[v]] = st.m[v]; p[HF + g.H + ln.head[v]] = st.z[v]; }
    }
  });
}

// launch 2: one lane group per row.  m and Z are what a backward reads: a family without one (KEEP_MZ false) does not write them
template <typename Fam, int LPR, int VEC>
__global__ __launch_bounds__(256) void da_fwd_row_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (row >= g.n) return;                                      // (whole lane groups; nothing below crosses a group)
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
  const int HF = g.H * g.F;
  DaState<VEC> st;
  da_init<VEC>(st);
  if (end - start > LONG_ROW) {
    for_long_records(start, end, [&](int64_t rec) {
      const float* p = g.part + rec * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        da_merge(st.m[v], st.z[v], st.acc[v], p[HF + ln.head[v]], p[HF + g.H + ln.head[v]], ld4(p + ln.ofs[v]));
    });
  } else if (end > start) {
    typename Fam::template Own<VEC> r;
    Fam::template load<VEC>(g, ln, row, r);
    Fam::template walk<LPR, VEC, 0>(g, ln, start, end, 1, false, Fam::key(g), r, st);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (!(ln.ok >> v & 1)) continue;
    const bool any = end > start;
    const float z = st.z[v];
    const float4 a = st.acc[v];
    st4(g.out + row * g.ldo + ln.ofs[v], any ? make_float4(a.x / z, a.y / z, a.z / z, a.w / z) : da_zero4());
    if constexpr (Fam::KEEP_MZ)
      if (ln.lead >> v & 1) {
        g.m[row * g.H + ln.head[v]] = any ? st.m[v] : 0.f;
        g.Z[row * g.H + ln.head[v]] = z;
      }
  }
}

// ------------------------------------------------------------------------------------------------------------- backward, row side
// what every backward holds of its row besides the row's own operand: G, m, 1 / Z and D = <G, out> per head
template <int VEC>
struct DaGrad {
  float4 G[VEC];
  float m[VEC], rz[VEC], D[VEC];
};
template <int LPR, int VEC>
__device__ __forceinline__ void da_grad_load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, DaGrad<VEC>& r) {
  float4 o[VEC];
  da_load_row<VEC>(g.G + row * g.ldg, ln, r.G);
  da_load_row<VEC>(g.out + row * g.ldo, ln, o);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    r.m[v] = g.m[row * g.H + ln.head[v]];
    r.rz[v] = 1.f / g.Z[row * g.H + ln.head[v]];
    r.D[v] = da_head_sum<LPR>(dot4(r.G[v], o[v]), g.LH);
  }
}

template <int VEC>
__device__ __forceinline__ void da_zero_row(float4 (&x)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) x[v] = da_zero4();
}
// the lane groups of a wave, a fixed butterfly
template <int LPR, int VEC>
__device__ __forceinline__ void da_wave_sum(float4 (&x)[VEC]) {
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
    for (int v = 0; v < VEC; ++v) da_add(x[v], da_shfl_xor(x[v], off));
}

// launch 1: one wave per chunk; the piece of every long row inside the chunk -> one partial record, the H F sums of the row's
// gradient.  (The zeroing and the butterfly are spelled out in both kernels, not da_zero_row and da_wave_sum: through the helpers,
// as K21 had them, 14 of K19's backward kernels came out reordered; spelled out, as K19 had them, 4 of K21's do.)
template <typename Fam, int LPR, int VEC>
__global__ __launch_bounds__(64) void da_bwd_long_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const auto key = Fam::key(g);
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int row, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    typename Fam::template Row<VEC> r;
    Fam::template bwd_load<LPR, VEC>(g, ln, row, r);
    float4 dx[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) dx[v] = da_zero4();
    Fam::template walk<LPR, VEC, 1>(g, ln, e0 + grp, e1, EPW, false, key, r, dx);     // (a piece of a long row is never lone)
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1)                   // lane groups of the wave, a fixed butterfly
#pragma unroll
      for (int v = 0; v < VEC; ++v) da_add(dx[v], da_shfl_xor(dx[v], off));
    if (grp == 0) da_store_row<VEC>(g.part + long_record(blockIdx.x, slot) * g.pstride, ln, dx);
  });
}

// launch 2: one lane group per row
template <typename Fam, int LPR, int VEC>
__global__ __launch_bounds__(256) void da_bwd_row_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (row >= g.n) return;                                      // (whole lane groups; nothing below crosses a group)
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
  float4 dx[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) dx[v] = da_zero4();
  if (end - start > LONG_ROW) {
    for_long_records(start, end, [&](int64_t rec) {
      const float* p = g.part + rec * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v) da_add(dx[v], ld4(p + ln.ofs[v]));
    });
  } else if (end > start) {                                    // (a row without entries: its G row is not read)
    typename Fam::template Row<VEC> r;
    Fam::template bwd_load<LPR, VEC>(g, ln, row, r);
    Fam::template walk<LPR, VEC, 1>(g, ln, start, end, 1, Fam::lone(start, end), Fam::key(g), r, dx);
  }
  da_store_row<VEC>(g.dq + row * g.lddq, ln, dx);
}

// --------------------------------------------------------------------------------------------------------------------------- host
// the shapes all three families take; pad_hint: how the family's caller reaches an allowed F
static int da_check_shape(const char* what, int64_t nnz, int H, int F, const char* pad_hint) {
  PYGAT_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31), "%s: nnz %lld outside [0, 2^31) (int32 entry indexing)", what, (long long)nnz);
  PYGAT_REQUIRE(H >= 1 && H <= 64, "%s: H=%d heads outside [1, 64]", what, H);
  PYGAT_REQUIRE(F >= 4 && F <= 256 && (F & (F - 1)) == 0, "%s: F=%d, a head's width must be a power of two in 4..256 (%s)", what, F,
                pad_hint);
  PYGAT_REQUIRE((int64_t)H * F <= DA_MAX_ROW, "%s: row too wide: H x F = %d x %d > %d floats", what, H, F, DA_MAX_ROW);
  return PYGAT_OK;
}

// the mask of the DROP launchers of all three families: the seed, a uint64 in device memory (8-byte loads), and p in [0, 1] (a NaN is
// outside)
struct DaDrop {
  float p;
  const void* seed;
  uint32_t stream_id;
};
static int da_check_drop(const char* what, const DaDrop& d, DropRng* rng) {
  PYGAT_REQUIRE(d.seed, "%s: null seed", what);
  PYGAT_REQUIRE((reinterpret_cast<uintptr_t>(d.seed) & 7u) == 0, "%s: seed must be 8-byte aligned", what);
  PYGAT_REQUIRE(make_rng(d.p, d.seed, d.stream_id, rng), "%s: p=%g outside [0, 1]", what, (double)d.p);
  return PYGAT_OK;
}

// the per-entry rows of the EDGE launchers of K19 and K21: e, and de where it is asked for, are row tables like the gathered ones,
// [nnz x H*F] at the caller's entry index; e is non-null where there are entries.  e_align: 16, or 8 where e is rows of bf16 values
// (K21's inference forward; the pointer then only stands for them)
struct DaEdge {
  const float* e;
  int64_t lde;
  float* de;                   // backward rows only; null: not asked for
  int64_t ldde;
};
static int da_check_edge(const char* what, int64_t nnz, int HF, const DaEdge& ed, int e_align = 16) {
  if (nnz > 0 || ed.e) DA_TABLE_ALIGNED(what, "e", ed.e, ed.lde, HF, e_align);
  if (ed.de) DA_TABLE(what, "de", ed.de, ed.ldde, HF);
  return PYGAT_OK;
}

// the long-row records of a pass, in floats: the workspace of K19 and K20, the front of K21's
static inline int64_t da_part_floats(int64_t nnz, int H, int F) { return long_records(nnz) * da_pstride(H, F); }

// a kernel name of pygat_kernel_footprint, <prefix>{fwd,bwd,col}_{long,row}_l<LPR>v<VEC> with a lane shape of PYGAT_DA_DISPATCH ->
// true, pass 0 | 1 | 2 in that order; anything else -> false
struct DaKernelName {
  int pass;
  bool lng;
  int lpr, vec;
};
static bool da_parse_kernel_name(const char* name, const char* prefix, DaKernelName* k) {
  char dir[8] = "", kind[8] = "", rest = 0;
  int lpr = 0, vec = 0;
  const size_t np = strlen(prefix);
  if (strncmp(name, prefix, np) || sscanf(name + np, "%3[a-z]_%4[a-z]_l%dv%d%c", dir, kind, &lpr, &vec, &rest) != 4) return false;
  const int pass = !strcmp(dir, "fwd") ? 0 : (!strcmp(dir, "bwd") ? 1 : (!strcmp(dir, "col") ? 2 : -1));
  if (pass < 0 || (strcmp(kind, "long") && strcmp(kind, "row"))) return false;
  if (lpr < 1 || lpr > 64 || (lpr & (lpr - 1)) || !(vec == 1 || (lpr == 64 && vec >= 2 && vec <= 4))) return false;
  *k = {pass, !strcmp(kind, "long"), lpr, vec};
  return true;
}

// the lane shape of a row of H x F floats and the grids of a pass over n rows: a wave per chunk, four waves of lane groups per block
struct DaGrid {
  int lpr, vec;
  unsigned chunks, blocks;
};
static inline DaGrid da_grid(int n, int64_t nnz, int H, int F) {
  DaGrid gd;
  int nch;
  da_pick(H, F, &gd.lpr, &gd.vec, &nch);
  gd.chunks = (unsigned)long_chunks(nnz);
  gd.blocks = (unsigned)cdiv(n, 4 * (64 / gd.lpr));
  return gd;
}
// the piece kernel where there are long rows, then the row kernel
static inline void da_launch_pair(const void* long_kernel, const void* row_kernel, DaArgs& g, unsigned chunks, unsigned blocks,
                                  void* stream) {
  void* args[] = {&g};
  if (chunks) (void)hipLaunchKernel(long_kernel, dim3(chunks), dim3(64), args, 0, (hipStream_t)stream);
  (void)hipLaunchKernel(row_kernel, dim3(blocks), dim3(256), args, 0, (hipStream_t)stream);
}

}  // namespace pygat
