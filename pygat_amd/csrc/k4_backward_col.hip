// K4 -- backward, column pass: dWh, dt (gfx950, wave64).
//
// Replaces `grad_b = a.t().matmul(grad_output)` of SpecialSpmmFunction.backward (reference
// layers.py:89) -- the transposed SpMM -- plus the autograd of the two a-halves matmuls
// (layers.py:60-61):
//     dWh_j = sum_i alpha~_ij Gp_i + ds_j a_src + dt_j a_dst        alpha~ = alpha * dropout mask
//     dt_j  = sum_i dz_ij                                            (column sums of dz)
// nnz split over the TRANSPOSED pattern: a slot walks transposed edges (j <- i) and gathers ONE
// contiguous row per edge, GR_i = [Gp_i | (s_i, m_i, 1/Z_i, D_i) per head]; with the row-local Wh_j
// (and t_j = Wh_j . a_dst) it recomputes alpha_ij and dz_ij in registers instead of reading a
// per-edge buffer through the edge permutation.  ds comes from K3b.  Rows cut by a slot border go
// through `part` + a fix-up launch (fixed order).  No atomics.
#include "attn_common.h"
#include "tail_stream.h"

namespace pygat {

struct ColArgs {
  GraphDev g;  // transposed pattern: rc[k] = (j, i) for the forward edge (i, j)
  RowShape rs;
  float alpha;
  const int32_t* perm;  // transposed position -> forward edge (only to index the dropout mask)
  const float* mask;    // [nnz][H] attention dropout mask in FORWARD edge order, or nullptr
  const float* Wh;
  const float* GR;
  int64_t ldgr;         // row stride of GR
  const float* a_pad;
  const float* ds;      // row sums from the row pass K3b, or nullptr: then the ds_j a_src term is left out here
  float* dz_t;          // [nnz][Htot] or nullptr: dz of every TRANSPOSED edge, for the row-sum pass that follows
  float* dWh;
  float* dt;
  float* part;  // [2 * nslots][R + 2H]: acc[R], dt[H]
  float* da_part;  // DA instantiations: [work-groups][2 R] = (sum ds_j Wh_j | sum dt_j Wh_j) over the rows the work-group finished
};

#ifndef PYGAT_DIAG_K4
#define PYGAT_DIAG_K4 0   // tools/build_variant.sh only: bit 0 no LDS sums, bit 1 no Wh_j load either (then da is wrong, the time is the point)
#endif

// CR > 0 (with LPH > 0, VEC == 1): dense row tables of CR floats, heads of 4 LPH columns -- constant strides
// DA (round 4): the attention-vector gradient da_src = sum_j ds_j Wh_j, da_dst = sum_j dt_j Wh_j (autograd of layers.py:60-61,
// a.mm(edge_h) layers.py:144) taken HERE, where row j finishes with dt_j just formed, ds_j loaded for the dWh term and Wh_j in
// L1 from the row's edges -- instead of by a pass of its own that streams Wh, ds and dt again (pygat_a_grad: 0.6 GB, 0.12 ms
// at config 5).  The 8 running sums of a lane live in LDS (da_lds[0], da_lds[da_stride]: its own two float4s, no other lane
// touches them), not in registers: the kernel sits at 122 of the 128 VGPRs that keep four waves per SIMD.
template <int VEC, int LPH = 0, int CR = 0, bool DA = false>
__device__ __forceinline__ void col_finish(const ColArgs& a, const LaneCols<VEC>& lc, int j,
                                           const float4 (&acc)[VEC], const float (&dt)[VEC], float4* da_lds = nullptr,
                                           int da_stride = 0) {
  const int Fp = CR ? 4 * LPH : a.rs.Fp;
  const int64_t ldr = CR ? CR : a.rs.ldr, ldh = CR ? CR / (4 * (LPH ? LPH : 1)) : a.rs.ldh;
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (!lc.valid[v]) continue;
    const int co = lc.cofs[v], h = lc.head[v], f0 = co & (Fp - 1);
    const float dsj = a.ds ? a.ds[(int64_t)j * ldh + h] : 0.f;
    const float4 as = ld4(a.a_pad + (int64_t)h * 2 * Fp + f0);
    const float4 ad = ld4(a.a_pad + (int64_t)h * 2 * Fp + Fp + f0);
    // DA: Wh_j, fetched HERE, with the other loads of the flush and before its stores -- vmcnt counts loads and stores
    // together in issue order (issued behind the dWh / dt stores, the wait for this load was a wait for their
    // acknowledgement from HBM: K4 1.21 -> 2.12 ms in the first build of this path, round 4 run r4b).  The fetch is
    // not free even so: the row comes from L2, not L1 (16 waves of 640-byte gathers turn the 32 KB L1 over every round), and
    // one more 512-byte read per finished row cost K4 0.05 ms (diagnostic builds, round 4 run r4f).  Taking the row from the
    // caller's registers instead, where the finished row's last edge was gathered in the same round of U edges (three
    // flushes of four), was measured and removed: the longer-lived rows cost 36 bytes of scratch at four waves (K4 1.26 ->
    // 1.39 ms) or the fourth wave at 144 VGPRs (1.38 ms; round 4 run r4g; DESIGN_HISTORY.md section 8).
    // (In a lambda, which hipcc folds in only after its early CSE: the row offset j * ldr is then not merged up front with
    // the dWh store's, and the da instantiation keeps, instruction for instruction, the schedule its figures were measured
    // on.  Written as a plain expression one address shift moves two instructions down.)
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (DA && !(PYGAT_DIAG_K4 & 2)) w = [&] { return ld4(a.Wh + (int64_t)j * ldr + co); }();
    float4 o;
    o.x = acc[v].x + dsj * as.x + dt[v] * ad.x;
    o.y = acc[v].y + dsj * as.y + dt[v] * ad.y;
    o.z = acc[v].z + dsj * as.z + dt[v] * ad.z;
    o.w = acc[v].w + dsj * as.w + dt[v] * ad.w;
    if constexpr (DA) {
      static_assert(VEC == 1, "da accumulation: one chunk per lane");
      // Read-modify-write of the lane's own two float4s, ONE AFTER THE OTHER (the fence keeps hipcc from fetching both up
      // front: with both in flight the kernel's peak is 130 VGPRs = three waves per SIMD instead of four).  Only this lane
      // touches these eight words, in program order: the sums are as reproducible as register accumulators.
      // (ds_add_f32 instead -- one product register at a time, 128 VGPRs -- was measured and removed: LDS float atomics
      // retire about one lane per clock, K4 1.20 -> 2.14 ms; round 4 runs r4b / r4c)
#if PYGAT_DIAG_K4 & 1     /* diagnostic builds only: the Wh_j load without the LDS sums */
      asm volatile("" :: "v"(w.x), "v"(w.y), "v"(w.z), "v"(w.w));
#else
      {
        float4 x = da_lds[0];
        x.x = fmaf(dsj, w.x, x.x); x.y = fmaf(dsj, w.y, x.y); x.z = fmaf(dsj, w.z, x.z); x.w = fmaf(dsj, w.w, x.w);
        da_lds[0] = x;
      }
      {
        float4 y = da_lds[da_stride];
        y.x = fmaf(dt[v], w.x, y.x); y.y = fmaf(dt[v], w.y, y.y); y.z = fmaf(dt[v], w.z, y.z); y.w = fmaf(dt[v], w.w, y.w);
        da_lds[da_stride] = y;
      }
#endif
    }
    st4(a.dWh + (int64_t)j * ldr + co, o);
    if (((co >> 2) & (a.rs.lph - 1)) == 0) a.dt[(int64_t)j * ldh + h] = dt[v];
  }
}

template <int VEC, int LPH = 0, int CR = 0, bool DA = false>
__device__ __forceinline__ void col_flush(const ColArgs& a, const LaneCols<VEC>& lc, int64_t q, int j,
                                          bool is_head, bool is_tail, const float4 (&acc)[VEC],
                                          const float (&dt)[VEC], float4* da_lds = nullptr, int da_stride = 0) {
  if (is_head || is_tail) {
    // (the slot id is looked up again HERE, in the rare cut-row branch: kept live through the walk -- it no longer follows
    // from the block and thread ids alone once a slot_order is allowed -- it cost the 8 x 16 da instantiation 12 bytes of scratch)
    const int64_t k = slot_at(a.g, q);
    float* p = a.part + (2 * k + (is_head ? 0 : 1)) * (int64_t)(a.rs.R + 2 * a.rs.H);
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      if (!lc.valid[v]) continue;
      st4(p + lc.cofs[v], acc[v]);
      if (((lc.cofs[v] >> 2) & (a.rs.lph - 1)) == 0) p[a.rs.R + lc.head[v]] = dt[v];
    }
  } else {
    col_finish<VEC, LPH, CR, DA>(a, lc, j, acc, dt, da_lds, da_stride);
  }
}

// one of U registers by a runtime index (U = 2 or 4)
template <int U, typename T>
__device__ __forceinline__ T pick(const T (&x)[U], int u) {
  T r = x[0];
#pragma unroll
  for (int q = 1; q < U; ++q) r = (u == q) ? x[q] : r;
  return r;
}

// WRITE_DZ: this pass computes every dz_ij anyway (for dt_j); written out per transposed edge (sequential
// 4H-byte records) they let the row sums ds_i = sum_j dz_ij be taken by a light pass that fetches the
// records through perm_f (pygat_gat_backward_rowsum) instead of the row pass K3b, which gathers a whole
// Wh_j row per forward edge just to recompute them.  (Scattering the records to their forward positions
// here, so that the row sums become a pure stream, was measured too: the random 32-byte stores cost K4
// 0.48 ms and saved 0.10 ms there.)
// The lanes of a head all hold dz for the U edges of a round: lane (u mod S) of the head stores edge u.
// LPH > 0: lanes per head known at compile time (0: read from the shape): the two head sums per edge are DPP chains
// whose length otherwise costs a scalar branch per step.
#ifndef PYGAT_K4_DA_WAVES
#define PYGAT_K4_DA_WAVES 4         // minimum waves per SIMD asked of the dense 8 x 16 instantiation that takes da along
#endif
#ifndef PYGAT_K4_QUAD_LOADS
#define PYGAT_K4_QUAD_LOADS 1       // heads of one DPP quad (LPH == 4), 4 edges per round: lane q of a quad loads edge q's record and row record, quad_bcast hands them round (0: every lane loads all four; 1: the dense instantiations, CR > 0; 2: those with run-time strides too)
#endif
#ifndef PYGAT_K4_QUAD_PREFETCH
#define PYGAT_K4_QUAD_PREFETCH 1    // on top of PYGAT_K4_QUAD_LOADS: the next round's edge records (one int2 per lane) fetched a round ahead, as K2 does
#endif
#ifndef PYGAT_K4_HEADLINE_WAVES
#define PYGAT_K4_HEADLINE_WAVES 1   // (experiment: minimum waves per SIMD asked of the CR > 0 instantiation)
#endif
template <int LPR, int VEC, bool WRITE_DZ, int LPH, int CR, bool DA>
__device__ __forceinline__ void col_walk(const ColArgs& a, const int64_t q, float4* da_lds, int da_stride) {
  const int64_t k = slot_at(a.g, q);   // grid position -> slot (pygat_graph.slot_order; identity without one)
  // narrow rows: next round's edge records prefetched (see gat_fwd_kernel; 8 edges per round were measured too: two rows
  // per edge in registers leave 2 waves per SIMD at U = 8, 0.30 -> 0.35 ms at one head of 16)
#ifndef PYGAT_K4_PREFETCH_ALL
#define PYGAT_K4_PREFETCH_ALL 0   // experiment (tools/build_variant.sh): edge-record prefetch on one-chunk rows of any width
#endif
  constexpr bool NARROW = (VEC == 1 && LPR <= 8) || (PYGAT_K4_PREFETCH_ALL && VEC == 1);
  constexpr int U = (VEC == 1) ? 4 : 2;
  const SlotView sl = open_slot(a.g, k);
  const int64_t e0 = sl.e0, e1 = sl.e1;
  const int2* __restrict__ rc = a.g.rc;
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(a.rs);
  const int R = CR ? CR : a.rs.R;
  constexpr int HC = CR / (4 * (LPH ? LPH : 1));   // heads, when CR > 0
  const int64_t RW = CR ? CR + 4 * HC : a.ldgr, ldr = CR ? CR : a.rs.ldr, ldh = CR ? HC : a.rs.ldh;
  const int lph = LPH > 0 ? LPH : (a.rs.lph < 64 ? a.rs.lph : 64);
  float4 adst[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    adst[v] = ld4(a.a_pad + (int64_t)lc.head[v] * 2 * a.rs.Fp + a.rs.Fp + (lc.cofs[v] & (a.rs.Fp - 1)));
    if (!lc.valid[v]) adst[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  int cur = sl.r_first;
  float4 acc[VEC];
  float dt[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { acc[v] = make_float4(0.f, 0.f, 0.f, 0.f); dt[v] = 0.f; }

  // QUAD: the operands of a round that are the same in all lanes of a head -- the edge records and the (s, m, 1/Z, D) record of
  // the gathered row -- are loaded once per quad instead of once per lane: a head is one DPP quad and a round has four edges,
  // so lane q of the quad loads edge q's copy (one instruction for the round) and quad_bcast hands the four round.  16 -> 10
  // vector-memory instructions per round; the addresses read (the row's fifth line among them), the arithmetic and its order
  // are the same.  A quad lies inside one lane group: its lanes are switched on and off together.
  // QPREF: with one record per lane, the next round's are fetched a round ahead, as in gat_fwd_kernel.
  // (The instantiations with run-time strides, CR == 0, take it at PYGAT_K4_QUAD_LOADS=2 only: their 64-bit row addresses
  // push them from 126 to 130 VGPRs, the fourth wave per SIMD, and 6 heads x 16 measured no gain: DESIGN.md section 8.)
  constexpr bool QUAD = (PYGAT_K4_QUAD_LOADS >= (CR > 0 ? 1 : 2)) && LPH == 4 && VEC == 1 && U == 4 && !WRITE_DZ && !NARROW;
  constexpr bool QPREF = QUAD && PYGAT_K4_QUAD_PREFETCH;
  const int ql = (int)(threadIdx.x & 3);
  int2 pn[NARROW ? U : 1];
  if constexpr (NARROW) {
#pragma unroll
    for (int u = 0; u < U; ++u) pn[u] = rc[(e0 + u < e1) ? e0 + u : e1 - 1];
  } else if constexpr (QPREF) {
    pn[0] = rc[(e0 + ql < e1) ? e0 + ql : e1 - 1];
  }
  for (int64_t e = e0; e < e1; e += U) {
    int2 p[U];  // (j, i): j = this (transposed) row, i = the forward row that attends to j
    int2 pq = make_int2(0, 0);   // QUAD: the record of edge e + ql
    if constexpr (QUAD) {
      if constexpr (QPREF) pq = pn[0];
      else pq = rc[(e + ql < e1) ? e + ql : e1 - 1];
      quad_spread(pq, p);
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (NARROW) p[u] = pn[u];
        else p[u] = rc[(e + u < e1) ? e + u : e1 - 1];
      }
    }
    float4 rt[U][VEC], gv[U][VEC], wv[U][VEC];
    float mk[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if constexpr (CR > 0) {   // both tables below 4 GiB (checked at launch): 32-bit element offsets from a scalar base
          // (measured and dropped, gpurun_out r4h / r4i: without the record read -- 128 of the row's 640 bytes, its fifth line --
          // K4 runs 1.24 -> 1.07 ms; from a table of its own (128 MB, Infinity-Cache sized) the records cost the same 0.17 ms:
          // the price is the gathered line, wherever it lies)
          const uint32_t go = (uint32_t)p[u].y * (uint32_t)RW;
          gv[u][v] = ld4(a.GR + (go + (uint32_t)lc.cofs[v]));
          if constexpr (!QUAD)
            rt[u][v] = (PYGAT_DIAG_K4 & 8) ? gv[u][v] : ld4(a.GR + (go + (uint32_t)(R + 4 * lc.head[v])));   // (bit 3: diagnostic, no scalar-record read)
          wv[u][v] = ld4(a.Wh + ((uint32_t)((PYGAT_DIAG_K4 & 4) ? (p[u].x & 63) : p[u].x) * (uint32_t)ldr + (uint32_t)lc.cofs[v]));   // (bit 2: diagnostic, row-local reads from 64 cached rows)
        } else {
        const float* gr = a.GR + (int64_t)p[u].y * RW;           // gathered: one contiguous row
        gv[u][v] = ld4(gr + lc.cofs[v]);
        if constexpr (!QUAD) rt[u][v] = ld4(gr + R + 4 * lc.head[v]);
        wv[u][v] = ld4(a.Wh + (int64_t)p[u].x * ldr + lc.cofs[v]);  // row-local (L1 after the first edge)
        }
        mk[u][v] = 1.f;
        if (a.mask) mk[u][v] = a.mask[(int64_t)a.perm[(e + u < e1) ? e + u : e1 - 1] * ldh + lc.head[v]];
      }
    if constexpr (QUAD) {   // the record of the row edge e + ql gathers, this lane's head
      float4 rq;
      if constexpr (CR > 0) {
        if constexpr (PYGAT_DIAG_K4 & 8) rq = make_float4(0.f, 0.f, 0.f, 0.f);   // (bit 3: diagnostic, no scalar-record read)
        else rq = ld4(a.GR + ((uint32_t)pq.y * (uint32_t)RW + (uint32_t)(R + 4 * lc.head[0])));
      } else {
        rq = ld4(a.GR + (int64_t)pq.y * RW + R + 4 * lc.head[0]);
      }
      if constexpr (QPREF) pn[0] = rc[(e + U + ql < e1) ? e + U + ql : e1 - 1];   // next round's records, behind this round's rows
      if constexpr (CR > 0 && (PYGAT_DIAG_K4 & 8)) {
        rt[0][0] = gv[0][0]; rt[1][0] = gv[1][0]; rt[2][0] = gv[2][0]; rt[3][0] = gv[3][0];
      } else {
        rt[0][0] = quad_bcast4<0>(rq); rt[1][0] = quad_bcast4<1>(rq); rt[2][0] = quad_bcast4<2>(rq); rt[3][0] = quad_bcast4<3>(rq);
      }
    }
    if constexpr (NARROW) {
#pragma unroll
      for (int u = 0; u < U; ++u) pn[u] = rc[(e + U + u < e1) ? e + U + u : e1 - 1];
    }
    float al[U][VEC], dz[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float dp = group_sum_rt(lc.valid[v] ? dot4(gv[u][v], wv[u][v]) : 0.f, lph);
        const float tj = group_sum_rt(dot4(wv[u][v], adst[v]), lph);
        const float zz = rt[u][v].x + tj;
        const float ev = zz > 0.f ? zz : a.alpha * zz;
        const float a0 = __expf(ev - rt[u][v].y) * rt[u][v].z;
        dz[u][v] = a0 * (mk[u][v] * dp - rt[u][v].w) * (zz > 0.f ? 1.f : a.alpha);
        al[u][v] = a0 * mk[u][v];
      }
    if constexpr (WRITE_DZ) {
      const int S = lph < U ? lph : U;                  // lanes of a head that store (1, 2 or 4)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const int lih = (lc.cofs[v] >> 2) & (lph - 1);  // lane inside its head
#pragma unroll
        for (int u = 0; u < U; ++u)                      // lane (u mod S) of the head stores edge u
          if (lih == (u & (S - 1)) && lc.valid[v] && e + u < e1) a.dz_t[(e + u) * ldh + lc.head[v]] = dz[u][v];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u < e1) {
        if (p[u].x != cur) {
          col_flush<VEC, LPH, CR, DA>(a, lc, q, cur, slot_head_partial(sl, cur), false, acc, dt, da_lds, da_stride);
          cur = p[u].x;
#pragma unroll
          for (int v = 0; v < VEC; ++v) { acc[v] = make_float4(0.f, 0.f, 0.f, 0.f); dt[v] = 0.f; }
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          acc[v].x = fmaf(al[u][v], gv[u][v].x, acc[v].x); acc[v].y = fmaf(al[u][v], gv[u][v].y, acc[v].y);
          acc[v].z = fmaf(al[u][v], gv[u][v].z, acc[v].z); acc[v].w = fmaf(al[u][v], gv[u][v].w, acc[v].w);
          dt[v] += dz[u][v];
        }
      }
    }
  }
  col_flush<VEC, LPH, CR, DA>(a, lc, q, cur, slot_head_partial(sl, cur), slot_tail_partial(a.g, sl, cur), acc, dt, da_lds, da_stride);
}

template <int LPR, int VEC, bool WRITE_DZ, int LPH = 0, int CR = 0, bool DA = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(CR > 0 ? (DA ? PYGAT_K4_DA_WAVES : PYGAT_K4_HEADLINE_WAVES) : 1))) void gat_bwd_col_kernel(ColArgs a) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t k = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * EPW + lane / LPR;   // grid position (-> slot: col_walk)
  if constexpr (!DA) {
    if (k >= a.g.kn) return;
    col_walk<LPR, VEC, WRITE_DZ, LPH, CR, false>(a, k, nullptr, 0);
  } else {
    extern __shared__ __attribute__((aligned(16))) float4 da_sm[];   // [2][blockDim.x]: (src | dst) running sums, one pair per lane
    __shared__ int da_arrived;
    const int nt = (int)blockDim.x;
    float4* mine = da_sm + threadIdx.x;
    mine[0] = make_float4(0.f, 0.f, 0.f, 0.f); mine[nt] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x == 0) da_arrived = 0;
    __syncthreads();   // (at the START, where the waves stand together anyway: the counter below must be zero before its first add)
    if (k < a.g.kn) col_walk<LPR, VEC, WRITE_DZ, LPH, CR, true>(a, k, mine, nt);
    // No barrier at the end: a wave that is done leaves its SIMD slot; the LAST wave of the work-group to arrive adds the lane
    // groups, always in the same order (so the record does not depend on which wave that is).  Its workgroup-scope
    // acquire-release add comes after every other wave's LDS sums (theirs precede their own add in program order).
    int old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(&da_arrived, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old == (nt >> 6) - 1) {
      const int R = CR ? CR : a.rs.R;
      for (int idx = lane; idx < 2 * LPR; idx += 64) {     // (which, c): float4 c of the (src | dst) half
        const int which = idx / LPR, c = idx % LPR;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int g = 0; g < nt / LPR; ++g) {
          const float4 x = da_sm[which * nt + g * LPR + c];
          t.x += x.x; t.y += x.y; t.z += x.z; t.w += x.w;
        }
        if (4 * c < R) st4(a.da_part + (int64_t)blockIdx.x * 2 * R + which * R + 4 * c, t);
      }
    }
  }
}

// Merge of one cut row (the counterpart of fwd_merge_row): its pieces tail(k), head(k + 1), ..., head(k + npieces - 1) are
// dealt round-robin to nw (1, or the NW waves of the work-group when `wide`) waves x G lane groups, PF records in flight each,
// summed inside a wave with shuffles and across waves through LDS, always in the same order.
// G: a wide row has the whole wave (64 / LPR lane groups); otherwise GP lane groups share a row and 64 / LPR / GP rows lie side
// by side in the wave, each lane group with its own k, r, npieces (the packed entries of the list).  `wide` is work-group
// uniform and then every wave of the work-group calls; a row that is not wide is merged by the one wave that calls, as wave 0.
template <int LPR, int VEC, int NW, int GP = 64 / LPR>
__device__ __forceinline__ void col_merge_row(const ColArgs& a, const LaneCols<VEC>& lc, float* fix_sm, int64_t k, int r,
                                              int npieces, bool wide, int w) {
  constexpr int EPW = 64 / LPR;
  constexpr int PF = (VEC == 1) ? 4 : 2;
  const int slot = (threadIdx.x & 63) / LPR;
  const int G = wide ? EPW : GP, g = slot % G;
  const int64_t PS = a.rs.R + 2 * a.rs.H;
  float4 acc[VEC];
  float dt[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) { acc[v] = make_float4(0.f, 0.f, 0.f, 0.f); dt[v] = 0.f; }
  {
    const int nw = wide ? NW : 1;
    for (int q = (wide ? w : 0) * G * PF + g; q < npieces; q += nw * G * PF) {
      float4 xp[PF][VEC];
      float tp[PF][VEC];
#pragma unroll
      for (int f = 0; f < PF; ++f) {
        const int qq = q + f * G;
        const int qc = qq < npieces ? qq : q;   // clamped: the loads stay unconditional
        const float* p = a.part + piece_record(k, qc) * PS;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          xp[f][v] = ld4(p + lc.cofs[v]); tp[f][v] = p[a.rs.R + lc.head[v]];
        }
      }
#pragma unroll
      for (int f = 0; f < PF; ++f)
        if (q + f * G < npieces) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            acc[v].x += xp[f][v].x; acc[v].y += xp[f][v].y; acc[v].z += xp[f][v].z; acc[v].w += xp[f][v].w;
            dt[v] += tp[f][v];
          }
        }
    }
    if (wide) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        acc[v] = slot_sum4<LPR>(acc[v]);
        dt[v] = slot_sum<LPR>(dt[v]);
      }
    } else {
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        acc[v] = slot_sum4<LPR, LPR * GP>(acc[v]);
        dt[v] = slot_sum<LPR, LPR * GP>(dt[v]);
      }
    }
  }
  if (wide) {
    if (slot == 0) {
      float* p = fix_sm + w * PS;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (lc.valid[v]) {
          st4(p + lc.cofs[v], acc[v]);
          if (((lc.cofs[v] >> 2) & (a.rs.lph - 1)) == 0) p[a.rs.R + lc.head[v]] = dt[v];
        }
    }
    __syncthreads();
    if (w == 0 && slot == 0) {
#pragma unroll
      for (int ww = 1; ww < NW; ++ww) {
        const float* p = fix_sm + ww * PS;
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const float4 x = ld4(p + lc.cofs[v]);
          acc[v].x += x.x; acc[v].y += x.y; acc[v].z += x.z; acc[v].w += x.w;
          dt[v] += p[a.rs.R + lc.head[v]];
        }
      }
    }
    __syncthreads();
  }
  if (w == 0 && g == 0 && npieces > 0) col_finish<VEC>(a, lc, r, acc, dt);
}

// Fix-up of cut rows without a list (same scheme as gat_fwd_fixup_kernel): a work-group screens FIX_SCREEN slots and its 4 waves
// merge every cut row they own in turn.
template <int LPR, int VEC>
__global__ __launch_bounds__(256) void gat_bwd_col_fixup_kernel(ColArgs a) {
  constexpr int EPW = 64 / LPR;
  constexpr int PF = (VEC == 1) ? 4 : 2;
  extern __shared__ __attribute__((aligned(16))) float fix_sm[];  // [4][R + 2H]
  const int w = threadIdx.x >> 6;
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(a.rs);
  screen_cut_rows(a.g, (int64_t)blockIdx.x * FIX_SCREEN, num_slots(a.g), [&](int64_t k, int r, int npieces) {
    const bool wide = npieces > EPW * PF;  // more pieces than one wave takes in a single round
    if (wide || w == 0) col_merge_row<LPR, VEC, 4>(a, lc, fix_sm, k, r, npieces, wide, w);
  });
}

// list-driven variant: entry q of g.cut = (owner slot k, row, pieces); the first n_cut_wide entries (long
// chains) get a whole work-group each, the others are packed fix_rows_per_wave(LPR) to a wave.
// (the body, for work-group `bid` of the fix-up's grid: also run by the leading work-groups of gat_bwd_col_finish_kernel)
template <int LPR, int VEC>
__device__ __forceinline__ void col_fixup_list_body(const ColArgs& a, const int bid) {
  constexpr int RPW = fix_rows_per_wave(LPR), GP = 64 / LPR / RPW;
  extern __shared__ __attribute__((aligned(16))) float fix_sm[];  // [FIX_LIST_WAVES][R + 2H]
  const int w = threadIdx.x >> 6;
  const bool wide = bid < a.g.n_cut_wide;   // (block-uniform)
  const int q0 = wide ? bid
                      : a.g.n_cut_wide + ((bid - a.g.n_cut_wide) * FIX_LIST_WAVES + w) * RPW + ((threadIdx.x & 63) / LPR) / GP;
  const bool have = q0 < a.g.n_cut;
  const int qe = have ? q0 : a.g.n_cut - 1;
  const int64_t k = a.g.cut[3 * qe];
  const int r = a.g.cut[3 * qe + 1];
  const int npieces = have ? a.g.cut[3 * qe + 2] : 0;
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(a.rs);
  col_merge_row<LPR, VEC, FIX_LIST_WAVES, GP>(a, lc, fix_sm, k, r, npieces, wide, wide ? w : 0);
}

template <int LPR, int VEC>
__global__ __launch_bounds__(64 * FIX_LIST_WAVES) void gat_bwd_col_fixup_list_kernel(ColArgs a) {
  col_fixup_list_body<LPR, VEC>(a, (int)blockIdx.x);
}

// The fix-up and the backward stream of the self-loop-only tail (tail_stream.h) in ONE launch: work-groups [0, fix_blocks)
// are the list-driven fix-up's, the ones behind them stream the tail, one 16-byte chunk per thread.  The branch is
// block-uniform and no work-group waits for another: the two bodies write disjoint rows of dWh, ds and dt (cut rows lie
// before the tail, whose rows have one edge each), and neither reads what the other writes.  The fix-up is latency per wave
// (a few hundred work-groups, a chain of dependent loads each), the stream is bytes: dispatched first, the fix-up's
// work-groups are resident while the stream runs, instead of owning a place in the launch sequence.
struct ColTailArgs {
  int row_first, n_rows, Fo, flags;
  const float* G;
  const float* y;
  const int32_t* urow;
  float* ds;
};
template <int LPR, int VEC>
__global__ __launch_bounds__(64 * FIX_LIST_WAVES) void gat_bwd_col_finish_kernel(ColArgs a, ColTailArgs t, int fix_blocks) {
  if ((int)blockIdx.x < fix_blocks) {   // (block-uniform)
    col_fixup_list_body<LPR, VEC>(a, (int)blockIdx.x);
  } else {
    bwd_tail_item(((int64_t)blockIdx.x - fix_blocks) * (64 * FIX_LIST_WAVES) + threadIdx.x, t.row_first, t.n_rows, a.rs.H, t.Fo,
                  a.rs.Fp, t.flags, t.G, t.y, t.urow, a.dWh, a.rs.ldr, 0, t.ds, a.dt);
  }
}


}  // namespace pygat

using namespace pygat;


namespace pygat {
int footprint_k4_headline_da(int* regs, int* scratch) {   // (pygat_kernel_footprint)
  return kernel_footprint_of(reinterpret_cast<const void*>(&gat_bwd_col_kernel<32, 1, false, 4, 128, true>), regs, scratch);
}
}  // namespace pygat

extern "C" size_t pygat_gat_backward_col_da_bytes(const pygat_graph* gT, int H, int Fo, int head_group) {
  GraphDev g;
  if (!gT || check_graph(gT, &g, 2) != PYGAT_OK) return 0;
  const int Fp = padded_width(Fo);
  if (H <= 0 || Fp <= 0) return 0;
  return (size_t)col_da_blocks(g, H, Fp, head_group_arg(head_group, g.n, H, Fp), nullptr) * 2 * (size_t)H * Fp * sizeof(float);
}

// phase: 0 = both launches, PYGAT_F_MAIN_ONLY / PYGAT_F_FIXUP_ONLY = one of them (pygat_gat_backward_col_phase)
static int backward_col(const pygat_graph* gT, const int32_t* perm_t, int H, int Fo, float alpha,
                        const float* Wh, const float* a_pad, const float* GR,
                        const float* att_mask, const float* ds, float* dWh, float* dt, float* dz_t,
                        void* part, float* da_part, int h_first, int h_count, int head_group, int phase, void* stream) {
  ColArgs a;
  int rc = check_graph(gT, &a.g, 2);
  if (rc) return rc;
  const int Fp = padded_width(Fo);
  HeadRange rg;
  PYGAT_REQUIRE(H > 0 && Fp > 0, "gat_backward_col: unsupported H=%d F'=%d", H, Fo);
  PYGAT_REQUIRE(make_head_range(H, h_first, h_count, &rg), "gat_backward_col: bad head range [%d, +%d) of %d", h_first, h_count, H);
  PYGAT_REQUIRE(Wh && a_pad && GR && dWh && dt && part, "gat_backward_col: null pointer");
  PYGAT_REQUIRE((ds != nullptr) != (dz_t != nullptr),
                "gat_backward_col: pass either ds (row sums known) or dz_t (row sums taken afterwards), not both");
  PYGAT_REQUIRE(!att_mask || perm_t, "gat_backward_col: an attention mask needs perm_t (mask is in forward edge order)");
  PYGAT_REQUIRE(aligned16(Wh) && aligned16(GR) && aligned16(dWh) && aligned16(a_pad) && aligned16(part),
                "gat_backward_col: row tables must be 16-byte aligned");
  const int hg = head_group_arg(head_group, a.g.n, rg.hr, Fp);
  PYGAT_REQUIRE(hg > 0, "gat_backward_col: head_group=%d gives rows of more than 1024 floats per pass", head_group);
  PYGAT_REQUIRE(phase == 0 || phase == PYGAT_F_MAIN_ONLY || phase == PYGAT_F_FIXUP_ONLY,
                "gat_backward_col: phase=%d (0, PYGAT_F_MAIN_ONLY or PYGAT_F_FIXUP_ONLY)", phase);
  // (one phase: the partial records of ONE window must outlive the call -- the windows of a wider level share `part`)
  PYGAT_REQUIRE(phase == 0 || hg >= rg.hr, "gat_backward_col: a single phase needs the level in one head window (pygat_gat_backward_col_phases_ok)");
  const bool do_main = phase != PYGAT_F_FIXUP_ONLY, do_fix = phase != PYGAT_F_MAIN_ONLY;
  if (da_part) {
    PYGAT_REQUIRE(ds && rg.hr == H && aligned16(da_part) && col_da_blocks(a.g, H, Fp, hg, nullptr) > 0,
                  "gat_backward_col: da_part needs ds, 8 heads x 16 in one pass and a cut-row list "
                  "(pygat_gat_backward_col_da_bytes() == 0 otherwise)");
  }
  a.da_part = da_part;
  hipStream_t st = (hipStream_t)stream;
  const int64_t nslots = a.g.kn;   // all slots, or the prefix before a self-loop-only tail (pygat_gat_backward_col_tail)
  PYGAT_REQUIRE(a.g.kn == num_slots(a.g) || (a.g.cut && !a.g.order), "gat_backward_col: a slot prefix needs the cut-row list and no slot_order");
  for (int h0 = 0; h0 < rg.hr; h0 += hg) {
    const int hc = (rg.hr - h0 < hg) ? rg.hr - h0 : hg;
    const int gh = rg.hb + h0;
    PYGAT_REQUIRE(make_window_shape(H, Fo, hc, &a.rs), "gat_backward_col: unsupported H=%d F'=%d", hc, Fo);
    a.alpha = alpha; a.perm = perm_t; a.mask = att_mask ? att_mask + gh : nullptr;
    a.Wh = Wh + (int64_t)gh * Fp; a.GR = GR + gr_window_offset(h0, Fp); a.ldgr = (int64_t)rg.hr * Fp + 4 * rg.hr;
    a.a_pad = a_pad + (int64_t)gh * 2 * Fp; a.ds = ds ? ds + gh : nullptr; a.dz_t = dz_t ? dz_t + gh : nullptr;
    a.dWh = dWh + (int64_t)gh * Fp; a.dt = dt + gh; a.part = (float*)part;
    int lpr, vec;
    pick_lanes(a.rs, &lpr, &vec);
    const MainGrid mg = main_grid(nslots, lpr, vec);
    const unsigned bt = mg.bt, blocks = mg.blocks;
    const size_t da_lds = da_part ? 2 * (size_t)bt * sizeof(float4) : 0;
    if (!do_main) {   // (the fix-up phase alone)
    } else if (dz_t) {
      PYGAT_DISPATCH_LANES(lpr, vec,
                           hipLaunchKernelGGL((gat_bwd_col_kernel<LPR, VEC, true>), dim3(blocks), dim3(bt), 0, st, a));
    } else if (lpr == 32 && vec == 1 && a.rs.lph == 4) {   // 8 heads x 16: the headline shape
      const bool dense = a.rs.R == 128 && a.rs.ldr == 128 && a.rs.ldh == 8 && a.ldgr == 160 && a.rs.H == 8 && !att_mask &&
                         (int64_t)a.g.n * 160 * 4 < ((int64_t)1 << 32);
      if (dense && da_part)
        hipLaunchKernelGGL((gat_bwd_col_kernel<32, 1, false, 4, 128, true>), dim3(blocks), dim3(bt), da_lds, st, a);
      else if (dense)
        hipLaunchKernelGGL((gat_bwd_col_kernel<32, 1, false, 4, 128>), dim3(blocks), dim3(bt), 0, st, a);
      else if (da_part)   // (8 x 16 with an attention mask or a table of 4 GiB and more: run-time strides, 130 VGPRs)
        hipLaunchKernelGGL((gat_bwd_col_kernel<32, 1, false, 4, 0, true>), dim3(blocks), dim3(bt), da_lds, st, a);
      else
        hipLaunchKernelGGL((gat_bwd_col_kernel<32, 1, false, 4>), dim3(blocks), dim3(bt), 0, st, a);
    } else {
      PYGAT_DISPATCH_LANES(lpr, vec,
                           hipLaunchKernelGGL((gat_bwd_col_kernel<LPR, VEC, false>), dim3(blocks), dim3(bt), 0, st, a));
    }
    PYGAT_CHECK_LAUNCH("gat_backward_col");
    if (!do_fix) continue;
    const FixGrid fg = fixup_grid(a.g, lpr);
    const size_t fix_lds = fg.waves * (size_t)(a.rs.R + 2 * a.rs.H) * sizeof(float);
    if (fg.blocks == 0) continue;   // (an empty list)
    if (fg.listed) {
      PYGAT_DISPATCH_LANES(lpr, vec, hipLaunchKernelGGL((gat_bwd_col_fixup_list_kernel<LPR, VEC>), dim3(fg.blocks),
                                                        dim3(64 * fg.waves), fix_lds, st, a));
    } else {
      PYGAT_DISPATCH_LANES(lpr, vec, hipLaunchKernelGGL((gat_bwd_col_fixup_kernel<LPR, VEC>), dim3(fg.blocks),
                                                        dim3(64 * fg.waves), fix_lds, st, a));
    }
    PYGAT_CHECK_LAUNCH("gat_backward_col_fixup");
  }
  return PYGAT_OK;
}

extern "C" int pygat_gat_backward_col(const pygat_graph* gT, const int32_t* perm_t, int H, int Fo, float alpha,
                                      const float* Wh, const float* a_pad, const float* GR,
                                      const float* att_mask, const float* ds, float* dWh, float* dt, float* dz_t,
                                      void* part, float* da_part, int h_first, int h_count, int head_group, void* stream) {
  return backward_col(gT, perm_t, H, Fo, alpha, Wh, a_pad, GR, att_mask, ds, dWh, dt, dz_t, part, da_part, h_first, h_count, head_group,
                      0, stream);
}

extern "C" int pygat_gat_backward_col_phase(const pygat_graph* gT, const int32_t* perm_t, int H, int Fo, float alpha,
                                            const float* Wh, const float* a_pad, const float* GR,
                                            const float* att_mask, const float* ds, float* dWh, float* dt, float* dz_t,
                                            void* part, float* da_part, int h_first, int h_count, int head_group, int phase,
                                            void* stream) {
  return backward_col(gT, perm_t, H, Fo, alpha, Wh, a_pad, GR, att_mask, ds, dWh, dt, dz_t, part, da_part, h_first, h_count, head_group,
                      phase, stream);
}

// 1: the column pass of all H heads over gT runs in one head window with a list-driven fix-up -- its two launches may be
// asked for one by one (pygat_gat_backward_col_phase) and the fix-up may share a launch with the tail's stream
// (pygat_gat_backward_col_finish); 0: it does not; negative: a bad graph or shape
extern "C" int pygat_gat_backward_col_phases_ok(const pygat_graph* gT, int H, int Fo, int head_group) {
  GraphDev g;
  const int rc = check_graph(gT, &g, 2);
  if (rc) return rc;
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(H > 0 && Fp > 0, "gat_backward_col_phases_ok: unsupported H=%d F'=%d", H, Fo);
  RowShape rs;
  if (!g.cut || g.order || !make_window_shape(H, Fo, H, &rs)) return 0;
  return head_group_arg(head_group, g.n, H, Fp) >= H ? 1 : 0;
}

extern "C" int pygat_gat_backward_col_finish(const pygat_graph* gT, int H, int Fo, const float* a_pad, float* ds, float* dWh,
                                             float* dt, void* part, int head_group, int row_first, int n_rows, int flags,
                                             const float* G, const float* y, const int32_t* user_row, void* stream) {
  ColArgs a;
  int rc = check_graph(gT, &a.g, 2);
  if (rc) return rc;
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(H > 0 && Fp > 0, "gat_backward_col_finish: unsupported H=%d F'=%d", H, Fo);
  PYGAT_REQUIRE(pygat_gat_backward_col_phases_ok(gT, H, Fo, head_group) == 1,
                "gat_backward_col_finish: needs a cut-row list, no slot_order and the level in one head window "
                "(pygat_gat_backward_col_phases_ok)");
  PYGAT_REQUIRE(a_pad && ds && dWh && dt && part && G && y, "gat_backward_col_finish: null pointer");
  PYGAT_REQUIRE(row_first >= 0 && n_rows > 0 && (int64_t)row_first + n_rows <= a.g.n,
                "gat_backward_col_finish: tail rows [%d, +%d) outside the %d nodes", row_first, n_rows, a.g.n);
  PYGAT_REQUIRE(aligned16(dWh) && aligned16(a_pad) && aligned16(part) && (Fo != Fp || (aligned16(G) && aligned16(y))),
                "gat_backward_col_finish: row tables must be 16-byte aligned");
  PYGAT_REQUIRE(make_window_shape(H, Fo, H, &a.rs), "gat_backward_col_finish: unsupported H=%d F'=%d", H, Fo);
  a.alpha = 0.f; a.perm = nullptr; a.mask = nullptr; a.Wh = nullptr; a.GR = nullptr; a.ldgr = 0; a.dz_t = nullptr; a.da_part = nullptr;
  a.a_pad = a_pad; a.ds = ds; a.dWh = dWh; a.dt = dt; a.part = (float*)part;
  ColTailArgs t;
  t.row_first = row_first; t.n_rows = n_rows; t.Fo = Fo; t.flags = flags & PYGAT_F_ELU; t.G = G; t.y = y; t.urow = user_row; t.ds = ds;
  int lpr, vec;
  pick_lanes(a.rs, &lpr, &vec);
  const int fb = (int)fixup_grid(a.g, lpr).blocks;   // (listed: pygat_gat_backward_col_phases_ok)
  const int64_t tb = cdiv((int64_t)n_rows * (a.rs.R / 4), 64 * FIX_LIST_WAVES);
  PYGAT_REQUIRE(fb + tb < ((int64_t)1 << 31), "gat_backward_col_finish: grid too large");
  const size_t fix_lds = FIX_LIST_WAVES * (size_t)(a.rs.R + 2 * a.rs.H) * sizeof(float);
  PYGAT_DISPATCH_LANES(lpr, vec, hipLaunchKernelGGL((gat_bwd_col_finish_kernel<LPR, VEC>), dim3((unsigned)(fb + tb)),
                                                    dim3(64 * FIX_LIST_WAVES), fix_lds, (hipStream_t)stream, a, t, fb));
  PYGAT_CHECK_LAUNCH("gat_backward_col_finish");
  return PYGAT_OK;
}
