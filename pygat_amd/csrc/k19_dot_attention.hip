// K19 -- dot_attention: softmax-weighted sums of value rows over the entries of every row of a sparse pattern, for H heads at once, in
// one pass, and the row side of its gradient.  One kernel family: four kernels (forward | backward) x (long | row), instantiated per
// lane shape and per variant, a set of compile-time flags (DA_BIAS, DA_DROP, DA_EDGE, DA_BF16).
//
// Arithmetic.  For an entry e = (i, j) of row i, c(e) its index in the CALLER's order (perm), per head h:
//   kk = k[j, h],  vv = v[j, h];                       EDGE: kk = k[j, h] + e[c, h], vv = v[j, h] + e[c, h], one rounded add per element,
//                                                      formed the same way in both passes
//   s = scale <q[i, h], kk>                            one rounding of the product, the same bits in both passes;  BIAS: the softmax runs
//                                                      over s + bias[c, h] (bias [nnz x H], or [nnz] with a head stride of 0), taken as
//                                                      s - (m - b): the bias goes to the maximum's side, so b = 0 is the plain expression
//   p = exp(s - m[i, h]) / Z[i, h]                     m, Z [n_rows x H]: the row's maximum and sum of exp(s - m), of the biased scores
//                                                      under BIAS and always of the undropped softmax
//   out[i, h] = sum_e p vv                             DROP: sum_e p mask[c, h] vv, mask in {0, 1 / (1 - p)}: a dropped entry stays in Z
//   backward_rows:  D = <G[i, h], out[i, h]>,  dp = <G[i, h], vv>  (DROP: mask dp),  ds = scale p (dp - D),  dq[i, h] = sum_e ds kk,
//     P[c, h] = p (DROP: p mask) and S[c, h] = ds for the column side: dk = spmm^T(S, q) and dv = spmm^T(P, G) are two
//     pygat_spmm_forward launches on the transposed pattern (K17);  BIAS: T = p (dp - D), the gradient of the bias, stored at [c, h]
//     where it is asked for (ds stays the expression without a bias);  EDGE: de[c] = ds q[i] + p G[i], a 16-byte store per lane and
//     entry where it is asked for -- an entry belongs to one row (in a long row to one piece), so every row of de is written exactly
//     once and nothing is zeroed.
//   The forward keeps out, m and Z, all the backward reads -- nothing per entry.  DROP draws its mask in registers in both passes, no
//   mask tensor exists: mask[c, h] is element c H + h of the flat layout of k7_dropout.hip's mask kernel (rng.h): word (idx & 3) of
//   Philox-4x32-10(counter = (idx >> 2 low, idx >> 2 high, stream_id, 0xFFFFFFFF), key = *seed) < thresh keeps, so
//   pygat_dropout_mask(nnz H, p, seed, stream_id) writes the same table.  The LH lanes of a head share a batch's draws (da_keep_batch).
//   BF16 (forward only, inference): k and v are rows of H*F bf16 values, a lane's chunk one 8-byte load widened in registers (a bf16
//   is the high half of an fp32); everything after the load sees the fp32 kernels' values in their order.  Neither m nor Z is written.
//   EDGE goes with neither DROP nor BF16, DROP not with BF16; BIAS goes with each.
//
// Lane mapping.  Rows are H*F floats, heads side by side, NOT padded; F a power of two in 4..256.  As K17's CW = 4 path: a group of
// LPR lanes holds one row, VEC chunks of 4 floats (16-byte loads) per lane, chunk c = c0 + 64 v.  F / 4 is a power of two, so the
// chunks of a head sit on LH = F / 4 adjacent lanes of one v, and a head's dot product is a butterfly over them; every lane of a head
// ends with the same s, m and Z.  q_i is loaded once per row.  Per entry k_j and v_j (and the e row) are gathered, several entries in
// flight (da_unroll), the indices and bias values of the next batch asked for under this batch's arithmetic (DaFam::walk), and folded
// into an online (m, Z, acc) state per head with one __expf per (entry, head) (da_fold; K18's es_fold).
//
// Long rows go through partial records (the rule of long_rows.h), one wave per chunk: its lane groups walk the piece
// entry-interleaved and are merged maximum first -- rescale once, then a fixed butterfly -- and records merge in chunk order by the
// same rule.  A record is (acc[H F], m[H], Z[H]) forward and the dq row backward, whatever the variant.
//
// Exactness.  No LDS, no float atomics, every sum in a fixed order: two runs give the same bits.
//   a row without entries   out = m = Z = dq = 0 exactly
//   a row of one entry      out_i = v_j bit for bit, p = 1 and ds = dq_i = 0;  BIAS: the same, T = 0, p = 1 to rounding;  DROP: out_i =
//                           mask v_j bit for bit;  EDGE: out_i = v_j + e_c and de_c = G_i bit for bit
//   a bias of zeros         changes no bit of out, dq, P or S; a large negative finite bias (-9e15) gives p = 0 exactly while the row
//                           keeps another entry
//   e = 0                   leaves out, dq, P and S at the values of the kernels without EDGE
//   all entries dropped     (and every row under p = 1) exact zeros
//   bf16 tables             the result of the fp32 kernels on the widened tables bit for bit
// A flag that is off leaves no trace in a kernel: the instantiations without it are instruction for instruction what they would be
// if the flag did not exist (profiles/k19_refactor_isa.txt).
// The kernel arguments, the lane mapping, the fold of one head, the record merge and the lane-shape dispatch are da_lanes.h's; the
// four kernels themselves, the shape check, the kernel-name parser and the launch of a pair are da_family.h's, instantiated on DaFam
// below.  Both are shared with K20 (k20_additive_attention.hip) and K21 (k21_gatv2_attention.hip).
#include "da_family.h"
#include <type_traits>

namespace pygat {

// a variant: the set of its flags, the template parameter V of everything below that depends on one
enum : unsigned { DA_BIAS = 1, DA_DROP = 2, DA_EDGE = 4, DA_BF16 = 8 };
constexpr bool da_has(unsigned v, unsigned flag) { return (v & flag) != 0; }
// the caller's entry index c(e) travels with the walk
constexpr bool da_eid_walk(unsigned v) { return da_has(v, DA_BIAS | DA_DROP | DA_EDGE); }
// the kernels that exist: bf16 tables are for inference (no dropout, no backward), per-entry rows go with fp32 tables and no dropout
constexpr bool da_exists(unsigned v, bool bwd) {
  return v < 16 && !(da_has(v, DA_EDGE) && da_has(v, DA_DROP | DA_BF16)) && !(da_has(v, DA_BF16) && (bwd || da_has(v, DA_DROP)));
}

// (a bf16 table, da_bf16, and its 8-byte da_load_row: da_lanes.h, shared with K20 and K21)

// the score of one entry: one rounding of the product, so the forward and the backward see the same bits
template <int LPR>
__device__ __forceinline__ float da_score(const DaArgs& g, const float4& q, const float4& k) {
  return __fmul_rn(g.scale, da_head_sum<LPR>(dot4(q, k), g.LH));
}

// (DROP: the key of the row's draws, da_key, and the keep factors of a batch, da_keep_batch: da_lanes.h, shared with K20 and K21)

// ----------------------------------------------------------------------------------------------------------- the fold and the walk
// (the fold of one head, da_fold, and the merge of two records, da_merge: da_lanes.h)
// U gathered entries: the k and v rows of columns src[0..U), loaded before any is used
template <int VEC, int U>
struct DaRows {
  float4 k[U][VEC], v[U][VEC];
};
// T: the element type of the k and v tables (float, or da_bf16 in the inference forward: g.k and g.v then point at bf16 rows, ldk and
// ldv counting elements all the same)
template <int VEC, int U, typename T = float>
__device__ __forceinline__ void da_gather(const DaArgs& g, const DaLane<VEC>& ln, const int32_t (&src)[U], DaRows<VEC, U>& w) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    da_load_row<VEC>(reinterpret_cast<const T*>(g.k) + (int64_t)src[u] * g.ldk, ln, w.k[u]);
    da_load_row<VEC>(reinterpret_cast<const T*>(g.v) + (int64_t)src[u] * g.ldv, ln, w.v[u]);
  }
}

// EDGE: the e rows of U entries at the caller's entry indices eid[0..U), asked for right behind the gather of their batch, and
// kk = k_j + e, vv = v_j + e in the gathered rows' place: one rounded add per element, the same in the forward and the backward
template <int VEC, int U, bool EDGE>
struct DaEdgeRows {
  float4 e[EDGE ? U : 1][EDGE ? VEC : 1];
};
template <int VEC, int U>
__device__ __forceinline__ void da_gather_edge(const DaArgs& g, const DaLane<VEC>& ln, const int32_t (&eid)[U],
                                               DaEdgeRows<VEC, U, true>& we) {
#pragma unroll
  for (int u = 0; u < U; ++u) da_load_row<VEC>(g.e + (int64_t)eid[u] * g.lde, ln, we.e[u]);
}
__device__ __forceinline__ void da_add_rn(float4& y, const float4& x) {
  y.x = __fadd_rn(y.x, x.x); y.y = __fadd_rn(y.y, x.y); y.z = __fadd_rn(y.z, x.z); y.w = __fadd_rn(y.w, x.w);
}
template <int VEC, int U>
__device__ __forceinline__ void da_edge_add(DaRows<VEC, U>& w, const DaEdgeRows<VEC, U, true>& we) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) { da_add_rn(w.k[u][v], we.e[u][v]); da_add_rn(w.v[u][v], we.e[u][v]); }
}

// ------------------------------------------------------------------------------------------------------------------------ forward
// the forward's fold of a batch; ctx: q_i and the row's state.  eid is looked at under DROP alone, ent and lone not at all
template <int LPR, int VEC, unsigned V>
struct DaFwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, const DaLane<VEC>& ln, uint2 key, const float4 (&q)[VEC],
                                              DaState<VEC>& st, const DaRows<VEC, U>& w, const int64_t (&)[U],
                                              const DaBias<VEC, U, da_has(V, DA_BIAS)>& bs, const int32_t (&eid)[U], bool) {
    constexpr bool BIAS = da_has(V, DA_BIAS), DROP = da_has(V, DA_DROP);
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) {
      int64_t base[U];
#pragma unroll
      for (int u = 0; u < U; ++u) base[u] = (int64_t)eid[u] * g.H;
      da_keep_batch<VEC, U>(g, ln, key, base, keep);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        da_fold<BIAS, DROP>(st.m[v], st.z[v], st.acc[v], da_score<LPR>(g, q[v], w.k[u][v]), BIAS ? bs.b[u][v] : 0.f,
                            DROP ? keep[u][v] : 1.f, w.v[u][v]);
  }
};

// ------------------------------------------------------------------------------------------------------------- backward, row side
template <int VEC>
struct DaRow : DaGrad<VEC> {   // what the backward holds of its row
  float4 q[VEC];
};

// the backward's fold of a batch; ctx: the row (DaRow) and its dq
// BIAS: T = p (<G_i, v_j> - D_i), the gradient of the bias, formed beside ds -- ds itself is the unbiased kernel's expression, so a
// bias of zeros leaves the bits of S, dq and dk alone -- and stored where it is asked for
// DROP: the batch's keep factors are drawn again (ent[u] + head is an entry's flat mask index); an entry's multiplies <G_i, v_j> --
// D_i = <G_i, out_i> is the row term of the dropped sum already -- and the stored P is p keep, what the transposed SpMM of dv
// multiplies G with
// EDGE: w holds kk and vv; every lane also stores its chunk of de[c(e)] = ds q_i + p G_i where de is asked for (eid: the batch's
// entry indices, looked at under EDGE alone).  lone (EDGE alone): the entry is the only one of its row, whose coefficient is 1 by
// definition and goes into de as that, so de_c = G_i bit for bit: the p formed here is exp(scale <q, kk> - m) with the product
// contracted into the difference, m the rounded product, and may come out an ulp above 1 where the scale is no power of two
template <int LPR, int VEC, unsigned V>
struct DaBwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, const DaLane<VEC>& ln, uint2 key, const DaRow<VEC>& r,
                                              float4 (&dq)[VEC], const DaRows<VEC, U>& w, const int64_t (&ent)[U],
                                              const DaBias<VEC, U, da_has(V, DA_BIAS)>& bs, [[maybe_unused]] const int32_t (&eid)[U],
                                              [[maybe_unused]] bool lone) {
    constexpr bool BIAS = da_has(V, DA_BIAS), DROP = da_has(V, DA_DROP), EDGE = da_has(V, DA_EDGE);
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) da_keep_batch<VEC, U>(g, ln, key, ent, keep);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float s = da_score<LPR>(g, r.q[v], w.k[u][v]);
        float p;
        if constexpr (BIAS) p = __expf(s - (r.m[v] - bs.b[u][v])) * r.rz[v];      // (as da_fold: s - m with the bias on m's side)
        else p = __expf(s - r.m[v]) * r.rz[v];
        float dp = da_head_sum<LPR>(dot4(r.G[v], w.v[u][v]), g.LH);
        float pk = p;
        if constexpr (DROP) {
          dp *= keep[u][v];
          pk *= keep[u][v];
        }
        const float ds = g.scale * p * (dp - r.D[v]);
        da_axpy(dq[v], ds, w.k[u][v]);
        if (ln.lead >> v & 1) {
          g.P[ent[u] + ln.head[v]] = pk;
          g.S[ent[u] + ln.head[v]] = ds;
          if constexpr (BIAS)
            if (g.dbias) g.dbias[ent[u] + ln.head[v]] = p * (dp - r.D[v]);
        }
        if constexpr (EDGE)
          if (g.de && (ln.ok >> v & 1)) {
            const float4 &qi = r.q[v], &Gi = r.G[v];
            const float pe = lone ? 1.f : p;
            st4(g.de + (int64_t)eid[u] * g.ldde + ln.ofs[v],
                make_float4(fmaf(ds, qi.x, pe * Gi.x), fmaf(ds, qi.y, pe * Gi.y), fmaf(ds, qi.z, pe * Gi.z), fmaf(ds, qi.w, pe * Gi.w)));
          }
      }
  }
};

// the family: what the kernels of da_family.h hold of a row and how they walk it, per variant.  m and Z are what a backward reads: the
// bf16-table kernels, which have none, do not write them.  lone: see walk
template <unsigned V>
struct DaFam {
  static constexpr bool KEEP_MZ = !da_has(V, DA_BF16);
  template <int VEC> using Own = float4[VEC];                  // q_i
  template <int VEC> using Row = DaRow<VEC>;
  __device__ __forceinline__ static uint2 key(const DaArgs& g) { return da_key<da_has(V, DA_DROP)>(g); }
  __device__ __forceinline__ static bool lone(int64_t start, int64_t end) { return da_has(V, DA_EDGE) && end - start == 1; }
  template <int VEC>
  __device__ __forceinline__ static void load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, float4 (&q)[VEC]) {
    da_load_row<VEC>(g.q + row * g.ldq, ln, q);
  }
  template <int LPR, int VEC>
  __device__ __forceinline__ static void bwd_load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, DaRow<VEC>& r) {
    load<VEC>(g, ln, row, r.q);
    da_grad_load<LPR, VEC>(g, ln, row, r);
  }
  // The walk of both passes (PASS 0 forward, 1 backward): the entries e0, e0 + step, ... < e1 of one row, handed to Fold::fold in that
  // order, U at a time and then one at a time.  w: the gathered k and v rows (kk and vv under EDGE); bs: the bias values; eid: the
  // caller's entry indices (where the variant carries them, da_eid_walk); ent: eid x H (BWD); key (DROP): the key of the row's draws;
  // ctx: what the pass keeps of its row, handed through; U = da_unroll.  Fold is DaFwdFold or DaBwdFold, a type and not a closure, key
  // travels by value, and the kernels of da_family.h call this member themselves: a closure, a key behind a reference or one more
  // function between a kernel and its walk all gave the same instructions in another order.
  // The order of the loads is the kernels' speed.  The column indices of the next U entries are asked for before this batch's rows are
  // used, so an iteration waits for one gather, not for an index and then a gather.  Where the variant carries entry indices, the next
  // batch's travel with its column indices as loaded words (da_eid_raw) and become indices only after this batch's fold; BIAS: the
  // next batch's bias values are asked for then, ahead of the next gather, so they are there when it is -- an iteration still waits for
  // one gather.  EDGE: the same entry indices place the batch's e rows, asked for right behind its gather, and its rows of de.
  // The backward without a flag needs the entry index only for its stores and forms it whole (da_entry) a batch ahead.
  // One at a time, the backward forms what it needs where it needs it: ent by da_entry, eid ahead of the bias load (BIAS) and again
  // behind the gather (EDGE); one index for all of them is fewer instructions, and changes those of every flagged backward kernel.
  // lone (the backward row kernel under EDGE says so; a piece of a long row never is): the walk is over a row of one entry
  template <int LPR, int VEC, int PASS, typename... Ctx>
  __device__ __forceinline__ static void walk(const DaArgs& g, const DaLane<VEC>& ln, int64_t e0, int64_t e1, int64_t step, bool lone,
                                              uint2 key, Ctx&... ctx) {
    constexpr bool BWD = PASS == 1;
    static_assert(da_exists(V, BWD), "bf16 tables are for inference: no dropout, no backward; per-entry rows: fp32 tables, no dropout");
    using Fold = std::conditional_t<BWD, DaBwdFold<LPR, VEC, V>, DaFwdFold<LPR, VEC, V>>;
    constexpr int U = da_unroll(BWD, VEC);
    constexpr bool BIAS = da_has(V, DA_BIAS), EDGE = da_has(V, DA_EDGE), EID = da_eid_walk(V);
    using T = std::conditional_t<da_has(V, DA_BF16), da_bf16, float>;      // the element type of the k and v tables
    int64_t e = e0;
    if constexpr (U > 1) {
      int32_t src[U];
      [[maybe_unused]] int64_t ent[U], ent_next[U];
      [[maybe_unused]] int32_t raw[U], eid[U];
      DaBias<VEC, U, BIAS> bs;
      bool full = e + (U - 1) * step < e1;
      if (full) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          src[u] = g.col[e + u * step];
          if constexpr (EID) raw[u] = da_eid_raw(g, e + u * step);
          else if constexpr (BWD) ent_next[u] = da_entry(g, e + u * step);
        }
        if constexpr (EID) da_eids<U>(g, raw, e, step, eid);
        if constexpr (BIAS) da_bias_load<VEC, U>(g, ln, eid, bs);
      }
      while (full) {
        DaRows<VEC, U> w;
        da_gather<VEC, U, T>(g, ln, src, w);
        [[maybe_unused]] DaEdgeRows<VEC, U, EDGE> we;
        if constexpr (EDGE) da_gather_edge<VEC, U>(g, ln, eid, we);
        if constexpr (BWD && !EID) {
#pragma unroll
          for (int u = 0; u < U; ++u) ent[u] = ent_next[u];
        }
        e += U * step;
        full = e + (U - 1) * step < e1;
        if (full) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            src[u] = g.col[e + u * step];
            if constexpr (EID) raw[u] = da_eid_raw(g, e + u * step);
            else if constexpr (BWD) ent_next[u] = da_entry(g, e + u * step);
          }
        }
        if constexpr (BWD && EID) {                                  // (eid: this batch's, formed after the last fold, not yet replaced)
#pragma unroll
          for (int u = 0; u < U; ++u) ent[u] = (int64_t)eid[u] * g.H;
        }
        if constexpr (EDGE) da_edge_add<VEC, U>(w, we);
        Fold::fold(g, ln, key, ctx..., w, ent, bs, eid, false);
        if constexpr (EID)
          if (full) {
            da_eids<U>(g, raw, e, step, eid);
            if constexpr (BIAS) da_bias_load<VEC, U>(g, ln, eid, bs);
          }
      }
    }
    for (; e < e1; e += step) {
      const int32_t src[1] = {g.col[e]};
      [[maybe_unused]] int64_t ent[1] = {0};
      [[maybe_unused]] int32_t eid[1] = {0};
      if constexpr (BWD) ent[0] = da_entry(g, e);
      if constexpr (BWD ? BIAS : EID) eid[0] = da_eid(g, da_eid_raw(g, e), e);
      DaBias<VEC, 1, BIAS> bs;
      if constexpr (BIAS) da_bias_load<VEC, 1>(g, ln, eid, bs);
      DaRows<VEC, 1> w;
      da_gather<VEC, 1, T>(g, ln, src, w);
      if constexpr (EDGE) {
        if constexpr (BWD) eid[0] = da_eid(g, da_eid_raw(g, e), e);
        DaEdgeRows<VEC, 1, true> we;
        da_gather_edge<VEC, 1>(g, ln, eid, we);
        da_edge_add<VEC, 1>(w, we);
      }
      Fold::fold(g, ln, key, ctx..., w, ent, bs, eid, lone);
    }
  }
};

// the table of the family (lane shapes: da_pick and PYGAT_DA_DISPATCH of da_lanes.h): (variant, forward | backward, long | row, lane
// shape) -> the kernel of da_family.h on DaFam<variant>; null where there is none.  What a launcher starts and what
// pygat_kernel_footprint reports on both come from here
template <int LPR, int VEC, unsigned V>
static const void* da_kernel_at(bool bwd, bool lng) {
  if constexpr (da_exists(V, true)) {
    if (bwd) return lng ? reinterpret_cast<const void*>(&da_bwd_long_kernel<DaFam<V>, LPR, VEC>)
                        : reinterpret_cast<const void*>(&da_bwd_row_kernel<DaFam<V>, LPR, VEC>);
  } else if (bwd) return nullptr;
  return lng ? reinterpret_cast<const void*>(&da_fwd_long_kernel<DaFam<V>, LPR, VEC>)
             : reinterpret_cast<const void*>(&da_fwd_row_kernel<DaFam<V>, LPR, VEC>);
}
template <unsigned V>
static const void* da_kernel_of(bool bwd, bool lng, int lpr, int vec) {
  PYGAT_DA_DISPATCH(lpr, vec, return (da_kernel_at<LPR, VEC, V>(bwd, lng)));
  return nullptr;
}
static const void* da_kernel(unsigned variant, bool bwd, bool lng, int lpr, int vec) {
  switch (variant) {
    case 0: return da_kernel_of<0>(bwd, lng, lpr, vec);
    case DA_BIAS: return da_kernel_of<DA_BIAS>(bwd, lng, lpr, vec);
    case DA_BF16: return da_kernel_of<DA_BF16>(bwd, lng, lpr, vec);
    case DA_BF16 | DA_BIAS: return da_kernel_of<DA_BF16 | DA_BIAS>(bwd, lng, lpr, vec);
    case DA_DROP: return da_kernel_of<DA_DROP>(bwd, lng, lpr, vec);
    case DA_DROP | DA_BIAS: return da_kernel_of<DA_DROP | DA_BIAS>(bwd, lng, lpr, vec);
    case DA_EDGE: return da_kernel_of<DA_EDGE>(bwd, lng, lpr, vec);
    case DA_EDGE | DA_BIAS: return da_kernel_of<DA_EDGE | DA_BIAS>(bwd, lng, lpr, vec);
  }
  return nullptr;
}

// pygat_kernel_footprint: <prefix>{fwd,bwd}_{long,row}_l<LPR>v<VEC> (the lane shapes of PYGAT_DA_DISPATCH); the prefix names the
// variant: k19_, k19b_ (BIAS), k19h_, k19hb_ (bf16 tables: fwd only), k19d_, k19db_ (DROP), k19e_, k19eb_ (EDGE)
int footprint_k19(const char* name, int* regs, int* scratch) {
  static const struct { const char* prefix; unsigned variant; } names[] = {
      {"k19_", 0}, {"k19b_", DA_BIAS}, {"k19h_", DA_BF16}, {"k19hb_", DA_BF16 | DA_BIAS},
      {"k19d_", DA_DROP}, {"k19db_", DA_DROP | DA_BIAS}, {"k19e_", DA_EDGE}, {"k19eb_", DA_EDGE | DA_BIAS}};
  const void* fn = nullptr;
  DaKernelName k;
  for (const auto& nm : names)
    if (da_parse_kernel_name(name, nm.prefix, &k) && k.pass <= 1) fn = da_kernel(nm.variant, k.pass == 1, k.lng, k.lpr, k.vec);
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k19{,b,h,hb,d,db,e,eb}_{fwd,bwd}_{long,row}_l<LPR>v<VEC>; k19h*: fwd only)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

#define DA_PAD_HINT "zero-padding the columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged"

// kv_bytes: the size of an element of k and v (4, or 2: bf16 tables); keep_mz: the launcher writes or reads m and Z
static int da_check_common(const char* what, int n_rows, int64_t nnz, int H, int F, const int32_t* rowptr, const int32_t* col,
                           const float* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv, const float* out,
                           int64_t ldo, const float* m, const float* Z, const void* ws, int kv_bytes = 4, bool keep_mz = true) {
  const int rc = da_check_shape(what, nnz, H, F, DA_PAD_HINT);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(n_rows >= 0, "%s: n_rows=%d", what, n_rows);
  PYGAT_REQUIRE(n_rows > 0 || nnz == 0, "%s: n_rows=0 with nnz=%lld entries", what, (long long)nnz);
  const int HF = H * F;
  PYGAT_REQUIRE(rowptr, "%s: null rowptr", what);
  PYGAT_REQUIRE(nnz == 0 || col, "%s: null col", what);
  DA_TABLE(what, "q", q, ldq, HF);
  DA_TABLE_ALIGNED(what, "k", k, ldk, HF, 4 * kv_bytes);
  DA_TABLE_ALIGNED(what, "v", v, ldv, HF, 4 * kv_bytes);
  DA_TABLE(what, "out", out, ldo, HF);
  PYGAT_REQUIRE(m || !keep_mz, "%s: null m", what);
  PYGAT_REQUIRE(Z || !keep_mz, "%s: null Z", what);
  PYGAT_REQUIRE(ws, "%s: null workspace", what);
  PYGAT_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_dot_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "dot_attn_workspace_bytes: null bytes");
  const int rc = da_check_shape("dot_attn_workspace_bytes", nnz, H, F, DA_PAD_HINT);
  if (rc != PYGAT_OK) return rc;
  *bytes = (size_t)da_part_floats(nnz, H, F) * sizeof(float);
  return PYGAT_OK;
}

// the per-entry term of the BIAS launchers: non-null where there are entries (4-byte loads: no alignment asked for), a head stride of 1
// ([nnz x H]) or 0 ([nnz], shared by the heads)
static int da_check_bias(const char* what, int64_t nnz, const float* bias, int bias_head_stride) {
  PYGAT_REQUIRE(nnz == 0 || bias, "%s: null bias", what);
  PYGAT_REQUIRE(bias_head_stride == 0 || bias_head_stride == 1, "%s: bias_head_stride=%d, 1 (bias [nnz x H]) or 0 (bias [nnz], shared by "
                "the heads) expected", what, bias_head_stride);
  return PYGAT_OK;
}

// (the mask of the DROP launchers, DaDrop and da_check_drop: da_family.h, shared with K20 and K21)

// (the per-entry rows of the EDGE launchers, DaEdge and da_check_edge: da_family.h, shared with K21)

// what an entry point asks for: its name, the variant and the pass, and every argument under the name include/pygat_amd.h gives it.
// k and v are float or bf16 rows by the variant; out, m and Z are written by the forward and read by the backward; what a variant or a
// pass does not have stays zero
struct DaCall {
  const char* what;
  unsigned variant;
  bool bwd;
  int n_rows;
  int64_t nnz;
  const int32_t *rowptr, *col, *perm;
  int H, F;
  float scale;
  const float* q;
  int64_t ldq;
  const void *k, *v;
  int64_t ldk, ldv;
  float* out;
  int64_t ldo;
  float *m, *Z;
  void *ws, *stream;
  const float* bias;           // DA_BIAS
  int bias_head_stride;
  float* dbias;                // ... backward; null: not asked for
  DaDrop drop;                 // DA_DROP
  DaEdge edge;                 // DA_EDGE
  const float* G;              // backward only from here
  int64_t ldg;
  float* dq;
  int64_t lddq;
  float *P, *S;
};
// the arguments all nine entry points have, from the entry point's own parameters
#define DA_CALL(c, name, var, back)                                                                                                 \
  DaCall c = {};                                                                                                                    \
  c.what = name; c.variant = var; c.bwd = back; c.n_rows = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.H = H; c.F = F;  \
  c.scale = scale; c.q = q; c.ldq = ldq; c.k = k; c.ldk = ldk; c.v = v; c.ldv = ldv; c.out = const_cast<float*>(out); c.ldo = ldo; \
  c.ws = ws; c.stream = stream
// ... and those of the backward's
#define DA_CALL_BWD(c) \
  c.perm = perm; c.m = const_cast<float*>(m); c.Z = const_cast<float*>(Z); c.G = G; c.ldg = ldg; c.dq = dq; c.lddq = lddq; c.P = P; c.S = S
// a null bias at an entry point that takes one or none: the variant without BIAS; bias_head_stride is then not looked at
static inline unsigned da_with_bias(unsigned variant, const float* bias) { return bias ? variant | DA_BIAS : variant; }

// every launcher: the checks, in one order; the kernel arguments; the piece kernel where there are long rows, then the row kernel
static int da_launch(const DaCall& c) {
  const char* what = c.what;
  const bool bias = da_has(c.variant, DA_BIAS), drop = da_has(c.variant, DA_DROP), edge = da_has(c.variant, DA_EDGE),
             bf16 = da_has(c.variant, DA_BF16);
  const int HF = c.H * c.F;
  int rc = da_check_common(what, c.n_rows, c.nnz, c.H, c.F, c.rowptr, c.col, c.q, c.ldq, c.k, c.ldk, c.v, c.ldv, c.out, c.ldo, c.m, c.Z,
                           c.ws, bf16 ? 2 : 4, !bf16);
  if (rc != PYGAT_OK) return rc;
  if (c.bwd) {
    DA_TABLE(what, "G", c.G, c.ldg, HF);
    DA_TABLE(what, "dq", c.dq, c.lddq, HF);
    PYGAT_REQUIRE(c.nnz == 0 || c.P, "%s: null P", what);
    PYGAT_REQUIRE(c.nnz == 0 || c.S, "%s: null S", what);
  }
  if (edge && (rc = da_check_edge(what, c.nnz, HF, c.edge)) != PYGAT_OK) return rc;
  if (bias && (rc = da_check_bias(what, c.nnz, c.bias, c.bias_head_stride)) != PYGAT_OK) return rc;
  DropRng rng;
  if (drop && (rc = da_check_drop(what, c.drop, &rng)) != PYGAT_OK) return rc;
  if (c.n_rows == 0) return PYGAT_OK;
  DaArgs g;
  memset(&g, 0, sizeof(g));
  g.n = c.n_rows; g.H = c.H; g.F = c.F; g.NCH = HF / 4; g.LH = c.F / 4; g.nnz = c.nnz; g.rowptr = c.rowptr; g.col = c.col; g.scale = c.scale;
  g.q = c.q; g.ldq = c.ldq; g.k = static_cast<const float*>(c.k); g.ldk = c.ldk; g.v = static_cast<const float*>(c.v); g.ldv = c.ldv;
  g.out = c.out; g.ldo = c.ldo; g.m = c.m; g.Z = c.Z; g.part = static_cast<float*>(c.ws); g.pstride = da_pstride(c.H, c.F);
  if (c.bwd || da_eid_walk(c.variant)) g.perm = c.perm;           // (the forward without a flag walks in CSR order alone)
  if (c.bwd) { g.G = c.G; g.ldg = c.ldg; g.dq = c.dq; g.lddq = c.lddq; g.P = c.P; g.S = c.S; }
  if (bias) { g.bias = c.bias; g.bhs = c.bias_head_stride; g.bstride = c.bias_head_stride ? c.H : 1; g.dbias = c.dbias; }
  if (drop) g.rng = rng;
  if (edge) { g.e = c.edge.e; g.lde = c.edge.lde; g.de = c.edge.de; g.ldde = c.edge.ldde; }
  const DaGrid gd = da_grid(c.n_rows, c.nnz, c.H, c.F);
  da_launch_pair(da_kernel(c.variant, c.bwd, true, gd.lpr, gd.vec), da_kernel(c.variant, c.bwd, false, gd.lpr, gd.vec), g, gd.chunks,
                 gd.blocks, c.stream);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

extern "C" int pygat_dot_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F, float scale,
                                           const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv,
                                           float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_forward", 0, false);
  c.m = m; c.Z = Z;
  return da_launch(c);
}

extern "C" int pygat_dot_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                                 int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                 const float* v, int64_t ldv, const float* out, int64_t ldo, const float* m,
                                                 const float* Z, const float* G, int64_t ldg, float* dq, int64_t lddq, float* P,
                                                 float* S, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_backward_rows", 0, true);
  DA_CALL_BWD(c);
  return da_launch(c);
}

// the same two with a per-entry term on the score: s[e, h] = scale <q_i, k_j> + bias[entry(e), h bias_head_stride]
extern "C" int pygat_dot_attn_bias_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                                int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                                const float* v, int64_t ldv, const float* bias, int bias_head_stride, float* out,
                                                int64_t ldo, float* m, float* Z, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_bias_forward", DA_BIAS, false);
  c.perm = perm; c.m = m; c.Z = Z; c.bias = bias; c.bias_head_stride = bias_head_stride;
  return da_launch(c);
}

// the inference forward on bf16 k and v tables (8-byte aligned rows, strides in elements); a null bias: the kernels without BIAS
extern "C" int pygat_dot_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                                int H, int F, float scale, const float* q, int64_t ldq, const void* k, int64_t ldk,
                                                const void* v, int64_t ldv, const float* bias, int bias_head_stride, float* out,
                                                int64_t ldo, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_bf16_forward", da_with_bias(DA_BF16, bias), false);
  c.perm = perm; c.bias = bias; c.bias_head_stride = bias_head_stride;
  return da_launch(c);
}

extern "C" int pygat_dot_attn_bias_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                                      const int32_t* perm, int H, int F, float scale, const float* q, int64_t ldq,
                                                      const float* k, int64_t ldk, const float* v, int64_t ldv, const float* bias,
                                                      int bias_head_stride, const float* out, int64_t ldo, const float* m,
                                                      const float* Z, const float* G, int64_t ldg, float* dq, int64_t lddq, float* P,
                                                      float* S, float* dbias, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_bias_backward_rows", DA_BIAS, true);
  DA_CALL_BWD(c);
  c.bias = bias; c.bias_head_stride = bias_head_stride; c.dbias = dbias;
  return da_launch(c);
}

// the bias pair with seeded dropout of the coefficients (the DROP instantiations): out = sum_e alpha mask v, mask[c(e), h] element
// c(e) H + h of the flat layout pygat_dropout_mask(nnz H, p, seed, stream_id) writes, drawn in registers in both passes.  A null bias: no
// bias, bias_head_stride is then not looked at
extern "C" int pygat_dot_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                              int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                              const float* v, int64_t ldv, const float* bias, int bias_head_stride, float p,
                                              const void* seed, uint32_t stream_id, float* out, int64_t ldo, float* m, float* Z,
                                              void* ws, void* stream) {
  DA_CALL(c, "dot_attn_dropout_forward", da_with_bias(DA_DROP, bias), false);
  c.perm = perm; c.m = m; c.Z = Z; c.bias = bias; c.bias_head_stride = bias_head_stride; c.drop = {p, seed, stream_id};
  return da_launch(c);
}

extern "C" int pygat_dot_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                                    const int32_t* perm, int H, int F, float scale, const float* q, int64_t ldq,
                                                    const float* k, int64_t ldk, const float* v, int64_t ldv, const float* bias,
                                                    int bias_head_stride, float p, const void* seed, uint32_t stream_id,
                                                    const float* out, int64_t ldo, const float* m, const float* Z, const float* G,
                                                    int64_t ldg, float* dq, int64_t lddq, float* P, float* S, float* dbias, void* ws,
                                                    void* stream) {
  DA_CALL(c, "dot_attn_dropout_backward_rows", da_with_bias(DA_DROP, bias), true);
  DA_CALL_BWD(c);
  c.bias = bias; c.bias_head_stride = bias_head_stride; c.dbias = dbias; c.drop = {p, seed, stream_id};
  return da_launch(c);
}

// the bias pair with a row of H*F floats per entry on both sides (the EDGE instantiations): s = scale <q_i, k_j + e_c> + bias,
// out_i = sum alpha (v_j + e_c), c the caller's entry index; backward_rows also forms de[c] = ds q_i + p G_i where de is not null.
// A null bias: no bias, bias_head_stride is then not looked at
extern "C" int pygat_dot_attn_edge_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                           int H, int F, float scale, const float* q, int64_t ldq, const float* k, int64_t ldk,
                                           const float* v, int64_t ldv, const float* e, int64_t lde, const float* bias,
                                           int bias_head_stride, float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_edge_forward", da_with_bias(DA_EDGE, bias), false);
  c.perm = perm; c.m = m; c.Z = Z; c.bias = bias; c.bias_head_stride = bias_head_stride; c.edge = {e, lde, nullptr, 0};
  return da_launch(c);
}

extern "C" int pygat_dot_attn_edge_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                                 const int32_t* perm, int H, int F, float scale, const float* q, int64_t ldq,
                                                 const float* k, int64_t ldk, const float* v, int64_t ldv, const float* e, int64_t lde,
                                                 const float* bias, int bias_head_stride, const float* out, int64_t ldo,
                                                 const float* m, const float* Z, const float* G, int64_t ldg, float* dq, int64_t lddq,
                                                 float* P, float* S, float* de, int64_t ldde, float* dbias, void* ws, void* stream) {
  DA_CALL(c, "dot_attn_edge_backward_rows", da_with_bias(DA_EDGE, bias), true);
  DA_CALL_BWD(c);
  c.bias = bias; c.bias_head_stride = bias_head_stride; c.dbias = dbias; c.edge = {e, lde, de, ldde};
  return da_launch(c);
}
