// K21 -- gatv2_attention: the GATv2 score a . LeakyReLU(x_dst_i + x_src_j) over the entries of every row of a sparse pattern whose row
// side and column side are different tables, for H heads at once, in one pass, and both sides of its gradient.  One kernel family in
// the shape of K19 and K20: (forward | backward rows | backward columns) x (long | row), instantiated per lane shape; the two row
// passes also per SHARED, the compile-time flag of v == x_src, and per DROP, that of the seeded dropout of the coefficients
// (gatv2_attention_dropout); all three passes per EDGE, that of a feature row per entry inside the score (gatv2_attention_edge); and
// the two kernels of the staged reduce of da.  The kernels of the two
// row passes are da_family.h's, shared with K19 and K20, on V2Fam below; the column pass and the reduce of da are written here.
//
// Arithmetic.  For an entry e = (i, j) of row i, c(e) its index in the CALLER's order (perm), per head h, feature f:
//   t[f] = x_dst[i, h, f] + x_src[j, h, f]             one rounded add
//   g[f] = t[f] > 0 ? t[f] : slope t[f]                one rounded product
//   s    = sum_f a[h, f] g[f]                          a fixed order: the lane's four elements (dot4), then the head's butterfly
//                                                      (da_head_sum) -- the same bits in the forward and in the backward
//   p    = exp(s - m[i, h]) / Z[i, h]                  m, Z [n_rows x H]: the row's maximum of s and its sum of exp(s - m)
//   out[i, h, :] = sum_e p v[j, h, :]                  SHARED: v is x_src, the gathered row serves both, one gather per entry
//   backward_rows:  D = <G[i, h], out[i, h]>,  dp = <G[i, h], v[j, h]>,  S = p (dp - D),
//     dx_dst[i, h, f] = sum_e S a[h, f] g'(t[f])  (g' = 1 for t > 0, else the slope: the slope at t == 0, as torch), held in registers
//     and written once per row,  P[c, h] = p and S[c, h] = S for the column side.
//   backward_cols, on the transposed pattern: column j holds x_src[j] and a, gathers x_dst[i] and S[c] per entry:
//     dx_src[j, h, f] = sum_e S a[h, f] g'(t[f]),  da[h, f] = sum over all entries of S g(t[f]).
//   dv = spmm^T(P, G) is K17 on the transposed pattern, the caller's launch.
//   The forward keeps out, m and Z, all the backward reads -- nothing per entry.
//   DROP: out[i, h, :] = sum_e p mask[c, h] v[j, h, :], mask in {0, 1 / (1 - p_drop)}: a dropped entry stays in Z, and m and Z are the
//     undropped softmax's.  mask[c, h] is K19's: element c H + h of the flat layout of k7_dropout.hip's mask kernel on the launcher's
//     stream id, drawn in registers in both row passes (da_keep_batch, da_lanes.h) -- no mask tensor exists.  backward_rows: S = p (mask
//     <G, v> - D), P[c, h] = p mask.  The forward then carries c and reads perm.  The column pass reads S alone: one variant serves both.
//   EDGE: t[f] = (x_dst[i, h, f] + x_src[j, h, f]) + e[c, h, f], two rounded adds in this order, the same bits in all three passes; e
//     [nnz x H F] is a row table at the CALLER's entry index, and enters the score alone: out is the sum over v as before.  A lane asks
//     for its 16 bytes of the entry's e row right behind the batch's gather (v2_gather), at the entry index the walk carries -- the
//     forward carries it too and reads perm, as under DROP.  backward_rows: de[c, h, f] = S a[h, f] g'(t[f]), the term dx_dst sums over
//     the row, stored by every lane once per entry (16 bytes) where de is asked for: an entry belongs to one row, in a long row to one
//     piece, so nothing is zeroed or added and there are no atomics.  The column pass forms t with e[c] gathered beside x_dst[i] and
//     S[c]: it has EDGE kernels of its own, which read g.e and g.lde alone -- DaArgs::de, dbias and ldde hold the da records there.
//     e = 0: t + 0 is t bit for bit (an exact zero may change its sign, which LeakyReLU and its slope treat alike), so every output has
//     gatv2_attention's bits.  EDGE goes with SHARED and not with DROP.  The unroll is da_unroll's at every lane shape: no EDGE kernel
//     spills at it (the e rows are one more gathered row per entry, and the widest lane shapes hold one or two entries in flight).
//   BF16 (forward only, inference: gatv2_attention_bf16, gatv2_attention_edge_bf16): x_src, the separate v and, under EDGE, e are rows of
//     H*F bf16 values, a lane's chunk one 8-byte load widened in registers (da_load_row, da_lanes.h); x_dst and a stay float, and
//     everything after the load sees the fp32 kernels' values in their order: the result of the fp32 forward on the widened tables bit
//     for bit.  Neither m nor Z is written.  BF16 goes with SHARED and EDGE and not with DROP; there is no backward pass on it.
//
// Lane mapping: K19's (da_lanes.h).  Rows are H*F floats, heads side by side, NOT padded; F a power of two in 4..256.  A group of LPR
// lanes holds one row, VEC chunks of 4 floats (16-byte loads) per lane; the chunks of a head sit on LH = F / 4 adjacent lanes of one
// chunk slot.  The walked side's own row and the lane's chunk of a are loaded once per row; per entry a lane loads its 16 bytes of the
// gathered row (and of v_j without SHARED; the S scalars of its heads in the column pass), several entries in flight (v2_unroll), the
// indices of the next batch asked for under this batch's arithmetic (V2Fam::walk, after K19's).  One __expf per (entry, head)
// goes into the online (m, Z, acc) state (da_fold).
//
// Long rows (and long columns) go through partial records (the rule of long_rows.h), one wave per chunk: its lane groups walk the
// piece entry-interleaved and are merged by a fixed butterfly (the forward: maximum first, one rescale), and records merge in chunk
// order.  A record is (acc[H F], m[H], Z[H]) forward and the H F sums of dx backward.
//
// da.  The column pass keeps the lane's chunk of da in registers, as a compensated sum (v2_da_add).  A work-group of the column
// kernel takes the columns that BEGIN inside one 2048-entry chunk of the transposed entry array (a column without entries begins
// where the next one does) -- work-groups of about equal work whatever the degrees are, which a fixed share of the columns is not:
// on an R-MAT graph the heavy columns sit a power of two apart -- so a wave leaves ONE record of H F floats for all its columns, the
// butterfly of its lane groups; a wave of the long-column kernel leaves one per chunk.  Two small kernels add the records in a
// fixed order (V2_DA_STAGE partial sums, then their sum, compensated too), as the GATv2 level's da reduce does.  No LDS anywhere.
//
// Exactness.  No LDS, no float atomics, every sum in a fixed order: two runs give the same bits.
//   a row without entries   out = m = Z = dx_dst = 0 exactly; a column without entries dx_src = 0
//   a row of one entry      out_i = v_j bit for bit and S = 0 exactly: D and dp are formed by the same routine on the same bits;
//                           DROP: out_i = mask v_j bit for bit; S = 0 exactly where the entry is dropped or mask is a power of two,
//                           otherwise mask <G, v> against <G, mask v>, two roundings apart
//   all entries dropped     (and every row under p_drop = 1) exact zeros in out
//   SHARED                  the same operations on the same values as the kernels without the flag fed a copy of x_src
#include "da_family.h"
#include <math.h>
#include <type_traits>

namespace pygat {

// The kernels take K19's argument block (DaArgs, da_lanes.h), so that its lane mapping and entry-index helpers serve as they stand:
//   row passes:   q = x_dst (ldq),  k = x_src (ldk),  v (ldv; SHARED: not looked at),  bias = a [H x F],  scale = the negative slope,
//                 dq = dx_dst (lddq)
//   column pass:  the walked pattern is the transposed one: q = x_src (the walked side),  k = x_dst (the gathered side),  bias = a,
//                 S read at the caller's entry index,  dq = dx_src,  de = the da records of the long-column kernel (one per chunk),
//                 dbias = those of the column kernel (one per wave),  ldde = H F
constexpr int V2_DA_STAGE = 128;               // partial sums between the da records and da

// entries in flight: da_unroll's values, under EDGE too (no kernel of the family uses scratch at them)
__host__ __device__ constexpr int v2_unroll(bool bwd, int vec, bool /*edge*/) { return da_unroll(bwd, vec); }

__device__ __forceinline__ float4 v2_t(const float4& x, const float4& y) {
  return make_float4(__fadd_rn(x.x, y.x), __fadd_rn(x.y, y.y), __fadd_rn(x.z, y.z), __fadd_rn(x.w, y.w));
}
__device__ __forceinline__ float v2_leaky1(float t, float slope) { return t > 0.f ? t : __fmul_rn(slope, t); }
__device__ __forceinline__ float4 v2_leaky(const float4& t, float slope) {
  return make_float4(v2_leaky1(t.x, slope), v2_leaky1(t.y, slope), v2_leaky1(t.z, slope), v2_leaky1(t.w, slope));
}
// y += c a g'(t)
__device__ __forceinline__ void v2_dside(float4& y, float c, const float4& a, const float4& t, float slope) {
  const float cs = c * slope;
  y.x = fmaf(t.x > 0.f ? c : cs, a.x, y.x); y.y = fmaf(t.y > 0.f ? c : cs, a.y, y.y);
  y.z = fmaf(t.z > 0.f ? c : cs, a.z, y.z); y.w = fmaf(t.w > 0.f ? c : cs, a.w, y.w);
}
// s += x with the rounding error of the sum carried in c (Kahan), every operation a rounded one in this order; s - c is the sum
__device__ __forceinline__ void v2_kahan(float& s, float& c, float x) {
  const float y = __fsub_rn(x, c), t = __fadd_rn(s, y);
  c = __fsub_rn(__fsub_rn(t, s), y);
  s = t;
}
// da += S g, compensated: da is a sum over ALL entries, which torch forms pairwise; a plain chain over a hub column of 699 entries at
// one lane group per wave missed four times an fp32 torch run's own error by a few per cent at F = 64 and 256
__device__ __forceinline__ void v2_da_add(float4& s, float4& c, float S, const float4& g) {
  v2_kahan(s.x, c.x, __fmul_rn(S, g.x)); v2_kahan(s.y, c.y, __fmul_rn(S, g.y));
  v2_kahan(s.z, c.z, __fmul_rn(S, g.z)); v2_kahan(s.w, c.w, __fmul_rn(S, g.w));
}
// the score of one (entry, chunk slot) from t: every lane of the head gets the head's
template <int LPR>
__device__ __forceinline__ float v2_score(const DaArgs& g, const float4& a, const float4& t) {
  return da_head_sum<LPR>(dot4(a, v2_leaky(t, g.scale)), g.LH);
}

// the entry index a walk carries: c(e) H, the place of the entry's scalars (da_entry); under EDGE c(e) itself, which places the
// entry's rows of e and de, and v2_scalars turns it into the place of the scalars
template <bool EDGE>
__device__ __forceinline__ int64_t v2_entry(const DaArgs& g, int64_t pos) {
  if constexpr (EDGE) return g.perm ? (int64_t)g.perm[pos] : pos;
  else return da_entry(g, pos);
}
template <bool EDGE>
__device__ __forceinline__ int64_t v2_scalars(const DaArgs& g, int64_t ent) {
  if constexpr (EDGE) return ent * g.H;
  else return ent;
}

// U gathered entries, loaded before any is used.  MODE 0: forward, 1: backward rows (x = x_src[j]; v = v[j] without SHARED), 2: the
// column pass (x = x_dst[i]; s = S[c, head of the chunk slot]).  EDGE: e = e[c], the entry's own row.  t: the argument of LeakyReLU
// from the walked side's own row, x_dst + x_src first and e behind it in every pass
template <int VEC, int U, bool EDGE>
struct V2EdgeRows {
  float4 e[U][VEC];
};
template <int VEC, int U>
struct V2EdgeRows<VEC, U, false> {};         // (an empty base: without EDGE the struct is what it was)
template <int VEC, int U, int MODE, bool SHARED, bool EDGE>
struct V2Rows : V2EdgeRows<VEC, U, EDGE> {
  static constexpr bool SEP = MODE != 2 && !SHARED;
  float4 x[U][VEC];
  float4 v[SEP ? U : 1][SEP ? VEC : 1];
  float s[MODE == 2 ? U : 1][MODE == 2 ? VEC : 1];
  __device__ __forceinline__ const float4& val(int u, int c) const {
    if constexpr (SEP) return v[u][c];
    else return x[u][c];
  }
  __device__ __forceinline__ float4 t(const float4& own, int u, int c) const {
    if constexpr (EDGE) return v2_t(MODE == 2 ? v2_t(x[u][c], own) : v2_t(own, x[u][c]), this->e[u][c]);
    else if constexpr (MODE == 2) return v2_t(x[u][c], own);
    else return v2_t(own, x[u][c]);
  }
};
// T: the element type of the gathered tables x, v and e (float, or da_bf16 in the inference forward: g.k, g.v and g.e then point at
// bf16 rows, their strides counting elements all the same)
template <int VEC, int U, int MODE, bool SHARED, bool EDGE, typename T = float>
__device__ __forceinline__ void v2_gather(const DaArgs& g, const DaLane<VEC>& ln, const int32_t (&src)[U], const int64_t (&ent)[U],
                                          V2Rows<VEC, U, MODE, SHARED, EDGE>& w) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
    da_load_row<VEC>(reinterpret_cast<const T*>(g.k) + (int64_t)src[u] * g.ldk, ln, w.x[u]);
    if constexpr (MODE != 2 && !SHARED) da_load_row<VEC>(reinterpret_cast<const T*>(g.v) + (int64_t)src[u] * g.ldv, ln, w.v[u]);
    if constexpr (EDGE) da_load_row<VEC>(reinterpret_cast<const T*>(g.e) + ent[u] * g.lde, ln, w.e[u]);
    if constexpr (MODE == 2) {
#pragma unroll
      for (int v = 0; v < VEC; ++v) w.s[u][v] = g.S[v2_scalars<EDGE>(g, ent[u]) + ln.head[v]];
    }
  }
}

// what every pass holds of the walked side: its own row (x_dst[i]; x_src[j] in the column pass) and the lane's chunks of a
template <int VEC>
struct V2Own {
  float4 x[VEC], a[VEC];
};

// the key of a kernel's draws: K19's under DROP, nothing without
template <bool DROP> using V2Key = std::conditional_t<DROP, uint2, DaNoKey>;

// ------------------------------------------------------------------------------------------------------------------------ forward
// ent is looked at under DROP alone: ent[u] + head is the entry's flat mask index, and (p keep) v goes into acc while Z takes p whole
// (under EDGE the gather has used it already)
template <int LPR, int VEC, bool SHARED, bool DROP, bool EDGE>
struct V2FwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, [[maybe_unused]] const DaLane<VEC>& ln, [[maybe_unused]] V2Key<DROP> key,
                                              const V2Own<VEC>& r, DaState<VEC>& st, const V2Rows<VEC, U, 0, SHARED, EDGE>& w,
                                              [[maybe_unused]] const int64_t (&ent)[U]) {
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) da_keep_batch<VEC, U>(g, ln, key, ent, keep);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float s = v2_score<LPR>(g, r.a[v], w.t(r.x[v], u, v));
        da_fold<false, DROP>(st.m[v], st.z[v], st.acc[v], s, 0.f, DROP ? keep[u][v] : 1.f, w.val(u, v));
      }
  }
};

// ------------------------------------------------------------------------------------------------------------- backward, row side
template <int VEC>
struct V2BwdRow : DaGrad<VEC> {   // what the backward holds of its row
  V2Own<VEC> own;
};

// the backward's fold of a batch; ctx: the row (V2BwdRow) and the lane's chunks of dx_dst.  In a row of one entry out_i is v_j bit for
// bit, so dp and D are one routine on the same bits and S is an exact zero
// DROP: the batch's keep factors are drawn again, as K19's backward does; an entry's multiplies <G_i, v_j> -- D_i = <G_i, out_i> is the
// row term of the dropped sum already -- and the stored P is p keep, what the transposed SpMM of dv multiplies G with; the column pass
// reads S alone and is the same launch with and without dropout.  In a row of one entry out_i is keep v_j bit for bit; S is an exact
// zero where the entry is dropped and where keep is a power of two, and otherwise a rounding of keep dp against one of D
// EDGE: ent[u] is c(e) itself; every lane also stores its chunk of de[c(e)] = S a g'(t), the term of dx_dst, where de is asked for.  In
// a row of one entry S is an exact zero and so is the row of de
template <int LPR, int VEC, bool SHARED, bool DROP, bool EDGE>
struct V2BwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, const DaLane<VEC>& ln, [[maybe_unused]] V2Key<DROP> key,
                                              const V2BwdRow<VEC>& r, float4 (&dx)[VEC], const V2Rows<VEC, U, 1, SHARED, EDGE>& w,
                                              const int64_t (&ent)[U]) {
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) da_keep_batch<VEC, U>(g, ln, key, ent, keep);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float4 t = w.t(r.own.x[v], u, v);
        const float s = v2_score<LPR>(g, r.own.a[v], t);
        const float p = __expf(s - r.m[v]) * r.rz[v];
        float dp = da_head_sum<LPR>(dot4(r.G[v], w.val(u, v)), g.LH);
        float pk = p;
        if constexpr (DROP) {
          dp *= keep[u][v];
          pk *= keep[u][v];
        }
        const float S = p * (dp - r.D[v]);
        v2_dside(dx[v], S, r.own.a[v], t, g.scale);
        if (ln.lead >> v & 1) {
          g.P[v2_scalars<EDGE>(g, ent[u]) + ln.head[v]] = pk;
          g.S[v2_scalars<EDGE>(g, ent[u]) + ln.head[v]] = S;
        }
        if constexpr (EDGE)
          if (g.de && (ln.ok >> v & 1)) {
            const float4& a = r.own.a[v];
            const float cs = S * g.scale;
            st4(g.de + ent[u] * g.ldde + ln.ofs[v], make_float4((t.x > 0.f ? S : cs) * a.x, (t.y > 0.f ? S : cs) * a.y,
                                                                (t.z > 0.f ? S : cs) * a.z, (t.w > 0.f ? S : cs) * a.w));
          }
      }
  }
};

template <int VEC, bool EDGE>
struct V2ColFold;

// the family: what the kernels of da_family.h hold of a row and how they walk it, per SHARED, DROP and EDGE (the column pass: per
// EDGE alone).  BF16: the inference forward on bf16 x_src, v and e tables; m and Z are what a backward reads, and it has none
template <bool SHARED, bool DROP = false, bool EDGE = false, bool BF16 = false>
struct V2Fam {
  static_assert(!(DROP && EDGE), "EDGE does not combine with DROP");
  static_assert(!(DROP && BF16), "bf16 tables are for inference: no dropout");
  static constexpr bool KEEP_MZ = !BF16;
  template <int VEC> using Own = V2Own<VEC>;
  template <int VEC> using Row = V2BwdRow<VEC>;
  __device__ __forceinline__ static V2Key<DROP> key([[maybe_unused]] const DaArgs& g) {
    if constexpr (DROP) return da_key<true>(g);
    else return {};
  }
  __device__ __forceinline__ static bool lone(int64_t, int64_t) { return false; }
  template <int VEC>
  __device__ __forceinline__ static void load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, V2Own<VEC>& r) {
    da_load_row<VEC>(g.q + row * g.ldq, ln, r.x);
    da_load_row<VEC>(g.bias, ln, r.a);
  }
  // The walk of all three passes, after K19's: the entries e0, e0 + step, ... < e1 of one row, handed to the pass's fold in that
  // order, U at a time and then one at a time.  The indices of the next U entries -- the other side's row and, in the backward passes,
  // the caller's entry index (da_entry) -- are asked for before this batch's gather is used, so an iteration waits for one gather, not
  // for an index and then a gather.  The forward carries no entry index and does not touch perm -- except under DROP, where the entry
  // index places the draws, and under EDGE, where it places the e rows: its forward forms it as the backward passes do (ENT).  key:
  // the key of the draws under DROP, by value.
  template <int LPR, int VEC, int MODE, typename... Ctx>
  __device__ __forceinline__ static void walk(const DaArgs& g, const DaLane<VEC>& ln, int64_t e0, int64_t e1, int64_t step, bool,
                                                V2Key<DROP> key, Ctx&... ctx) {
    static_assert(MODE != 2 || !DROP, "the column pass reads S alone: it has no DROP variant");
    static_assert(MODE == 0 || !BF16, "bf16 tables are for inference: the forward alone");
    using T = std::conditional_t<BF16, da_bf16, float>;         // the element type of the gathered tables
    using Fold = std::conditional_t<MODE == 0, V2FwdFold<LPR, VEC, SHARED, DROP, EDGE>,
                                    std::conditional_t<MODE == 1, V2BwdFold<LPR, VEC, SHARED, DROP, EDGE>, V2ColFold<VEC, EDGE>>>;
    constexpr int U = v2_unroll(MODE != 0, VEC, EDGE);
    constexpr bool ENT = MODE != 0 || DROP || EDGE;
    int64_t e = e0;
    if constexpr (U > 1) {
      int32_t src[U];
      int64_t ent[U], ent_next[U];
#pragma unroll
      for (int u = 0; u < U; ++u) ent[u] = ent_next[u] = 0;
      bool full = e + (U - 1) * step < e1;
      if (full) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          src[u] = g.col[e + u * step];
          if constexpr (ENT) ent_next[u] = v2_entry<EDGE>(g, e + u * step);
        }
      }
      while (full) {
        if constexpr (ENT) {
#pragma unroll
          for (int u = 0; u < U; ++u) ent[u] = ent_next[u];
        }
        V2Rows<VEC, U, MODE, SHARED, EDGE> w;
        v2_gather<VEC, U, MODE, SHARED, EDGE, T>(g, ln, src, ent, w);
        e += U * step;
        full = e + (U - 1) * step < e1;
        if (full) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            src[u] = g.col[e + u * step];
            if constexpr (ENT) ent_next[u] = v2_entry<EDGE>(g, e + u * step);
          }
        }
        Fold::fold(g, ln, key, ctx..., w, ent);
      }
    }
    for (; e < e1; e += step) {
      const int32_t src[1] = {g.col[e]};
      int64_t ent[1] = {0};
      if constexpr (ENT) ent[0] = v2_entry<EDGE>(g, e);
      V2Rows<VEC, 1, MODE, SHARED, EDGE> w;
      v2_gather<VEC, 1, MODE, SHARED, EDGE, T>(g, ln, src, ent, w);
      Fold::fold(g, ln, key, ctx..., w, ent);
    }
  }
  template <int LPR, int VEC>
  __device__ __forceinline__ static void bwd_load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, V2BwdRow<VEC>& r) {
    load<VEC>(g, ln, row, r.own);
    da_grad_load<LPR, VEC>(g, ln, row, r);
  }
};

// ---------------------------------------------------------------------------------------------------------- backward, column side
// the column pass's fold of a batch; ctx: the column's own row and a (V2Own), the lane's chunks of dx_src, of da and of da's
// compensation.  EDGE: t is the row pass's, e[c] behind x_dst[i] + x_src[j]
template <int VEC, bool EDGE>
struct V2ColFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, const DaLane<VEC>&, DaNoKey, const V2Own<VEC>& r, float4 (&dx)[VEC],
                                              float4 (&da)[VEC], float4 (&dc)[VEC], const V2Rows<VEC, U, 2, false, EDGE>& w,
                                              const int64_t (&)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float4 t = w.t(r.x[v], u, v);                    // x_dst[i] + x_src[j] (+ e[c]), the row pass's t
        const float S = w.s[u][v];
        v2_dside(dx[v], S, r.a[v], t, g.scale);
        v2_da_add(da[v], dc[v], S, v2_leaky(t, g.scale));
      }
  }
};

// s <- s - c, the compensated sum, before the lane groups of a wave are added
template <int VEC>
__device__ __forceinline__ void v2_settle(float4 (&s)[VEC], const float4 (&c)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) { s[v].x -= c[v].x; s[v].y -= c[v].y; s[v].z -= c[v].z; s[v].w -= c[v].w; }
}

// launch 1: one wave per chunk of the transposed pattern; the piece of every long column inside the chunk -> one partial record, the
// H F sums of dx_src; the wave's da of all its pieces -> da record `chunk`
template <int LPR, int VEC, bool EDGE>
__global__ __launch_bounds__(64) void v2_col_long_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  float4 da[VEC], dc[VEC];
  da_zero_row<VEC>(da);
  da_zero_row<VEC>(dc);
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int row, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    V2Own<VEC> r;
    da_load_row<VEC>(g.q + (int64_t)row * g.ldq, ln, r.x);
    da_load_row<VEC>(g.bias, ln, r.a);
    float4 dx[VEC];
    da_zero_row<VEC>(dx);
    V2Fam<false, false, EDGE>::template walk<LPR, VEC, 2>(g, ln, e0 + grp, e1, EPW, false, DaNoKey{}, r, dx, da, dc);
    da_wave_sum<LPR, VEC>(dx);
    if (grp == 0) da_store_row<VEC>(g.part + long_record(blockIdx.x, slot) * g.pstride, ln, dx);
  });
  v2_settle<VEC>(da, dc);
  da_wave_sum<LPR, VEC>(da);
  if (grp == 0) da_store_row<VEC>(g.de + (int64_t)blockIdx.x * g.ldde, ln, da);
}

// the first c in [0, n] with rowptr[c] >= x (x <= rowptr[n])
__device__ __forceinline__ int v2_first_at(const int32_t* rowptr, int n, int64_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] >= x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// launch 2: one work-group per chunk of LONG_CHUNK entries: the columns that begin inside the chunk (the last work-group: from its
// chunk on, the columns without entries at the end among them), a lane group every (lane groups of the work-group)-th of them, so a
// wave's da stays in registers over all its columns and leaves one record
template <int LPR, int VEC, bool EDGE>
__global__ __launch_bounds__(256) void v2_col_row_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane / LPR;
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  V2Own<VEC> r;
  da_load_row<VEC>(g.bias, ln, r.a);
  float4 da[VEC], dc[VEC];
  da_zero_row<VEC>(da);
  da_zero_row<VEC>(dc);
  const int64_t x0 = (int64_t)blockIdx.x * LONG_CHUNK;
  const int c0 = v2_first_at(g.rowptr, g.n, x0);
  const int c1 = blockIdx.x + 1 == gridDim.x ? g.n : v2_first_at(g.rowptr, g.n, x0 + LONG_CHUNK);
  for (int64_t base = c0 + wave * EPW; base < c1; base += 4 * EPW) {                              // (uniform in the wave)
    const int64_t row = base + grp;
    if (row >= c1) continue;                                   // (whole lane groups; nothing inside the loop crosses a group)
    const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
    float4 dx[VEC];
    da_zero_row<VEC>(dx);
    if (end - start > LONG_ROW) {                              // (its da went into the long-column kernel's records)
      for_long_records(start, end, [&](int64_t rec) {
        const float* p = g.part + rec * g.pstride;
#pragma unroll
        for (int v = 0; v < VEC; ++v) da_add(dx[v], ld4(p + ln.ofs[v]));
      });
    } else if (end > start) {
      da_load_row<VEC>(g.q + row * g.ldq, ln, r.x);
      V2Fam<false, false, EDGE>::template walk<LPR, VEC, 2>(g, ln, start, end, 1, false, DaNoKey{}, r, dx, da, dc);
    }
    da_store_row<VEC>(g.dq + row * g.lddq, ln, dx);
  }
  v2_settle<VEC>(da, dc);
  da_wave_sum<LPR, VEC>(da);
  if (grp == 0) da_store_row<VEC>(g.dbias + ((int64_t)blockIdx.x * 4 + wave) * g.ldde, ln, da);
}

// the da records -> da, two launches in a fixed order: V2_DA_STAGE work-groups, each the sum of every V2_DA_STAGE-th record; then
// their sum.  Both sums are compensated (Kahan, in fp32, every operation a rounded one in this order): da is a sum over ALL entries
// whose partial sums reach the size of the result long before the end, and a plain chain of 128 such steps alone cost more than the
// whole of the rest (hub pattern, 4 x 64: 1.3e-4 on |da| = 201 against 3.3e-5 of an fp32 torch run)
__global__ __launch_bounds__(256) void v2_da_stage_kernel(int R, int nrec, const float* __restrict__ part, float* __restrict__ out2) {
  for (int c = threadIdx.x; c < R; c += 256) {
    float acc = 0.f, comp = 0.f;
    int b = blockIdx.x;
    for (; b + 3 * V2_DA_STAGE < nrec; b += 4 * V2_DA_STAGE) {
      const float x0 = part[(int64_t)b * R + c], x1 = part[(int64_t)(b + V2_DA_STAGE) * R + c];
      const float x2 = part[(int64_t)(b + 2 * V2_DA_STAGE) * R + c], x3 = part[(int64_t)(b + 3 * V2_DA_STAGE) * R + c];
      v2_kahan(acc, comp, x0); v2_kahan(acc, comp, x1); v2_kahan(acc, comp, x2); v2_kahan(acc, comp, x3);
    }
    for (; b < nrec; b += V2_DA_STAGE) v2_kahan(acc, comp, part[(int64_t)b * R + c]);
    out2[(int64_t)blockIdx.x * R + c] = acc;
  }
}
__global__ __launch_bounds__(256) void v2_da_final_kernel(int R, const float* __restrict__ part, float* __restrict__ da) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= R) return;
  float acc = 0.f, comp = 0.f;
  for (int b = 0; b < V2_DA_STAGE; ++b) v2_kahan(acc, comp, part[(int64_t)b * R + c]);
  da[c] = acc;
}

// the table of the family: (SHARED, DROP, EDGE, forward | backward rows | columns, long | row, lane shape) -> the kernel.  What a
// launcher starts and what pygat_kernel_footprint reports on both come from here.  pass: 0 forward, 1 backward rows, 2 columns (per
// EDGE alone).  BF16: the forward pair alone, null for the other passes
template <int LPR, int VEC, bool SHARED, bool DROP, bool EDGE, bool BF16>
static const void* v2_kernel_at(int pass, bool lng) {
  if constexpr (BF16) {
    if (pass != 0) return nullptr;
  } else {
    if (pass == 2) return lng ? reinterpret_cast<const void*>(&v2_col_long_kernel<LPR, VEC, EDGE>)
                              : reinterpret_cast<const void*>(&v2_col_row_kernel<LPR, VEC, EDGE>);
    if (pass == 1) return lng ? reinterpret_cast<const void*>(&da_bwd_long_kernel<V2Fam<SHARED, DROP, EDGE>, LPR, VEC>)
                              : reinterpret_cast<const void*>(&da_bwd_row_kernel<V2Fam<SHARED, DROP, EDGE>, LPR, VEC>);
  }
  return lng ? reinterpret_cast<const void*>(&da_fwd_long_kernel<V2Fam<SHARED, DROP, EDGE, BF16>, LPR, VEC>)
             : reinterpret_cast<const void*>(&da_fwd_row_kernel<V2Fam<SHARED, DROP, EDGE, BF16>, LPR, VEC>);
}
template <bool SHARED, bool DROP, bool EDGE, bool BF16 = false>
static const void* v2_kernel_of(int pass, bool lng, int lpr, int vec) {
  PYGAT_DA_DISPATCH(lpr, vec, return (v2_kernel_at<LPR, VEC, SHARED, DROP, EDGE, BF16>(pass, lng)));
  return nullptr;
}
// (the column pass has one variant per EDGE: whatever else is asked for, the kernels without SHARED and DROP; EDGE is without DROP;
// bf16 tables: the forward alone, without DROP)
static const void* v2_kernel(bool shared, bool drop, bool edge, bool bf16, int pass, bool lng, int lpr, int vec) {
  if (bf16) {
    if (drop || pass != 0) return nullptr;
    if (edge) return shared ? v2_kernel_of<true, false, true, true>(pass, lng, lpr, vec) : v2_kernel_of<false, false, true, true>(pass, lng, lpr, vec);
    return shared ? v2_kernel_of<true, false, false, true>(pass, lng, lpr, vec) : v2_kernel_of<false, false, false, true>(pass, lng, lpr, vec);
  }
  if (pass == 2) return edge ? v2_kernel_of<false, false, true>(pass, lng, lpr, vec) : v2_kernel_of<false, false, false>(pass, lng, lpr, vec);
  if (edge) return shared ? v2_kernel_of<true, false, true>(pass, lng, lpr, vec) : v2_kernel_of<false, false, true>(pass, lng, lpr, vec);
  if (drop) return shared ? v2_kernel_of<true, true, false>(pass, lng, lpr, vec) : v2_kernel_of<false, true, false>(pass, lng, lpr, vec);
  return shared ? v2_kernel_of<true, false, false>(pass, lng, lpr, vec) : v2_kernel_of<false, false, false>(pass, lng, lpr, vec);
}

// pygat_kernel_footprint: <prefix>{fwd,bwd,col}_{long,row}_l<LPR>v<VEC> (the lane shapes of PYGAT_DA_DISPATCH); k21_: a v table of its
// own, k21s_: SHARED, k21d_: DROP, k21ds_: DROP and SHARED (fwd and bwd only: the column pass has one variant, under k21_);
// k21e_: EDGE, with a column pass of its own, k21es_: EDGE and SHARED (fwd and bwd only); k21h_, k21hs_, k21he_, k21hes_: the same four
// on bf16 tables (fwd only); k21_da_stage, k21_da_final: the reduce of da
int footprint_k21(const char* name, int* regs, int* scratch) {
  static const struct { const char* prefix; bool shared, drop, edge, bf16; } names[] = {
      {"k21_", false, false, false, false}, {"k21s_", true, false, false, false}, {"k21d_", false, true, false, false},
      {"k21ds_", true, true, false, false}, {"k21e_", false, false, true, false}, {"k21es_", true, false, true, false},
      {"k21h_", false, false, false, true}, {"k21hs_", true, false, false, true}, {"k21he_", false, false, true, true},
      {"k21hes_", true, false, true, true}};
  const void* fn = nullptr;
  if (!strcmp(name, "k21_da_stage")) fn = reinterpret_cast<const void*>(&v2_da_stage_kernel);
  if (!strcmp(name, "k21_da_final")) fn = reinterpret_cast<const void*>(&v2_da_final_kernel);
  DaKernelName k;
  for (const auto& nm : names)
    if (!fn && da_parse_kernel_name(name, nm.prefix, &k) && (k.pass != 2 || !(nm.shared || nm.drop)))
      fn = v2_kernel(nm.shared, nm.drop, nm.edge, nm.bf16, k.pass, k.lng, k.lpr, k.vec);
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k21{,s,d,ds,e,es}_{fwd,bwd}_{long,row}_l<LPR>v<VEC>, "
              "k21{,e}_col_{long,row}_l<LPR>v<VEC>, k21h{,s,e,es}_fwd_{long,row}_l<LPR>v<VEC>, k21_da_stage, k21_da_final)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

#define V2_PAD_HINT "zero-padding the columns of x_dst, x_src, a and v to the next allowed F leaves the first F columns of the result " \
                    "unchanged: zero columns of a add nothing to a score"

static int v2_check_shape(const char* what, int64_t nnz, int H, int F) { return da_check_shape(what, nnz, H, F, V2_PAD_HINT); }

// the workspace, in floats: the long-row records of a pass (every pass starts at the front), then the da records -- one per chunk of
// the long-column kernel, then one per wave of the column kernel, four to a chunk -- then the staged partial sums
// (the column kernel's grid: a work-group per chunk of entries, one for a pattern without entries)
static inline int64_t v2_col_blocks(int64_t nnz) { return nnz > 0 ? long_chunks(nnz) : 1; }
static inline int64_t v2_da_records(int64_t nnz) { return long_chunks(nnz) + 4 * v2_col_blocks(nnz); }
static inline int64_t v2_ws_floats(int64_t nnz, int H, int F) {
  return da_part_floats(nnz, H, F) + (v2_da_records(nnz) + V2_DA_STAGE) * (int64_t)H * F;
}

// what an entry point asks for, every argument under the name include/pygat_amd.h gives it; pass 0 forward, 1 backward rows, 2
// backward columns (there n, rowptr, col, perm are n_cols, rowptr_t, row_t, perm_t); what a pass does not have stays zero
struct V2Call {
  const char* what;
  int pass;
  int n;
  int64_t nnz;
  const int32_t *rowptr, *col, *perm;
  int H, F;
  float negative_slope;
  const float *x_dst, *a;
  const void *x_src, *v;       // float rows, or bf16 rows under kv_bytes == 2
  int64_t ldd, lds, ldv;
  int kv_bytes;                // the size of an element of x_src, v and e: 4, or 2 (the bf16 inference forward, pass 0 alone, which
                               // neither writes nor takes m and Z); 0 counts as 4
  float* out;
  int64_t ldo;
  float *m, *Z;
  const float* G;
  int64_t ldg;
  float* dx;                   // dx_dst | dx_src
  int64_t lddx;
  float *P, *S, *da;
  void *ws, *stream;
  bool dropout;                // the DROP kernels of the two row passes, on the mask of drop
  DaDrop drop;
  bool edge;                   // the EDGE kernels of all three passes, on the rows of ed (de: the row pass's alone)
  DaEdge ed;
};

// all three launchers: the checks, in one order; the kernel arguments; the piece kernel where there are long rows, then the row kernel
static int v2_launch(const V2Call& c) {
  const char* what = c.what;
  const bool cols = c.pass == 2, bf16 = c.kv_bytes == 2;
  const int talign = bf16 ? 8 : 16;                              // a lane's chunk of a gathered table: 4 elements
  const int rc = v2_check_shape(what, c.nnz, c.H, c.F);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(isfinite(c.negative_slope), "%s: negative_slope=%g, a finite slope expected", what, (double)c.negative_slope);
  const char* nname = cols ? "n_cols" : "n_rows";
  PYGAT_REQUIRE(c.n >= 0, "%s: %s=%d", what, nname, c.n);
  PYGAT_REQUIRE(c.n > 0 || c.nnz == 0, "%s: %s=0 with nnz=%lld entries", what, nname, (long long)c.nnz);
  const int HF = c.H * c.F;
  PYGAT_REQUIRE(c.rowptr, "%s: null %s", what, cols ? "rowptr_t" : "rowptr");
  PYGAT_REQUIRE(c.nnz == 0 || c.col, "%s: null %s", what, cols ? "row_t" : "col");
  DA_TABLE(what, "x_dst", c.x_dst, c.ldd, HF);
  DA_TABLE_ALIGNED(what, "x_src", c.x_src, c.lds, HF, talign);
  PYGAT_REQUIRE(c.a, "%s: null a", what);
  PYGAT_REQUIRE(aligned16(c.a), "%s: a must be 16-byte aligned", what);
  if (!cols) {
    if (c.v) DA_TABLE_ALIGNED(what, "v", c.v, c.ldv, HF, talign);      // (null: v is x_src, the SHARED kernels)
    DA_TABLE(what, "out", c.out, c.ldo, HF);
    PYGAT_REQUIRE(c.m || bf16, "%s: null m", what);
    PYGAT_REQUIRE(c.Z || bf16, "%s: null Z", what);
  }
  PYGAT_REQUIRE(c.ws, "%s: null workspace", what);
  PYGAT_REQUIRE(aligned16(c.ws), "%s: the workspace must be 16-byte aligned", what);
  if (c.pass == 1) {
    DA_TABLE(what, "G", c.G, c.ldg, HF);
    DA_TABLE(what, "dx_dst", c.dx, c.lddx, HF);
    PYGAT_REQUIRE(c.nnz == 0 || c.P, "%s: null P", what);
    PYGAT_REQUIRE(c.nnz == 0 || c.S, "%s: null S", what);
  }
  if (cols) {
    PYGAT_REQUIRE(c.nnz == 0 || c.S, "%s: null S", what);
    DA_TABLE(what, "dx_src", c.dx, c.lddx, HF);
    PYGAT_REQUIRE(c.da, "%s: null da", what);
    PYGAT_REQUIRE(aligned16(c.da), "%s: da must be 16-byte aligned", what);
  }
  if (c.edge) {
    const int re = da_check_edge(what, c.nnz, HF, c.ed, talign);
    if (re != PYGAT_OK) return re;
  }
  DropRng rng;
  if (c.dropout) {
    const int rd = da_check_drop(what, c.drop, &rng);
    if (rd != PYGAT_OK) return rd;
  }
  if (c.n == 0) return PYGAT_OK;
  DaArgs g;
  memset(&g, 0, sizeof(g));
  g.n = c.n; g.H = c.H; g.F = c.F; g.NCH = HF / 4; g.LH = c.F / 4; g.nnz = c.nnz; g.rowptr = c.rowptr; g.col = c.col;
  g.scale = c.negative_slope; g.bias = c.a; g.part = static_cast<float*>(c.ws); g.pstride = da_pstride(c.H, c.F);
  if (cols) { g.q = static_cast<const float*>(c.x_src); g.ldq = c.lds; g.k = c.x_dst; g.ldk = c.ldd; }
  else {
    g.q = c.x_dst; g.ldq = c.ldd; g.k = static_cast<const float*>(c.x_src); g.ldk = c.lds; g.v = static_cast<const float*>(c.v);
    g.ldv = c.ldv;
    g.out = c.out; g.ldo = c.ldo; g.m = c.m; g.Z = c.Z;
  }
  if (c.pass != 0) { g.perm = c.perm; g.dq = c.dx; g.lddq = c.lddx; g.S = c.S; }   // (the forward walks in CSR order alone)
  if (c.pass == 1) { g.G = c.G; g.ldg = c.ldg; g.P = c.P; }
  if (c.dropout) { g.perm = c.perm; g.rng = rng; }                                 // (... but for the draws: its entry index places them)
  if (c.edge) { g.perm = c.perm; g.e = c.ed.e; g.lde = c.ed.lde; }                 // (... and for the e rows)
  if (c.edge && c.pass == 1) { g.de = c.ed.de; g.ldde = c.ed.ldde; }               // (the column pass: de and ldde are the da records')
  DaGrid gd = da_grid(c.n, c.nnz, c.H, c.F);
  float* stage = nullptr;
  if (cols) {
    gd.blocks = (unsigned)v2_col_blocks(c.nnz);
    g.ldde = HF;
    g.de = g.part + da_part_floats(c.nnz, c.H, c.F);
    g.dbias = g.de + (int64_t)gd.chunks * HF;
    stage = g.de + v2_da_records(c.nnz) * HF;
  }
  hipStream_t st = (hipStream_t)c.stream;
  const bool shared = !cols && !c.v;
  da_launch_pair(v2_kernel(shared, c.dropout, c.edge, bf16, c.pass, true, gd.lpr, gd.vec),
                 v2_kernel(shared, c.dropout, c.edge, bf16, c.pass, false, gd.lpr, gd.vec), g, gd.chunks, gd.blocks, c.stream);
  if (cols) {
    const int nrec = (int)(gd.chunks + 4 * gd.blocks);
    hipLaunchKernelGGL(v2_da_stage_kernel, dim3(V2_DA_STAGE), dim3(256), 0, st, HF, nrec, (const float*)g.de, stage);
    hipLaunchKernelGGL(v2_da_final_kernel, dim3((unsigned)cdiv(HF, 256)), dim3(256), 0, st, HF, (const float*)stage, c.da);
  }
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_v2_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "v2_attn_workspace_bytes: null bytes");
  const int rc = v2_check_shape("v2_attn_workspace_bytes", nnz, H, F);
  if (rc != PYGAT_OK) return rc;
  *bytes = (size_t)v2_ws_floats(nnz, H, F) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_v2_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F,
                                     float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds,
                                     const float* a, const float* v, int64_t ldv, float* out, int64_t ldo, float* m, float* Z, void* ws,
                                     void* stream) {
  V2Call c = {};
  c.what = "v2_attn_forward"; c.pass = 0; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.H = H; c.F = F;
  c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v; c.ldv = ldv;
  c.out = out; c.ldo = ldo; c.m = m; c.Z = Z; c.ws = ws; c.stream = stream;
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                           int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                           int64_t lds, const float* a, const float* v, int64_t ldv, const float* out, int64_t ldo,
                                           const float* m, const float* Z, const float* G, int64_t ldg, float* dx_dst, int64_t lddx,
                                           float* P, float* S, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_backward_rows"; c.pass = 1; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H;
  c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v;
  c.ldv = ldv; c.out = const_cast<float*>(out); c.ldo = ldo; c.m = const_cast<float*>(m); c.Z = const_cast<float*>(Z); c.G = G;
  c.ldg = ldg; c.dx = dx_dst; c.lddx = lddx; c.P = P; c.S = S; c.ws = ws; c.stream = stream;
  return v2_launch(c);
}

// the two row passes with seeded dropout of the coefficients (the DROP instantiations): out = sum_e alpha mask v, mask[c(e), h] element
// c(e) H + h of the flat layout pygat_dropout_mask(nnz H, p, seed, stream_id) writes, drawn in registers in both passes -- the mask of
// pygat_dot_attn_dropout_forward.  The forward takes perm: the entry index places the draws.  pygat_v2_attn_backward_cols reads S alone
// and serves as it is
extern "C" int pygat_v2_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                             int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                             int64_t lds, const float* a, const float* v, int64_t ldv, float p, const void* seed,
                                             uint32_t stream_id, float* out, int64_t ldo, float* m, float* Z, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_dropout_forward"; c.pass = 0; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H;
  c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v; c.ldv = ldv;
  c.out = out; c.ldo = ldo; c.m = m; c.Z = Z; c.ws = ws; c.stream = stream; c.dropout = true; c.drop = {p, seed, stream_id};
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                                   const int32_t* perm, int H, int F, float negative_slope, const float* x_dst,
                                                   int64_t ldd, const float* x_src, int64_t lds, const float* a, const float* v,
                                                   int64_t ldv, float p, const void* seed, uint32_t stream_id, const float* out,
                                                   int64_t ldo, const float* m, const float* Z, const float* G, int64_t ldg,
                                                   float* dx_dst, int64_t lddx, float* P, float* S, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_dropout_backward_rows"; c.pass = 1; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm;
  c.H = H; c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v;
  c.ldv = ldv; c.out = const_cast<float*>(out); c.ldo = ldo; c.m = const_cast<float*>(m); c.Z = const_cast<float*>(Z); c.G = G;
  c.ldg = ldg; c.dx = dx_dst; c.lddx = lddx; c.P = P; c.S = S; c.ws = ws; c.stream = stream; c.dropout = true;
  c.drop = {p, seed, stream_id};
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_backward_cols(int n_cols, int64_t nnz, const int32_t* rowptr_t, const int32_t* row_t,
                                           const int32_t* perm_t, int H, int F, float negative_slope, const float* x_dst, int64_t ldd,
                                           const float* x_src, int64_t lds, const float* a, const float* S, float* dx_src,
                                           int64_t lddx, float* da, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_backward_cols"; c.pass = 2; c.n = n_cols; c.nnz = nnz; c.rowptr = rowptr_t; c.col = row_t; c.perm = perm_t;
  c.H = H; c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a;
  c.S = const_cast<float*>(S); c.dx = dx_src; c.lddx = lddx; c.da = da; c.ws = ws; c.stream = stream;
  return v2_launch(c);
}

// all three passes with a feature row per entry inside the score (the EDGE instantiations): t = (x_dst_i + x_src_j) + e_c, e [nnz x
// H*F] at the CALLER's entry index.  The forward takes perm: the entry index places the rows of e.  backward_rows writes de where it is
// asked for (a null de: not asked for); backward_cols reads e beside S
extern "C" int pygat_v2_attn_edge_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                          int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src, int64_t lds,
                                          const float* a, const float* v, int64_t ldv, const float* e, int64_t lde, float* out,
                                          int64_t ldo, float* m, float* Z, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_edge_forward"; c.pass = 0; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H;
  c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v; c.ldv = ldv;
  c.out = out; c.ldo = ldo; c.m = m; c.Z = Z; c.ws = ws; c.stream = stream; c.edge = true; c.ed = {e, lde, nullptr, 0};
  return v2_launch(c);
}

// the two inference forwards on bf16 tables (8-byte aligned rows, strides in elements): the BF16 instantiations of the forward pair,
// x_src, v and (the edge one) e rows of bf16 values; x_dst, a and out stay float.  m and Z are neither taken nor written
extern "C" int pygat_v2_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, int H, int F,
                                          float negative_slope, const float* x_dst, int64_t ldd, const void* x_src, int64_t lds,
                                          const float* a, const void* v, int64_t ldv, float* out, int64_t ldo, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_bf16_forward"; c.pass = 0; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.H = H; c.F = F;
  c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v; c.ldv = ldv;
  c.kv_bytes = 2; c.out = out; c.ldo = ldo; c.ws = ws; c.stream = stream;
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_edge_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                               int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const void* x_src,
                                               int64_t lds, const float* a, const void* v, int64_t ldv, const void* e, int64_t lde,
                                               float* out, int64_t ldo, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_edge_bf16_forward"; c.pass = 0; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H;
  c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v; c.ldv = ldv;
  c.kv_bytes = 2; c.out = out; c.ldo = ldo; c.ws = ws; c.stream = stream; c.edge = true;
  c.ed = {static_cast<const float*>(e), lde, nullptr, 0};
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_edge_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                                int H, int F, float negative_slope, const float* x_dst, int64_t ldd, const float* x_src,
                                                int64_t lds, const float* a, const float* v, int64_t ldv, const float* e, int64_t lde,
                                                const float* out, int64_t ldo, const float* m, const float* Z, const float* G,
                                                int64_t ldg, float* dx_dst, int64_t lddx, float* P, float* S, float* de, int64_t ldde,
                                                void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_edge_backward_rows"; c.pass = 1; c.n = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H;
  c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a; c.v = v;
  c.ldv = ldv; c.out = const_cast<float*>(out); c.ldo = ldo; c.m = const_cast<float*>(m); c.Z = const_cast<float*>(Z); c.G = G;
  c.ldg = ldg; c.dx = dx_dst; c.lddx = lddx; c.P = P; c.S = S; c.ws = ws; c.stream = stream; c.edge = true; c.ed = {e, lde, de, ldde};
  return v2_launch(c);
}

extern "C" int pygat_v2_attn_edge_backward_cols(int n_cols, int64_t nnz, const int32_t* rowptr_t, const int32_t* row_t,
                                                const int32_t* perm_t, int H, int F, float negative_slope, const float* x_dst,
                                                int64_t ldd, const float* x_src, int64_t lds, const float* a, const float* e, int64_t lde,
                                                const float* S, float* dx_src, int64_t lddx, float* da, void* ws, void* stream) {
  V2Call c = {};
  c.what = "v2_attn_edge_backward_cols"; c.pass = 2; c.n = n_cols; c.nnz = nnz; c.rowptr = rowptr_t; c.col = row_t; c.perm = perm_t;
  c.H = H; c.F = F; c.negative_slope = negative_slope; c.x_dst = x_dst; c.ldd = ldd; c.x_src = x_src; c.lds = lds; c.a = a;
  c.S = const_cast<float*>(S); c.dx = dx_src; c.lddx = lddx; c.da = da; c.ws = ws; c.stream = stream; c.edge = true;
  c.ed = {e, lde, nullptr, 0};
  return v2_launch(c);
}
