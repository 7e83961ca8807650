// K20 -- additive_attention: the GAT score over the entries of every row of a sparse pattern whose row side and column side are
// different tables, for H heads at once, in one pass, and the row side of its gradient.  One kernel family in K19's shape: four
// kernels (forward | backward rows) x (long | row), instantiated per lane shape, per LOGIT, the compile-time flag of the per-entry
// term, and per DROP, that of the seeded dropout of the coefficients (additive_attention_dropout).  The forward pair is da_family.h's,
// shared with K19 and K21, on AaFam below; the backward pair, whose row gradient is one scalar per head and not a row of H*F floats, is
// written here.
//
// Arithmetic.  For an entry e = (i, j) of row i, c(e) its index in the CALLER's order (perm), per head h:
//   z = s_dst[i, h] + s_src[j, h]                      one rounded add;  LOGIT: z = (s_dst[i, h] + s_src[j, h]) + u[c, h], two rounded
//                                                      adds in this order, as K15 forms it (u [nnz x H], or [nnz] with a head stride
//                                                      of 0), the same bits in both passes
//   l = z > 0 ? z : slope z                            one rounded product, never contracted into the difference below: the forward's m
//                                                      and the backward's l are the same bits
//   p = exp(l - m[i, h]) / Z[i, h]                     m, Z [n_rows x H]: the row's maximum of l and its sum of exp(l - m)
//   out[i, h] = sum_e p v[j, h]
//   backward_rows:  D = <G[i, h], out[i, h]>,  dp = <G[i, h], v[j, h]>,  T = p (dp - D),  dz = T (z > 0 ? 1 : slope)  (the slope
//     at z == 0, as torch and the reference),  ds_dst[i, h] = sum_e dz, held in registers and written once per row,  P[c, h] = p and
//     S[c, h] = dz for the column side: dv = spmm^T(P, G) and ds_src = spmm^T(S, ones[n_rows x H x 1]) are two pygat_spmm_forward
//     launches on the transposed pattern (K17).  S is the gradient of u as it is.
//   The forward keeps out, m and Z, all the backward reads -- nothing per entry.
//   DROP: out[i, h] = sum_e p mask[c, h] v[j, h], mask in {0, 1 / (1 - p_drop)}: a dropped entry stays in Z, and m and Z are the
//     undropped softmax's.  mask[c, h] is K19's: element c H + h of the flat layout of k7_dropout.hip's mask kernel on the launcher's
//     stream id, drawn in registers in both passes (da_keep_batch, da_lanes.h) -- no mask tensor exists.  backward_rows: dp = mask <G, v>,
//     T = p (dp - D), dz and ds_dst as above, P[c, h] = p mask, S[c, h] = dz.  The walk then carries c in both passes, on LOGIT's path,
//     and the forward reads perm; without LOGIT it loads no logit.
//   BF16 (forward only, inference: additive_attention_bf16): v is rows of H*F bf16 values, a lane's chunk one 8-byte load widened in
//     registers (da_load_row, da_lanes.h); s_src stays float, and everything after the load sees the fp32 kernels' values in their
//     order: the result of the fp32 forward on the widened table bit for bit.  Neither m nor Z is written.  BF16 goes with LOGIT and
//     not with DROP.
//
// Lane mapping: K19's (da_lanes.h).  Rows of v, out and G are H*F floats, heads side by side, NOT padded; F a power of two in 4..256.
// A group of LPR lanes holds one row, VEC chunks of 4 floats (16-byte loads) per lane, chunk c = c0 + 64 v; the chunks of a head sit
// on LH = F / 4 adjacent lanes of one v.  s_dst[i, :] is loaded once per row.  Per entry a lane loads s_src[j, head of its chunk], one
// 4-byte load per chunk slot -- the LH lanes of a head ask for the same word and the H floats of a column are contiguous -- and its 16
// bytes of v_j, several entries in flight (da_unroll), the indices (LOGIT: and logits) of the next batch asked for under this batch's
// arithmetic (aa_walk, after K19's da_walk).  Every lane of a head forms the same l: the forward has no butterfly.  One __expf per
// (entry, head) goes into the online (m, Z, acc) state (da_fold).  The backward's butterflies are D (once per row) and dp (per entry).
// Without LOGIT the walk does not carry the caller's entry index and the forward does not touch perm.
//
// Long rows go through partial records (the rule of long_rows.h), one wave per chunk: its lane groups walk the piece
// entry-interleaved and are merged maximum first -- rescale once, then a fixed butterfly -- and records merge in chunk order by the
// same rule.  A record is (acc[H F], m[H], Z[H]) forward and the H sums of dz backward.
//
// Exactness.  No LDS, no float atomics, every sum in a fixed order: two runs give the same bits.
//   a row without entries   out = m = Z = ds_dst = 0 exactly
//   a row of one entry      out_i = v_j bit for bit and dz = 0 exactly: D and dp are formed by the same routine on the same bits;
//                           DROP: out_i = mask v_j bit for bit; dz = 0 exactly where the entry is dropped or mask is a power of two,
//                           otherwise mask <G, v> against <G, mask v>, two roundings apart
//   all entries dropped     (and every row under p_drop = 1) exact zeros in out
//   u = 0                   changes no bit of out, ds_dst, P or S against the kernels without LOGIT (x + 0 is x), with and without DROP
//   a large negative finite u (-9e15) gives p = 0 exactly while the row keeps another entry and slope > 0 (at slope 0 l is 0: no mask)
#include "da_family.h"
#include <math.h>
#include <type_traits>

namespace pygat {

// The kernels take K19's argument block (DaArgs, da_lanes.h), so that its lane mapping and entry-index helpers serve as they stand:
//   q = s_dst [n x H] (ldq = H),  k = s_src [n_cols x H] (ldk = H),  scale = the negative slope,  bias / bstride / bhs = the logit u,
//   dq = ds_dst [n x H],  rng = the mask of the DROP kernels.  dbias, e and de are not looked at.
__device__ __forceinline__ float aa_leaky(float z, float slope) { return z > 0.f ? z : __fmul_rn(slope, z); }

// U gathered entries: the s_src scalars (one per chunk slot) and the v rows of columns src[0..U), loaded before any is used
template <int VEC, int U>
struct AaRows {
  float t[U][VEC];
  float4 v[U][VEC];
};
// T: the element type of the v table (float, or da_bf16 in the inference forward: g.v then points at bf16 rows, ldv counting elements
// all the same)
template <int VEC, int U, typename T = float>
__device__ __forceinline__ void aa_gather(const DaArgs& g, const DaLane<VEC>& ln, const int32_t (&src)[U], AaRows<VEC, U>& w) {
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) w.t[u][v] = g.k[(int64_t)src[u] * g.ldk + ln.head[v]];
    da_load_row<VEC>(reinterpret_cast<const T*>(g.v) + (int64_t)src[u] * g.ldv, ln, w.v[u]);
  }
}

// z of one (entry, chunk slot): the order of the rounded adds is the arithmetic above
template <bool LOGIT>
__device__ __forceinline__ float aa_z(float sd, float t, float u) {
  const float z = __fadd_rn(sd, t);
  return LOGIT ? __fadd_rn(z, u) : z;
}

// The walk of both passes, after K19's da_walk: the entries e0, e0 + step, ... < e1 of one row, handed to Fold::fold in that order, U
// at a time and then one at a time.  The column indices of the next U entries are asked for before this batch's gather is used, so an
// iteration waits for one gather, not for an index and then a gather.  LOGIT: the next batch's entry indices travel with its column
// indices as loaded words (da_eid_raw) and become indices only after this batch's fold, when the next batch's logits are asked for,
// ahead of the next gather.  Without LOGIT the forward carries no entry index; the backward needs it only for its stores and forms it
// whole (da_entry) a batch ahead.  DROP: the entry index places the draws, so it travels on LOGIT's path in BOTH passes (EID), the
// forward's included, whether or not there is a logit to load; ent = eid x H is then formed in the forward too.  key: the key of the
// draws under DROP (by value, K19's way), a DaNoKey without.  T: the element type of the v table (aa_gather).
template <int VEC, bool LOGIT, bool DROP, bool BWD, typename Fold, typename T = float, typename Key, typename... Ctx>
__device__ __forceinline__ void aa_walk(const DaArgs& g, const DaLane<VEC>& ln, int64_t e0, int64_t e1, int64_t step, Key key,
                                        Ctx&... ctx) {
  constexpr int U = da_unroll(BWD, VEC);
  constexpr bool EID = LOGIT || DROP;
  int64_t e = e0;
  if constexpr (U > 1) {
    int32_t src[U];
    [[maybe_unused]] int64_t ent[U], ent_next[U];
    [[maybe_unused]] int32_t raw[U], eid[U];
    DaBias<VEC, U, LOGIT> bs;
    bool full = e + (U - 1) * step < e1;
    if (full) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        src[u] = g.col[e + u * step];
        if constexpr (EID) raw[u] = da_eid_raw(g, e + u * step);
        else if constexpr (BWD) ent_next[u] = da_entry(g, e + u * step);
      }
      if constexpr (EID) da_eids<U>(g, raw, e, step, eid);
      if constexpr (LOGIT) da_bias_load<VEC, U>(g, ln, eid, bs);
    }
    while (full) {
      AaRows<VEC, U> w;
      aa_gather<VEC, U, T>(g, ln, src, w);
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
      if constexpr ((BWD || DROP) && EID) {                        // (eid: this batch's, formed after the last fold, not yet replaced)
#pragma unroll
        for (int u = 0; u < U; ++u) ent[u] = (int64_t)eid[u] * g.H;
      }
      Fold::fold(g, ln, key, ctx..., w, ent, bs);
      if constexpr (EID)
        if (full) {
          da_eids<U>(g, raw, e, step, eid);
          if constexpr (LOGIT) da_bias_load<VEC, U>(g, ln, eid, bs);
        }
    }
  }
  for (; e < e1; e += step) {
    const int32_t src[1] = {g.col[e]};
    [[maybe_unused]] int64_t ent[1] = {0};
    [[maybe_unused]] int32_t eid[1] = {0};
    if constexpr (BWD || DROP) ent[0] = da_entry(g, e);
    DaBias<VEC, 1, LOGIT> bs;
    if constexpr (LOGIT) {
      eid[0] = da_eid(g, da_eid_raw(g, e), e);
      da_bias_load<VEC, 1>(g, ln, eid, bs);
    }
    AaRows<VEC, 1> w;
    aa_gather<VEC, 1, T>(g, ln, src, w);
    Fold::fold(g, ln, key, ctx..., w, ent, bs);
  }
}

// ------------------------------------------------------------------------------------------------------------------------ forward
// s_dst[row, head of the chunk slot], once per row
template <int VEC>
__device__ __forceinline__ void aa_load_sd(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, float (&sd)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) sd[v] = g.q[row * g.ldq + ln.head[v]];
}

// the key of a kernel's draws: K19's under DROP, nothing without
template <bool DROP> using AaKey = std::conditional_t<DROP, uint2, DaNoKey>;

// the forward's fold of a batch; ctx: s_dst of the row and the row's state.  ent is looked at under DROP alone: ent[u] + head is the
// entry's flat mask index, and (p keep) v goes into acc while Z takes p whole (da_fold)
template <int VEC, bool LOGIT, bool DROP>
struct AaFwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, [[maybe_unused]] const DaLane<VEC>& ln, [[maybe_unused]] AaKey<DROP> key,
                                              const float (&sd)[VEC], DaState<VEC>& st, const AaRows<VEC, U>& w,
                                              [[maybe_unused]] const int64_t (&ent)[U], const DaBias<VEC, U, LOGIT>& bs) {
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) da_keep_batch<VEC, U>(g, ln, key, ent, keep);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float z = aa_z<LOGIT>(sd[v], w.t[u][v], LOGIT ? bs.b[u][v] : 0.f);
        da_fold<false, DROP>(st.m[v], st.z[v], st.acc[v], aa_leaky(z, g.scale), 0.f, DROP ? keep[u][v] : 1.f, w.v[u][v]);
      }
  }
};

// the family: what the forward kernels of da_family.h hold of a row and how they walk it, per LOGIT and DROP.  walk forwards to
// aa_walk, which the backward kernels below call themselves: as the family's member, K21's way, it moved the LOGIT forward at 64
// lanes a row.  BF16: the inference forward on a bf16 v table; m and Z are what a backward reads, and it has none
template <bool LOGIT, bool DROP, bool BF16 = false>
struct AaFam {
  static_assert(!(BF16 && DROP), "bf16 tables are for inference: no dropout");
  static constexpr bool KEEP_MZ = !BF16;
  template <int VEC> using Own = float[VEC];                   // s_dst of the row, per chunk slot
  __device__ __forceinline__ static AaKey<DROP> key([[maybe_unused]] const DaArgs& g) {
    if constexpr (DROP) return da_key<true>(g);
    else return {};
  }
  template <int VEC>
  __device__ __forceinline__ static void load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, float (&sd)[VEC]) {
    aa_load_sd<VEC>(g, ln, row, sd);
  }
  template <int LPR, int VEC, int PASS>
  __device__ __forceinline__ static void walk(const DaArgs& g, const DaLane<VEC>& ln, int64_t e0, int64_t e1, int64_t step, bool,
                                              AaKey<DROP> key, const float (&sd)[VEC], DaState<VEC>& st) {
    static_assert(PASS == 0, "the family serves the forward pair alone");
    aa_walk<VEC, LOGIT, DROP, false, AaFwdFold<VEC, LOGIT, DROP>, std::conditional_t<BF16, da_bf16, float>>(g, ln, e0, e1, step, key, sd,
                                                                                                       st);
  }
};

// ------------------------------------------------------------------------------------------------------------- backward, row side
template <int VEC>
struct AaRow : DaGrad<VEC> {   // what the backward holds of its row
  float sd[VEC];
};

template <int LPR, int VEC>
__device__ __forceinline__ void aa_bwd_load(const DaArgs& g, const DaLane<VEC>& ln, int64_t row, AaRow<VEC>& r) {
  aa_load_sd<VEC>(g, ln, row, r.sd);
  da_grad_load<LPR, VEC>(g, ln, row, r);
}

// the backward's fold of a batch; ctx: the row (AaRow) and the sums of dz of its heads, one per chunk slot (every lane of a head holds
// the head's).  In a row of one entry out_i is v_j bit for bit, so dp and D are one routine on the same bits and dz is an exact zero
// DROP: the batch's keep factors are drawn again, as K19's backward does (ent[u] + head is an entry's flat mask index); an entry's
// multiplies <G_i, v_j> -- D_i = <G_i, out_i> is the row term of the dropped sum already -- and the stored P is p keep, what the
// transposed SpMM of dv multiplies G with.  In a row of one entry out_i is keep v_j bit for bit; dz is an exact zero where the entry is
// dropped and where keep is a power of two (p = 0.5: 2), and otherwise a rounding of keep dp against one of D
template <int LPR, int VEC, bool LOGIT, bool DROP>
struct AaBwdFold {
  template <int U>
  __device__ __forceinline__ static void fold(const DaArgs& g, const DaLane<VEC>& ln, [[maybe_unused]] AaKey<DROP> key,
                                              const AaRow<VEC>& r, float (&ds)[VEC], const AaRows<VEC, U>& w, const int64_t (&ent)[U],
                                              const DaBias<VEC, U, LOGIT>& bs) {
    [[maybe_unused]] float keep[DROP ? U : 1][DROP ? VEC : 1];
    if constexpr (DROP) da_keep_batch<VEC, U>(g, ln, key, ent, keep);
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float z = aa_z<LOGIT>(r.sd[v], w.t[u][v], LOGIT ? bs.b[u][v] : 0.f);
        const float p = __expf(aa_leaky(z, g.scale) - r.m[v]) * r.rz[v];
        float dp = da_head_sum<LPR>(dot4(r.G[v], w.v[u][v]), g.LH);
        float pk = p;
        if constexpr (DROP) {
          dp *= keep[u][v];
          pk *= keep[u][v];
        }
        const float dz = p * (dp - r.D[v]) * (z > 0.f ? 1.f : g.scale);
        ds[v] += dz;
        if (ln.lead >> v & 1) {
          g.P[ent[u] + ln.head[v]] = pk;
          g.S[ent[u] + ln.head[v]] = dz;
        }
      }
  }
};

// launch 1: one wave per chunk; the piece of every long row inside the chunk -> one partial record, the H sums of dz
template <int LPR, int VEC, bool LOGIT, bool DROP>
__global__ __launch_bounds__(64) void aa_bwd_long_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const auto key = AaFam<LOGIT, DROP>::key(g);
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int row, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    AaRow<VEC> r;
    aa_bwd_load<LPR, VEC>(g, ln, row, r);
    float ds[VEC];
#pragma unroll
    for (int v = 0; v < VEC; ++v) ds[v] = 0.f;
    aa_walk<VEC, LOGIT, DROP, true, AaBwdFold<LPR, VEC, LOGIT, DROP>>(g, ln, e0 + grp, e1, EPW, key, r, ds);
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1)                   // lane groups of the wave, a fixed butterfly
#pragma unroll
      for (int v = 0; v < VEC; ++v) ds[v] += __shfl_xor(ds[v], off);
    if (grp == 0) {
      float* p = g.part + long_record(blockIdx.x, slot) * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (ln.lead >> v & 1) p[ln.head[v]] = ds[v];
    }
  });
}

// launch 2: one lane group per row
template <int LPR, int VEC, bool LOGIT, bool DROP>
__global__ __launch_bounds__(256) void aa_bwd_row_kernel(DaArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (row >= g.n) return;                                      // (whole lane groups; nothing below crosses a group)
  const DaLane<VEC> ln = da_lane<LPR, VEC>(g);
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
  float ds[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) ds[v] = 0.f;
  if (end - start > LONG_ROW) {
    for_long_records(start, end, [&](int64_t rec) {
      const float* p = g.part + rec * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v) ds[v] += p[ln.head[v]];
    });
  } else if (end > start) {                                    // (a row without entries: its G row is not read)
    AaRow<VEC> r;
    aa_bwd_load<LPR, VEC>(g, ln, row, r);
    aa_walk<VEC, LOGIT, DROP, true, AaBwdFold<LPR, VEC, LOGIT, DROP>>(g, ln, start, end, 1, AaFam<LOGIT, DROP>::key(g), r, ds);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (ln.lead >> v & 1) g.dq[row * g.lddq + ln.head[v]] = ds[v];
}

// the table of the family: (LOGIT, DROP, BF16, forward | backward, long | row, lane shape) -> the kernel; null where there is none
// (bf16 tables: the forward pair alone, without DROP).  What a launcher starts and what pygat_kernel_footprint reports on both come
// from here
template <int LPR, int VEC, bool LOGIT, bool DROP, bool BF16>
static const void* aa_kernel_at(bool bwd, bool lng) {
  if constexpr (BF16) {
    if (bwd) return nullptr;
  } else if (bwd) return lng ? reinterpret_cast<const void*>(&aa_bwd_long_kernel<LPR, VEC, LOGIT, DROP>)
                             : reinterpret_cast<const void*>(&aa_bwd_row_kernel<LPR, VEC, LOGIT, DROP>);
  return lng ? reinterpret_cast<const void*>(&da_fwd_long_kernel<AaFam<LOGIT, DROP, BF16>, LPR, VEC>)
             : reinterpret_cast<const void*>(&da_fwd_row_kernel<AaFam<LOGIT, DROP, BF16>, LPR, VEC>);
}
template <bool LOGIT, bool DROP, bool BF16 = false>
static const void* aa_kernel_of(bool bwd, bool lng, int lpr, int vec) {
  PYGAT_DA_DISPATCH(lpr, vec, return (aa_kernel_at<LPR, VEC, LOGIT, DROP, BF16>(bwd, lng)));
  return nullptr;
}
static const void* aa_kernel(bool logit, bool drop, bool bf16, bool bwd, bool lng, int lpr, int vec) {
  if (bf16) {
    if (drop) return nullptr;
    return logit ? aa_kernel_of<true, false, true>(bwd, lng, lpr, vec) : aa_kernel_of<false, false, true>(bwd, lng, lpr, vec);
  }
  if (drop) return logit ? aa_kernel_of<true, true>(bwd, lng, lpr, vec) : aa_kernel_of<false, true>(bwd, lng, lpr, vec);
  return logit ? aa_kernel_of<true, false>(bwd, lng, lpr, vec) : aa_kernel_of<false, false>(bwd, lng, lpr, vec);
}

// pygat_kernel_footprint: <prefix>{fwd,bwd}_{long,row}_l<LPR>v<VEC> (the lane shapes of PYGAT_DA_DISPATCH); k20_: the kernels without
// a flag, k20u_: LOGIT, k20d_: DROP, k20du_: DROP and LOGIT, k20h_: bf16 v table, k20hu_: bf16 v table and LOGIT (fwd only)
int footprint_k20(const char* name, int* regs, int* scratch) {
  static const struct { const char* prefix; bool logit, drop, bf16; } names[] = {
      {"k20_", false, false, false}, {"k20u_", true, false, false}, {"k20d_", false, true, false}, {"k20du_", true, true, false},
      {"k20h_", false, false, true}, {"k20hu_", true, false, true}};
  const void* fn = nullptr;
  DaKernelName k;
  for (const auto& nm : names)
    if (da_parse_kernel_name(name, nm.prefix, &k) && k.pass <= 1)
      fn = aa_kernel(nm.logit, nm.drop, nm.bf16, k.pass == 1, k.lng, k.lpr, k.vec);
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k20{,u,d,du,h,hu}_{fwd,bwd}_{long,row}_l<LPR>v<VEC>; k20h*: fwd only)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

#define AA_PAD_HINT "zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged"

static int aa_check_shape(const char* what, int64_t nnz, int H, int F) { return da_check_shape(what, nnz, H, F, AA_PAD_HINT); }

// what an entry point asks for, every argument under the name include/pygat_amd.h gives it; out, m and Z are written by the forward
// and read by the backward; what the forward does not have stays zero
struct AaCall {
  const char* what;
  bool bwd;
  int n_rows;
  int64_t nnz;
  const int32_t *rowptr, *col, *perm;
  int H, F;
  float negative_slope;
  const float *s_dst, *s_src;
  const void* v;               // float rows, or bf16 rows under v_bytes == 2
  int64_t ldv;
  int v_bytes;                 // the size of an element of v: 4, or 2 (the bf16 inference forward, which neither writes nor takes m and Z)
  const float* edge_logit;     // null: the kernels without LOGIT
  int logit_head_stride;
  bool dropout;                // the DROP kernels, on the mask of drop
  DaDrop drop;
  float* out;
  int64_t ldo;
  float *m, *Z;
  void *ws, *stream;
  const float* G;              // backward only from here
  int64_t ldg;
  float *ds_dst, *P, *S;
};

// both launchers: the checks, in one order; the kernel arguments; the piece kernel where there are long rows, then the row kernel
static int aa_launch(const AaCall& c) {
  const char* what = c.what;
  const bool logit = c.edge_logit != nullptr, bf16 = c.v_bytes == 2;
  const int rc = aa_check_shape(what, c.nnz, c.H, c.F);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(isfinite(c.negative_slope), "%s: negative_slope=%g, a finite slope expected", what, (double)c.negative_slope);
  PYGAT_REQUIRE(c.n_rows >= 0, "%s: n_rows=%d", what, c.n_rows);
  PYGAT_REQUIRE(c.n_rows > 0 || c.nnz == 0, "%s: n_rows=0 with nnz=%lld entries", what, (long long)c.nnz);
  const int HF = c.H * c.F;
  PYGAT_REQUIRE(c.rowptr, "%s: null rowptr", what);
  PYGAT_REQUIRE(c.nnz == 0 || c.col, "%s: null col", what);
  PYGAT_REQUIRE(c.s_dst, "%s: null s_dst", what);
  PYGAT_REQUIRE(c.s_src, "%s: null s_src", what);
  DA_TABLE_ALIGNED(what, "v", c.v, c.ldv, HF, 4 * c.v_bytes);
  DA_TABLE(what, "out", c.out, c.ldo, HF);
  PYGAT_REQUIRE(c.m || bf16, "%s: null m", what);
  PYGAT_REQUIRE(c.Z || bf16, "%s: null Z", what);
  PYGAT_REQUIRE(c.ws, "%s: null workspace", what);
  PYGAT_REQUIRE(aligned16(c.ws), "%s: the workspace must be 16-byte aligned", what);
  if (c.bwd) {
    DA_TABLE(what, "G", c.G, c.ldg, HF);
    PYGAT_REQUIRE(c.ds_dst, "%s: null ds_dst", what);
    PYGAT_REQUIRE(c.nnz == 0 || c.P, "%s: null P", what);
    PYGAT_REQUIRE(c.nnz == 0 || c.S, "%s: null S", what);
  }
  PYGAT_REQUIRE(!logit || c.logit_head_stride == 0 || c.logit_head_stride == 1, "%s: logit_head_stride=%d, 1 (edge_logit [nnz x H]) or 0 "
                "(edge_logit [nnz], shared by the heads) expected", what, c.logit_head_stride);
  DropRng rng;
  if (c.dropout) {
    const int rd = da_check_drop(what, c.drop, &rng);
    if (rd != PYGAT_OK) return rd;
  }
  if (c.n_rows == 0) return PYGAT_OK;
  DaArgs g;
  memset(&g, 0, sizeof(g));
  g.n = c.n_rows; g.H = c.H; g.F = c.F; g.NCH = HF / 4; g.LH = c.F / 4; g.nnz = c.nnz; g.rowptr = c.rowptr; g.col = c.col;
  g.scale = c.negative_slope; g.q = c.s_dst; g.ldq = c.H; g.k = c.s_src; g.ldk = c.H; g.v = static_cast<const float*>(c.v); g.ldv = c.ldv;
  g.out = c.out; g.ldo = c.ldo; g.m = c.m; g.Z = c.Z; g.part = static_cast<float*>(c.ws); g.pstride = da_pstride(c.H, c.F);
  if (c.bwd || logit || c.dropout) g.perm = c.perm;               // (the forward without a flag walks in CSR order alone)
  if (c.bwd) { g.G = c.G; g.ldg = c.ldg; g.dq = c.ds_dst; g.lddq = c.H; g.P = c.P; g.S = c.S; }
  if (logit) { g.bias = c.edge_logit; g.bhs = c.logit_head_stride; g.bstride = c.logit_head_stride ? c.H : 1; }
  if (c.dropout) g.rng = rng;
  const DaGrid gd = da_grid(c.n_rows, c.nnz, c.H, c.F);
  da_launch_pair(aa_kernel(logit, c.dropout, bf16, c.bwd, true, gd.lpr, gd.vec),
                 aa_kernel(logit, c.dropout, bf16, c.bwd, false, gd.lpr, gd.vec), g, gd.chunks, gd.blocks, c.stream);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_add_attn_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "add_attn_workspace_bytes: null bytes");
  const int rc = aa_check_shape("add_attn_workspace_bytes", nnz, H, F);
  if (rc != PYGAT_OK) return rc;
  *bytes = (size_t)da_part_floats(nnz, H, F) * sizeof(float);
  return PYGAT_OK;
}

#define AA_CALL(c, name, back)                                                                                                      \
  AaCall c = {};                                                                                                                    \
  c.what = name; c.bwd = back; c.n_rows = n_rows; c.nnz = nnz; c.rowptr = rowptr; c.col = col; c.perm = perm; c.H = H; c.F = F;    \
  c.negative_slope = negative_slope; c.s_dst = s_dst; c.s_src = s_src; c.v = v; c.ldv = ldv; c.v_bytes = 4;                         \
  c.edge_logit = edge_logit;                                                                                                        \
  c.logit_head_stride = logit_head_stride; c.out = const_cast<float*>(out); c.ldo = ldo; c.m = const_cast<float*>(m);               \
  c.Z = const_cast<float*>(Z); c.ws = ws; c.stream = stream

extern "C" int pygat_add_attn_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                      int F, float negative_slope, const float* s_dst, const float* s_src, const float* v,
                                      int64_t ldv, const float* edge_logit, int logit_head_stride, float* out, int64_t ldo, float* m,
                                      float* Z, void* ws, void* stream) {
  AA_CALL(c, "add_attn_forward", false);
  return aa_launch(c);
}

extern "C" int pygat_add_attn_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                            int H, int F, float negative_slope, const float* s_dst, const float* s_src,
                                            const float* v, int64_t ldv, const float* edge_logit, int logit_head_stride,
                                            const float* out, int64_t ldo, const float* m, const float* Z, const float* G, int64_t ldg,
                                            float* ds_dst, float* P, float* S, void* ws, void* stream) {
  AA_CALL(c, "add_attn_backward_rows", true);
  c.G = G; c.ldg = ldg; c.ds_dst = ds_dst; c.P = P; c.S = S;
  return aa_launch(c);
}

// the inference forward on a bf16 v table (8-byte aligned rows, ldv in elements): the BF16 instantiations of the forward pair.  m and
// Z are neither taken nor written.  A null edge_logit: the kernels without LOGIT; perm and logit_head_stride are then not looked at
extern "C" int pygat_add_attn_bf16_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                           int F, float negative_slope, const float* s_dst, const float* s_src, const void* v,
                                           int64_t ldv, const float* edge_logit, int logit_head_stride, float* out, int64_t ldo, void* ws,
                                           void* stream) {
  const float *m = nullptr, *Z = nullptr;
  AA_CALL(c, "add_attn_bf16_forward", false);
  c.v_bytes = 2;
  return aa_launch(c);
}

// the same two with seeded dropout of the coefficients (the DROP instantiations): out = sum_e alpha mask v, mask[c(e), h] element
// c(e) H + h of the flat layout pygat_dropout_mask(nnz H, p, seed, stream_id) writes, drawn in registers in both passes -- the mask of
// pygat_dot_attn_dropout_forward.  A null edge_logit: no term, logit_head_stride is then not looked at
extern "C" int pygat_add_attn_dropout_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm,
                                              int H, int F, float negative_slope, const float* s_dst, const float* s_src,
                                              const float* v, int64_t ldv, const float* edge_logit, int logit_head_stride, float p,
                                              const void* seed, uint32_t stream_id, float* out, int64_t ldo, float* m, float* Z,
                                              void* ws, void* stream) {
  AA_CALL(c, "add_attn_dropout_forward", false);
  c.dropout = true; c.drop = {p, seed, stream_id};
  return aa_launch(c);
}

extern "C" int pygat_add_attn_dropout_backward_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col,
                                                    const int32_t* perm, int H, int F, float negative_slope, const float* s_dst,
                                                    const float* s_src, const float* v, int64_t ldv, const float* edge_logit,
                                                    int logit_head_stride, float p, const void* seed, uint32_t stream_id,
                                                    const float* out, int64_t ldo, const float* m, const float* Z, const float* G,
                                                    int64_t ldg, float* ds_dst, float* P, float* S, void* ws, void* stream) {
  AA_CALL(c, "add_attn_dropout_backward_rows", true);
  c.G = G; c.ldg = ldg; c.ds_dst = ds_dst; c.P = P; c.S = S;
  c.dropout = true; c.drop = {p, seed, stream_id};
  return aa_launch(c);
}
