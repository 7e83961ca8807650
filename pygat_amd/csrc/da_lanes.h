// The lanes of the fused attention families over an edge pattern: K19 (k19_dot_attention.hip, the dot-product score), K20
// (k20_additive_attention.hip, the GAT score) and K21 (k21_gatv2_attention.hip, the GATv2 score).  The kernel arguments, the lane
// mapping of a row of H*F floats, the row loads (16 bytes of a float table, 8 of a bf16 one), the online softmax fold of one head and the merge of two partial records, the caller's entry index
// of a CSR position, the per-entry scalar term, the draws of the DROP instantiations (the seeded dropout of the coefficients, one copy
// for the three families), the lane-shape dispatch and the table checks of the launchers.  Moved here from
// k19_dot_attention.hip as it stood; K19's device code is the same before and after (profiles/k20_k19_unchanged.txt).  The kernels
// built on these, one copy for the three families, and the launcher tail: da_family.h.  A family's walk and folds are its own.
#pragma once
#include "long_rows.h"
#include "rng.h"
#include <float.h>

namespace pygat {

constexpr int DA_MAX_ROW = 1024;               // floats per row, H * F
constexpr float DA_SEED = -FLT_MAX;            // running-max seed: finite, so no difference of two maxima is a NaN

struct DaArgs {
  int n, H, F, NCH, LH;        // rows of the walked pattern; heads; width of a head; chunks of 4 floats per row; lanes per head
  int64_t nnz;
  const int32_t *rowptr, *col, *perm;
  const float *q, *k, *v;
  int64_t ldq, ldk, ldv;
  float scale;
  float* out;                  // forward: written; backward: read
  int64_t ldo;
  float *m, *Z;                // [n x H]  forward: written; backward: read
  const float* G;              // backward only from here
  int64_t ldg;
  float* dq;
  int64_t lddq;
  float *P, *S;                // [nnz x H], the caller's entry order
  float* part;                 // [long_records(nnz) x pstride]
  int64_t pstride;             // H * F + 2 H rounded up to 4 floats
  const float* bias;           // BIAS kernels only from here: bias[entry * bstride + head * bhs] at the CALLER's entry index (perm)
  int64_t bstride;             // H for a [nnz x H] bias, 1 for a [nnz] one shared by the heads
  int bhs;                     // 1 | 0
  float* dbias;                // [nnz x H], the caller's entry order; null: not asked for
  DropRng rng;                 // DROP kernels only: the seed (device memory), stream id, keep threshold and 1 / keep of the mask
  const float* e;              // EDGE kernels only from here: the entry's row e + entry * lde at the CALLER's entry index (perm)
  int64_t lde;
  float* de;                   // [nnz x ldde], the caller's entry order; null: not asked for
  int64_t ldde;
};

static inline int64_t da_pstride(int H, int F) { return ((int64_t)H * F + 2 * H + 3) & ~(int64_t)3; }

// entries whose k and v rows a lane group has in flight before it folds them (registers: U * VEC * 8).  The forward affords more than
// the backward, which holds q, G and dq of its row besides: at 8 x 64 (two chunks per lane) a build with 4 entries in both was 0.6 ms
// faster in the forward and 1.5 ms slower in the backward than one with 2 in both
__host__ __device__ constexpr int da_unroll(bool bwd, int vec) { return bwd ? (vec == 1 ? 4 : (vec == 2 ? 2 : 1)) : (vec <= 2 ? 4 : 2); }

template <int VEC>
struct DaLane {
  int ofs[VEC];      // float offset of the lane's chunk inside a row (0 when the chunk lies beyond the row)
  int head[VEC];
  unsigned ok;       // bit v: the chunk lies inside the row
  unsigned lead;     // bit v: ... and is the first of its head (the lane that stores the head's scalars)
};

template <int LPR, int VEC>
__device__ __forceinline__ DaLane<VEC> da_lane(const DaArgs& g) {
  DaLane<VEC> ln;
  ln.ok = ln.lead = 0;
  const int c0 = (threadIdx.x & 63) & (LPR - 1);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int c = c0 + 64 * v;
    const bool in = c < g.NCH;
    ln.ofs[v] = in ? 4 * c : 0;
    ln.head[v] = ln.ofs[v] / g.F;
    if (in) ln.ok |= 1u << v;
    if (in && (c & (g.LH - 1)) == 0) ln.lead |= 1u << v;
  }
  return ln;
}

// sum over the lh adjacent lanes of a head (lh a power of two <= LPR): group_sum_rt without the steps a lane shape cannot take
template <int LPR>
__device__ __forceinline__ float da_head_sum(float x, int lh) {
  if constexpr (LPR >= 64) return group_sum_rt(x, lh);
  if constexpr (LPR >= 2) if (lh >= 2) x += dpp_mov<0xB1>(x);
  if constexpr (LPR >= 4) if (lh >= 4) x += dpp_mov<0x4E>(x);
  if constexpr (LPR >= 8) if (lh >= 8) x += dpp_mov<0x141>(x);
  if constexpr (LPR >= 16) if (lh >= 16) x += dpp_mov<0x140>(x);
  if constexpr (LPR >= 32) if (lh >= 32) x += __shfl_xor(x, 16);
  return x;
}

__device__ __forceinline__ float4 da_zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void da_axpy(float4& y, float a, const float4& x) {
  y.x = fmaf(a, x.x, y.x); y.y = fmaf(a, x.y, y.y); y.z = fmaf(a, x.z, y.z); y.w = fmaf(a, x.w, y.w);
}
__device__ __forceinline__ void da_add(float4& y, const float4& x) { y.x += x.x; y.y += x.y; y.z += x.z; y.w += x.w; }
__device__ __forceinline__ void da_scale(float4& y, float a) { y.x *= a; y.y *= a; y.z *= a; y.w *= a; }
__device__ __forceinline__ float4 da_shfl_xor(const float4& x, int off) {
  return make_float4(__shfl_xor(x.x, off), __shfl_xor(x.y, off), __shfl_xor(x.z, off), __shfl_xor(x.w, off));
}

template <int VEC>
__device__ __forceinline__ void da_load_row(const float* p, const DaLane<VEC>& ln, float4 (&w)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) w[v] = ld4(p + ln.ofs[v]);
}
// a bf16 table (the inference forwards of all three families): the same 4 row elements per chunk in one 8-byte load, widened exactly (element 0 is the low half of the first word)
typedef unsigned short da_bf16;
template <int VEC>
__device__ __forceinline__ void da_load_row(const da_bf16* p, const DaLane<VEC>& ln, float4 (&w)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const uint2 r = *reinterpret_cast<const uint2*>(p + ln.ofs[v]);
    w[v] = make_float4(__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                       __uint_as_float(r.y & 0xffff0000u));
  }
}
template <int VEC>
__device__ __forceinline__ void da_store_row(float* p, const DaLane<VEC>& ln, const float4 (&w)[VEC]) {
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (ln.ok >> v & 1) st4(p + ln.ofs[v], w[v]);
}

// the caller's entry index of CSR position pos, without a branch: a pattern without a permutation reads col[pos] in perm's place
// (the line its walk has just asked for) and keeps pos.  As a branch around the load this put an s_waitcnt vmcnt(0) behind every
// gather of the prefetching walk, which then waited for the gather, then for the indices (8 x 16 forward 6.64 ms against 3.68 ms
// without a bias)
// without a bias).  The loaded word is kept as it comes and turned into the index only where it is used, a batch later: taking the
// choice at once made the walk wait for the word, and with it for the gather issued before it
__device__ __forceinline__ int32_t da_eid_raw(const DaArgs& g, int64_t pos) { return (g.perm ? g.perm : g.col)[pos]; }
__device__ __forceinline__ int32_t da_eid(const DaArgs& g, int32_t raw, int64_t pos) { return g.perm ? raw : (int32_t)pos; }
template <int U>
__device__ __forceinline__ void da_eids(const DaArgs& g, const int32_t (&raw)[U], int64_t e, int64_t step, int32_t (&eid)[U]) {
#pragma unroll
  for (int u = 0; u < U; ++u) eid[u] = da_eid(g, raw[u], e + u * step);
}

// BIAS: the per-entry terms of U entries, one 4-byte load per (entry, chunk): every lane of a head asks for the same address, one
// transaction (a lane past the row asks for head 0's)
template <int VEC, int U, bool BIAS>
struct DaBias {
  float b[BIAS ? U : 1][BIAS ? VEC : 1];
};
template <int VEC, int U>
__device__ __forceinline__ void da_bias_load(const DaArgs& g, const DaLane<VEC>& ln, const int32_t (&eid)[U], DaBias<VEC, U, true>& bs) {
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v) bs.b[u][v] = g.bias[(int64_t)eid[u] * g.bstride + ln.head[v] * g.bhs];
}

// online softmax state of one head and the lane's part of its weighted sum, one __expf per (entry, head) (K18's es_fold).
// BIAS: the fold of the score s + b.  The bias goes to the maximum's side of the difference, (s) - (m - b), and leaves the expression
// s - m as it is: under b = 0 both compile to the same operations on the same values (m - 0 is m), whether or not the compiler
// contracts the product inside s into that difference -- it does -- so a bias of zeros changes no bit.
// DROP: (p keep) v goes into acc; z takes p whole: a dropped entry stays in the denominator.  (b, keep: 0 and 1 without the flag)
template <bool BIAS, bool DROP>
__device__ __forceinline__ void da_fold(float& m, float& z, float4& acc, float s, float b, float keep, const float4& w) {
  const float d = BIAS ? s - (m - b) : s - m;
  const float ex = __expf(-fabsf(d));
  const bool up = d > 0.f;
  const float r = up ? ex : 1.f, p = up ? 1.f : ex;
  const float pk = DROP ? p * keep : p;
  z = fmaf(z, r, p);
  acc.x = fmaf(acc.x, r, pk * w.x); acc.y = fmaf(acc.y, r, pk * w.y); acc.z = fmaf(acc.z, r, pk * w.z); acc.w = fmaf(acc.w, r, pk * w.w);
  m = up ? (BIAS ? __fadd_rn(s, b) : s) : m;
}

// DROP (all three families): the key of the row's draws, read once per kernel, and the keep factor (0 or 1 / (1 - p)) of flat mask
// element idx = c(e) H + h
template <bool DROP>
__device__ __forceinline__ uint2 da_key(const DaArgs& g) {
  if constexpr (!DROP) return make_uint2(0u, 0u);
  else {
    const uint64_t seed = *g.rng.seed;
    return make_uint2((uint32_t)seed, (uint32_t)(seed >> 32));
  }
}
__device__ __forceinline__ float da_keep(const DaArgs& g, uint2 key, int64_t idx) {
  const uint64_t q4 = (uint64_t)idx >> 2;
  const uint4 w = philox4x32_10(make_uint4((uint32_t)q4, (uint32_t)(q4 >> 32), g.rng.stream_id, 0xFFFFFFFFu), key);
  return word_of(w, (int)(idx & 3)) < g.rng.thresh ? g.rng.scale : 0.f;
}
// ... of a batch of U entries, base[u] = c(e_u) H.  The LH lanes of a head would all draw the same word for an entry, so they share the
// batch instead: in a round, lane i of the head draws for entry t0 + i, and the head's lanes read each other's factor, one __shfl per
// (entry, chunk): ceil(U / LH) Philox calls per lane and chunk, not U (a lane's place in its head is the same for all its chunks: 64 is
// a multiple of LH; the lanes of a real head are all inside the row).  The rounds are a loop on purpose: unrolled, it is U copies of
// the ten rounds
template <int VEC, int U>
__device__ __forceinline__ void da_keep_batch(const DaArgs& g, const DaLane<VEC>& ln, uint2 key, const int64_t (&base)[U],
                                              float (&keep)[U][VEC]) {
  if constexpr (U == 1) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) keep[0][v] = da_keep(g, key, base[0] + ln.head[v]);
  } else {
    const int li = (threadIdx.x & 63) & (g.LH - 1);
#pragma unroll 1
    for (int t0 = 0; t0 < U; t0 += g.LH) {
      int64_t b = base[U - 1];                                   // (a lane past the batch draws for its last entry; nobody reads it)
#pragma unroll
      for (int u = 0; u < U - 1; ++u) b = t0 + li == u ? base[u] : b;
      float mine[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) mine[v] = da_keep(g, key, b + ln.head[v]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (u >= t0 && u < t0 + g.LH) {
#pragma unroll
          for (int v = 0; v < VEC; ++v) keep[u][v] = __shfl(mine[v], u - t0, g.LH);
        }
    }
  }
}

// (m, z, acc) <- (m, z, acc) (+) (m2, z2, acc2), the earlier entries on the left
__device__ __forceinline__ void da_merge(float& m, float& z, float4& acc, float m2, float z2, const float4& acc2) {
  const float mn = fmaxf(m, m2);
  const float f1 = __expf(m - mn), f2 = __expf(m2 - mn);
  z = z * f1 + z2 * f2;
  acc.x = acc.x * f1 + acc2.x * f2; acc.y = acc.y * f1 + acc2.y * f2; acc.z = acc.z * f1 + acc2.z * f2; acc.w = acc.w * f1 + acc2.w * f2;
  m = mn;
}

// the caller's entry index (x H) of CSR position pos, as the backward without a flag forms it: with the load, no word carried
__device__ __forceinline__ int64_t da_entry(const DaArgs& g, int64_t pos) { return (g.perm ? (int64_t)g.perm[pos] : pos) * g.H; }

template <int VEC>
struct DaState {
  float m[VEC], z[VEC];
  float4 acc[VEC];
};
template <int VEC>
__device__ __forceinline__ void da_init(DaState<VEC>& st) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) { st.m[v] = DA_SEED; st.z[v] = 0.f; st.acc[v] = da_zero4(); }
}

// (LPR, VEC) of a row of H * F floats = nch chunks of 4
static inline void da_pick(int H, int F, int* lpr, int* vec, int* nch) {
  *nch = H * F / 4;
  if (*nch <= 64) {
    int l = 1;
    while (l < *nch) l <<= 1;
    *lpr = l; *vec = 1;
  } else {
    *lpr = 64; *vec = (*nch + 63) / 64;
  }
}

#define PYGAT_DA_DISPATCH(LPRV, VECV, ...)                                  \
  do {                                                                       \
    if ((VECV) == 1) {                                                       \
      switch (LPRV) {                                                        \
        case 1: { constexpr int LPR = 1, VEC = 1; __VA_ARGS__; } break;      \
        case 2: { constexpr int LPR = 2, VEC = 1; __VA_ARGS__; } break;      \
        case 4: { constexpr int LPR = 4, VEC = 1; __VA_ARGS__; } break;      \
        case 8: { constexpr int LPR = 8, VEC = 1; __VA_ARGS__; } break;      \
        case 16: { constexpr int LPR = 16, VEC = 1; __VA_ARGS__; } break;    \
        case 32: { constexpr int LPR = 32, VEC = 1; __VA_ARGS__; } break;    \
        default: { constexpr int LPR = 64, VEC = 1; __VA_ARGS__; } break;    \
      }                                                                      \
    } else if ((VECV) == 2) { constexpr int LPR = 64, VEC = 2; __VA_ARGS__; } \
    else if ((VECV) == 3) { constexpr int LPR = 64, VEC = 3; __VA_ARGS__; }  \
    else { constexpr int LPR = 64, VEC = 4; __VA_ARGS__; }                   \
  } while (0)

// a row table: non-null, aligned to a lane's chunk of 4 elements (16 bytes of floats, 8 of bf16), its stride a multiple of 4 elements
// and at least H x F
#define DA_TABLE_ALIGNED(what, name, ptr, ld, HF, align)                                                               \
  do {                                                                                                                 \
    PYGAT_REQUIRE(ptr, "%s: null %s", what, name);                                                                     \
    PYGAT_REQUIRE((reinterpret_cast<uintptr_t>(ptr) & ((align) - 1u)) == 0, "%s: %s must be %d-byte aligned", what, name, (int)(align)); \
    PYGAT_REQUIRE((ld) >= (HF) && (ld) % 4 == 0, "%s: the row stride of %s, %lld, must be a multiple of 4 and at least H x F = %d", \
                  what, name, (long long)(ld), (int)(HF));                                                             \
  } while (0)
#define DA_TABLE(what, name, ptr, ld, HF) DA_TABLE_ALIGNED(what, name, ptr, ld, HF, 16)

}  // namespace pygat
