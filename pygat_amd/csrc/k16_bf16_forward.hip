// K16 -- the inference forward of the GAT level on a bf16 feature table (gat_level(..., table_dtype=torch.bfloat16), opt-in).
//
// The level is EXACTLY the fp32 level applied to the table Whq = Q(X W), Q = round-to-nearest-even from fp32 to bf16:
//   pack     a row stream over the fp32 projection: Whq_i (uint16, row stride R = H * Fp, padded columns 0) and
//            s_i = Whq_i . a_src from the ROUNDED values, in fp32;
//   forward  K2's nnz split (k2_forward.hip) on the same slot, cut-row and fix-up tables of pygat_graph: a lane group owns a slot
//            of edges, issues U independent row gathers at a time, forms t_j = Whq_j . a_dst from the gathered chunk, folds the
//            edges into the online-softmax state (m, Z, acc) of the current row -- all fp32 -- and writes finished rows; the first /
//            last row of a slot may continue in a neighbour slot, then its state goes to an fp32 partial record and the fix-up
//            launch merges the records of a cut row in slot order.  No LDS, no float atomics: bitwise reproducible.
// What the bf16 table changes is the lane mapping: a lane's gather is one chunk of CW table elements --
//   CW = 8 (16 bytes) for heads of Fp >= 8: a row is R / 8 chunks, the 8 x 16 level takes 16 lanes per row instead of K2's 32 and
//          a wave carries twice as many slots; a chunk never straddles a head, the Fp / 8 lanes of a head are consecutive;
//   CW = 4 (8 bytes) for Fp = 4 (F' <= 4), where 8 elements would span two heads (or, with one head, two rows).
// A pass takes rows of at most 1024 floats (CW = 8: 128 chunks, two per lane) resp. 64 heads of Fp = 4 (one chunk per lane);
// wider levels are walked head window by head window, as K2 does.  No backward exists for this path.
#include "attn_common.h"
#include <string.h>

namespace pygat {

struct BfArgs {
  GraphDev g;
  int H, Fo, Fp, fp_shift;   // heads of THIS pass (a window of the level), true / padded head width
  int R, nch, lph;           // H * Fp; chunks per row = R / CW; lanes per head = max(Fp / CW, 1)
  int64_t ldr, ldh, ldo;     // the level's row strides: R-wide tables (Whq, sk, hattn), per-head tables (s), out
  int64_t ps;                // floats per partial record: [acc R | m H | z H], rounded up to 16 bytes
  float alpha;
  int flags;
  const uint16_t* Whq;
  const float *s, *a_pad, *sk;
  float *out, *hattn, *part;
};

// fp32 -> bf16, round to nearest, ties to even (what v_cvt_pk_bf16_f32 computes), in integer arithmetic; NaN stays NaN
__device__ __forceinline__ uint32_t bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ float bf_leaky(float z, float alpha) { return z > 0.f ? z : alpha * z; }

// ---------------------------------------------------------------- pack: one thread per 4 columns of a row
__global__ __launch_bounds__(256) void bf_pack_kernel(int64_t total, int nch4, int Fo, int Fp, int fp_shift, int lph4, int H,
                                                      const float* __restrict__ Wh, int64_t ldwh, const float* __restrict__ a_pad,
                                                      uint16_t* __restrict__ Whq, float* __restrict__ s) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = q < total;
  const int64_t qc = live ? q : total - 1;       // (whole head groups fall off the end together: total is a multiple of lph4)
  const int64_t row = qc / nch4;
  const int co = 4 * (int)(qc - row * nch4);
  const int h = co >> fp_shift, f0 = co & (Fp - 1);
  const float4 w = ld4(Wh + row * ldwh + co);
  const float in[4] = {w.x, w.y, w.z, w.w};
  uint32_t b[4];
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    b[k] = f0 + k < Fo ? bf16_rne(in[k]) : 0u;     // padded columns of the table are zero
    r[k] = __uint_as_float(b[k] << 16);
  }
  const float4 as = ld4(a_pad + (int64_t)h * 2 * Fp + f0);
  const float sh = group_sum_rt(dot4(make_float4(r[0], r[1], r[2], r[3]), as), lph4);
  if (live) {
    *reinterpret_cast<uint2*>(Whq + row * (int64_t)(4 * nch4) + co) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
    if (f0 == 0) s[row * H + h] = sh;
  }
}

// ---------------------------------------------------------------- forward
template <int VEC>
struct BfCols {
  int cofs[VEC];   // column of the lane's chunk inside a padded row (clamped when invalid)
  int head[VEC];
  bool valid[VEC];
};
template <int CW, int LPR, int VEC>
__device__ __forceinline__ BfCols<VEC> bf_cols(const BfArgs& a) {
  BfCols<VEC> lc;
  const int c0 = (threadIdx.x & 63) & (LPR - 1);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int c = c0 + 64 * v;
    lc.valid[v] = c < a.nch;
    const int cc = lc.valid[v] ? c : 0;
    lc.cofs[v] = CW * cc;
    lc.head[v] = (CW * cc) >> a.fp_shift;
  }
  return lc;
}

template <int CW>
struct BfChunk { uint32_t w[CW / 2]; };
template <int CW>
__device__ __forceinline__ BfChunk<CW> bf_gather(const uint16_t* p) {
  BfChunk<CW> c;
  if constexpr (CW == 8) {
    const uint4 q = *reinterpret_cast<const uint4*>(p);
    c.w[0] = q.x; c.w[1] = q.y; c.w[2] = q.z; c.w[3] = q.w;
  } else {
    const uint2 q = *reinterpret_cast<const uint2*>(p);
    c.w[0] = q.x; c.w[1] = q.y;
  }
  return c;
}
// element 2k in the low half of word k: widening is a shift resp. a mask
template <int CW>
__device__ __forceinline__ void bf_widen(const BfChunk<CW>& c, float* f) {
#pragma unroll
  for (int k = 0; k < CW / 2; ++k) {
    f[2 * k] = __uint_as_float(c.w[k] << 16);
    f[2 * k + 1] = __uint_as_float(c.w[k] & 0xffff0000u);
  }
}

template <int CW, int VEC>
struct BfState {   // online softmax of one row: running max, sum of p, sum of p Whq_j
  float m[VEC], z[VEC];
  float acc[VEC][CW];
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      m[v] = NEG_BIG; z[v] = 0.f;
#pragma unroll
      for (int k = 0; k < CW; ++k) acc[v][k] = 0.f;
    }
  }
};

// fold one edge (logit ev, widened chunk w) into the state: one exp per edge (K2's fold_edge)
template <int CW>
__device__ __forceinline__ void bf_fold(float& m, float& z, float* acc, float ev, const float* w) {
  const float d = ev - m;
  const float ex = __expf(-fabsf(d));
  const bool up = d > 0.f;
  const float sc = up ? ex : 1.f, p = up ? 1.f : ex;
  z = fmaf(z, sc, p);
#pragma unroll
  for (int k = 0; k < CW; ++k) acc[k] = fmaf(acc[k], sc, p * w[k]);
  m = up ? ev : m;
}
template <int CW>
__device__ __forceinline__ void bf_merge(float& m, float& z, float* acc, float m2, float z2, const float* acc2) {
  const float mn = fmaxf(m, m2);
  const float sa = __expf(m - mn), sb = __expf(m2 - mn);
  z = z * sa + z2 * sb;
#pragma unroll
  for (int k = 0; k < CW; ++k) acc[k] = acc[k] * sa + acc2[k] * sb;
  m = mn;
}

// normalise, epilogue (skip, ELU) and stores of a finished row i
template <int CW, int VEC>
__device__ __forceinline__ void bf_finish(const BfArgs& a, const BfCols<VEC>& lc, int i, const BfState<CW, VEC>& st) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (!lc.valid[v]) continue;
    const int co = lc.cofs[v], h = lc.head[v];
    const float rz = 1.0f / st.z[v];
    float hat[CW];
#pragma unroll
    for (int k = 0; k < CW; ++k) hat[k] = st.acc[v][k] * rz;
    if (a.hattn) {
#pragma unroll
      for (int k = 0; k < CW; k += 4) st4(a.hattn + (int64_t)i * a.ldr + co + k, make_float4(hat[k], hat[k + 1], hat[k + 2], hat[k + 3]));
    }
    if (a.out) {
      if (a.flags & PYGAT_F_SKIP) {
#pragma unroll
        for (int k = 0; k < CW; k += 4) {
          const float4 k4 = ld4(a.sk + (int64_t)i * a.ldr + co + k);
          hat[k] += k4.x; hat[k + 1] += k4.y; hat[k + 2] += k4.z; hat[k + 3] += k4.w;
        }
      }
      if (a.flags & PYGAT_F_ELU) {
#pragma unroll
        for (int k = 0; k < CW; ++k) hat[k] = elu1(hat[k]);
      }
      if (a.Fo == a.Fp) {
#pragma unroll
        for (int k = 0; k < CW; k += 4) st4(a.out + (int64_t)i * a.ldo + co + k, make_float4(hat[k], hat[k + 1], hat[k + 2], hat[k + 3]));
      } else {
        const int f0 = co & (a.Fp - 1);
        float* o = a.out + (int64_t)i * a.ldo + (int64_t)h * a.Fo + f0;
#pragma unroll
        for (int k = 0; k < CW; ++k)
          if (f0 + k < a.Fo) o[k] = hat[k];
      }
    }
  }
}

template <int CW, int VEC>
__device__ __forceinline__ void bf_part_store(const BfArgs& a, const BfCols<VEC>& lc, float* p, const BfState<CW, VEC>& st) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (!lc.valid[v]) continue;
#pragma unroll
    for (int k = 0; k < CW; k += 4)
      st4(p + lc.cofs[v] + k, make_float4(st.acc[v][k], st.acc[v][k + 1], st.acc[v][k + 2], st.acc[v][k + 3]));
    if ((lc.cofs[v] & (a.Fp - 1)) == 0) {
      p[a.R + lc.head[v]] = st.m[v];
      p[a.R + a.H + lc.head[v]] = st.z[v];
    }
  }
}
template <int CW, int VEC>
__device__ __forceinline__ void bf_part_load(const BfArgs& a, const BfCols<VEC>& lc, const float* p, BfState<CW, VEC>& r) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    r.m[v] = p[a.R + lc.head[v]];
    r.z[v] = p[a.R + a.H + lc.head[v]];
#pragma unroll
    for (int k = 0; k < CW; k += 4) {
      const float4 q = ld4(p + lc.cofs[v] + k);
      r.acc[v][k] = q.x; r.acc[v][k + 1] = q.y; r.acc[v][k + 2] = q.z; r.acc[v][k + 3] = q.w;
    }
  }
}

// row finished inside the slot -> final stores; row continuing in a neighbour slot -> partial record 2k (head) / 2k + 1 (tail)
template <int CW, int VEC>
__device__ __forceinline__ void bf_flush(const BfArgs& a, const BfCols<VEC>& lc, int64_t k, int i, bool is_head, bool is_tail,
                                         const BfState<CW, VEC>& st) {
  if (is_head || is_tail) bf_part_store<CW, VEC>(a, lc, a.part + (2 * k + (is_head ? 0 : 1)) * a.ps, st);
  else bf_finish<CW, VEC>(a, lc, i, st);
}

template <int CW, int LPR, int VEC>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VEC == 1 ? 4 : 1))) void bf_fwd_kernel(BfArgs a) {
  constexpr int EPW = 64 / LPR;
  constexpr int U = (VEC == 1) ? 4 : 2;      // independent gathers in flight per lane
  const int lane = threadIdx.x & 63;
  const int64_t kl = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (kl >= a.g.kn) return;   // lane groups are independent: no cross-group op below
  const int64_t k = a.g.order ? a.g.order[kl] : kl;
  const SlotView sl = open_slot(a.g, k);
  const int64_t e0 = sl.e0, e1 = sl.e1;
  const int2* __restrict__ rc = a.g.rc;
  const BfCols<VEC> lc = bf_cols<CW, LPR, VEC>(a);
  const int lph = a.lph;
  float adst[VEC][CW];   // this lane's slice of a_dst (zero on invalid chunks; the padded columns of a_pad are zero)
#pragma unroll
  for (int v = 0; v < VEC; ++v)
#pragma unroll
    for (int kk = 0; kk < CW; kk += 4) {
      float4 q = ld4(a.a_pad + (int64_t)lc.head[v] * 2 * a.Fp + a.Fp + (lc.cofs[v] & (a.Fp - 1)) + kk);
      if (!lc.valid[v]) q = make_float4(0.f, 0.f, 0.f, 0.f);
      adst[v][kk] = q.x; adst[v][kk + 1] = q.y; adst[v][kk + 2] = q.z; adst[v][kk + 3] = q.w;
    }
  int cur = sl.r_first;
  BfState<CW, VEC> st;
  st.reset();
  for (int64_t e = e0; e < e1; e += U) {
    int2 p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = rc[(e + u < e1) ? e + u : e1 - 1];
    __builtin_amdgcn_sched_barrier(0);   // all U edge records are issued before the first one is used (k2_forward.hip)
    BfChunk<CW> wq[U][VEC];
    float sv[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        wq[u][v] = bf_gather<CW>(a.Whq + (int64_t)p[u].y * a.ldr + lc.cofs[v]);
        sv[u][v] = a.s[(int64_t)p[u].x * a.ldh + lc.head[v]];
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float w[VEC][CW], tv[VEC];
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        bf_widen<CW>(wq[u][v], w[v]);
        float d = 0.f;
#pragma unroll
        for (int kk = 0; kk < CW; ++kk) d = fmaf(w[v][kk], adst[v][kk], d);
        tv[v] = group_sum_rt(d, lph);   // t_j of the head, in every lane of it (all lanes of the group are active here)
      }
      if (e + u < e1) {
        if (p[u].x != cur) {
          bf_flush<CW, VEC>(a, lc, k, cur, slot_head_partial(sl, cur), false, st);
          cur = p[u].x;
          st.reset();
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) bf_fold<CW>(st.m[v], st.z[v], st.acc[v], bf_leaky(sv[u][v] + tv[v], a.alpha), w[v]);
      }
    }
  }
  bf_flush<CW, VEC>(a, lc, k, cur, slot_head_partial(sl, cur), slot_tail_partial(a.g, sl, cur), st);
}

// Merge of one cut row by one wave: its pieces tail(k), head(k + 1), ..., head(k + npieces - 1) are dealt round-robin to the
// 64 / LPR lane groups (PF pieces in flight each) and combined with shuffles, always in the same order.
template <int CW, int LPR, int VEC>
__device__ __forceinline__ void bf_merge_row(const BfArgs& a, const BfCols<VEC>& lc, int64_t k, int r, int npieces) {
  constexpr int G = 64 / LPR;
  constexpr int PF = (VEC == 1) ? 4 : 2;
  const int g = (threadIdx.x & 63) / LPR;
  BfState<CW, VEC> st;
  st.reset();
  for (int q = g; q < npieces; q += G * PF) {
    BfState<CW, VEC> rec[PF];
#pragma unroll
    for (int f = 0; f < PF; ++f) {
      const int qq = q + f * G;
      const int qc = qq < npieces ? qq : q;   // clamped: the loads stay unconditional
      bf_part_load<CW, VEC>(a, lc, a.part + piece_record(k, qc) * a.ps, rec[f]);
    }
#pragma unroll
    for (int f = 0; f < PF; ++f)
      if (q + f * G < npieces) {
#pragma unroll
        for (int v = 0; v < VEC; ++v) bf_merge<CW>(st.m[v], st.z[v], st.acc[v], rec[f].m[v], rec[f].z[v], rec[f].acc[v]);
      }
  }
#pragma unroll
  for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float mo = __shfl_xor(st.m[v], off), zo = __shfl_xor(st.z[v], off);
      float ao[CW];
#pragma unroll
      for (int kk = 0; kk < CW; ++kk) ao[kk] = __shfl_xor(st.acc[v][kk], off);
      bf_merge<CW>(st.m[v], st.z[v], st.acc[v], mo, zo, ao);
    }
  }
  if (g == 0 && npieces > 0) bf_finish<CW, VEC>(a, lc, r, st);
}

// Fix-up of the rows cut by a slot border, one wave per row of the graph's cut-row list (longest chains first); without a
// list a wave screens FIX_SCREEN consecutive slots -- slot k OWNS a cut row if its last row starts inside k and continues
// beyond -- and merges the rows they own in turn.
template <int CW, int LPR, int VEC>
__global__ __launch_bounds__(256) void bf_fixup_kernel(BfArgs a) {
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const BfCols<VEC> lc = bf_cols<CW, LPR, VEC>(a);
  if (a.g.cut) {
    if (wv >= a.g.n_cut) return;   // (wave-uniform)
    bf_merge_row<CW, LPR, VEC>(a, lc, a.g.cut[3 * wv], a.g.cut[3 * wv + 1], a.g.cut[3 * wv + 2]);
    return;
  }
  screen_cut_rows(a.g, wv * FIX_SCREEN, a.g.kn, [&](int64_t k, int r, int npieces) { bf_merge_row<CW, LPR, VEC>(a, lc, k, r, npieces); });
}

// lane shapes: CW = 8 -> (LPR, 1) for LPR = 1 .. 64 and (64, 2); CW = 4 -> (LPR, 1)
#define PYGAT_BF_DISPATCH(CWV, LPRV, VECV, CALL)                                 \
  do {                                                                           \
    if ((CWV) == 4) {                                                            \
      switch (LPRV) {                                                            \
        case 1: { constexpr int CW = 4, LPR = 1, VEC = 1; CALL; } break;         \
        case 2: { constexpr int CW = 4, LPR = 2, VEC = 1; CALL; } break;         \
        case 4: { constexpr int CW = 4, LPR = 4, VEC = 1; CALL; } break;         \
        case 8: { constexpr int CW = 4, LPR = 8, VEC = 1; CALL; } break;         \
        case 16: { constexpr int CW = 4, LPR = 16, VEC = 1; CALL; } break;       \
        case 32: { constexpr int CW = 4, LPR = 32, VEC = 1; CALL; } break;       \
        default: { constexpr int CW = 4, LPR = 64, VEC = 1; CALL; } break;       \
      }                                                                          \
    } else if ((VECV) == 2) { constexpr int CW = 8, LPR = 64, VEC = 2; CALL;     \
    } else {                                                                     \
      switch (LPRV) {                                                            \
        case 1: { constexpr int CW = 8, LPR = 1, VEC = 1; CALL; } break;         \
        case 2: { constexpr int CW = 8, LPR = 2, VEC = 1; CALL; } break;         \
        case 4: { constexpr int CW = 8, LPR = 4, VEC = 1; CALL; } break;         \
        case 8: { constexpr int CW = 8, LPR = 8, VEC = 1; CALL; } break;         \
        case 16: { constexpr int CW = 8, LPR = 16, VEC = 1; CALL; } break;       \
        case 32: { constexpr int CW = 8, LPR = 32, VEC = 1; CALL; } break;       \
        default: { constexpr int CW = 8, LPR = 64, VEC = 1; CALL; } break;       \
      }                                                                          \
    }                                                                            \
  } while (0)

static inline int bf_chunk_width(int Fp) { return Fp >= 8 ? 8 : 4; }
// heads one pass takes: rows of 1024 floats (head_group_fwd), and one chunk per lane at Fp = 4
static inline int bf_head_cap(int H, int Fp) { return Fp >= 8 ? head_group_fwd(H, Fp) : (H < 64 ? H : 64); }
static inline int64_t bf_part_stride(int H, int Fp) { return (int64_t)H * Fp + ((2 * H + 3) & ~3); }
static inline void bf_pick_lanes(int nch, int* lpr, int* vec) {
  if (nch <= 64) {
    int l = 1;
    while (l < nch) l <<= 1;
    *lpr = l; *vec = 1;
  } else {
    *lpr = 64; *vec = 2;
  }
}

// pygat_kernel_footprint: k16_pack, k16_{fwd,fix}_c<CW>l<LPR>v<VEC> (the lane shapes of PYGAT_BF_DISPATCH)
int footprint_k16(const char* name, int* regs, int* scratch) {
  const void* fn = nullptr;
  if (!strcmp(name, "k16_pack")) {
    fn = reinterpret_cast<const void*>(&bf_pack_kernel);
  } else {
    char kind[8] = "";
    int cw = 0, lpr = 0, vec = 0;
    if (sscanf(name, "k16_%3[a-z]_c%dl%dv%d", kind, &cw, &lpr, &vec) == 4 && (cw == 4 || cw == 8) && lpr >= 1 && lpr <= 64 &&
        (lpr & (lpr - 1)) == 0 && (vec == 1 || (vec == 2 && cw == 8 && lpr == 64))) {
      if (!strcmp(kind, "fwd")) PYGAT_BF_DISPATCH(cw, lpr, vec, fn = reinterpret_cast<const void*>(&bf_fwd_kernel<CW, LPR, VEC>));
      else if (!strcmp(kind, "fix")) PYGAT_BF_DISPATCH(cw, lpr, vec, fn = reinterpret_cast<const void*>(&bf_fixup_kernel<CW, LPR, VEC>));
    }
  }
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k16_pack, k16_{fwd,fix}_c<CW>l<LPR>v<VEC>)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_gat_bf16_workspace_bytes(int64_t nnz, int slot_edges, int H, int Fo, size_t* bytes) {
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(bytes, "gat_bf16_workspace_bytes: null bytes");
  PYGAT_REQUIRE(nnz > 0 && slot_edges >= 4 && (slot_edges & 3) == 0 && H > 0 && Fp > 0,
                "gat_bf16_workspace_bytes: nnz=%lld, slot_edges=%d, H=%d or F'=%d out of range", (long long)nnz, slot_edges, H, Fo);
  // two records (head piece, tail piece) per slot, sized for the widest head window = the whole level
  *bytes = (size_t)(2 * cdiv(nnz, slot_edges)) * (size_t)bf_part_stride(H, Fp) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_gat_pack_bf16(int n, int H, int Fo, const float* Wh, int64_t ldwh, const float* a_pad, void* Whq, float* s,
                                   void* stream) {
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(Wh && a_pad && Whq && s, "gat_pack_bf16: null Wh / a_pad / Whq / s");
  PYGAT_REQUIRE(n > 0 && H > 0, "gat_pack_bf16: n=%d rows, H=%d heads", n, H);
  PYGAT_REQUIRE(Fp > 0, "gat_pack_bf16: head width F'=%d outside [1, 256]", Fo);
  const int64_t R = (int64_t)H * Fp, total = (int64_t)n * (R / 4);
  PYGAT_REQUIRE(ldwh >= R && (ldwh & 3) == 0, "gat_pack_bf16: ldwh=%lld: rows of Wh are H x padded F' = %lld floats and 16-byte multiples",
                (long long)ldwh, (long long)R);
  PYGAT_REQUIRE(aligned16(Wh) && aligned16(Whq) && aligned16(a_pad), "gat_pack_bf16: Wh, a_pad and the bf16 table must be 16-byte aligned");
  PYGAT_REQUIRE(cdiv(total, 256) < ((int64_t)1 << 31), "gat_pack_bf16: table too wide for one pass: %d rows of %lld columns", n, (long long)R);
  hipLaunchKernelGGL(bf_pack_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, total, (int)(R / 4), Fo, Fp,
                     ilog2(Fp), Fp / 4, H, Wh, ldwh, a_pad, static_cast<uint16_t*>(Whq), s);
  PYGAT_CHECK_LAUNCH("gat_pack_bf16");
  return PYGAT_OK;
}

extern "C" int pygat_gat_forward_bf16(const pygat_graph* g, int H, int Fo, float alpha, int flags, const void* Whq, const float* s,
                                      const float* a_pad, const float* sk, float* out, float* hattn, int head_group, void* part,
                                      void* stream) {
  PYGAT_REQUIRE(g, "gat_forward_bf16: null graph");
  PYGAT_REQUIRE(!g->user_row, "gat_forward_bf16: a graph with a row map (pygat_graph.user_row) is not supported: this path writes row i");
  PYGAT_REQUIRE(g->slot_count == 0, "gat_forward_bf16: a slot range is not supported");
  PYGAT_REQUIRE(Whq && s && a_pad && part, "gat_forward_bf16: null Whq / s / a_pad / part");
  PYGAT_REQUIRE(out || hattn, "gat_forward_bf16: need out and/or hattn");
  PYGAT_REQUIRE((flags & ~(PYGAT_F_ELU | PYGAT_F_SKIP)) == 0, "gat_forward_bf16: flags %d: PYGAT_F_ELU and PYGAT_F_SKIP only", flags);
  PYGAT_REQUIRE(!(flags & PYGAT_F_SKIP) || sk, "gat_forward_bf16: PYGAT_F_SKIP without sk");
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(H > 0, "gat_forward_bf16: H=%d heads", H);
  PYGAT_REQUIRE(Fp > 0, "gat_forward_bf16: head width F'=%d outside [1, 256]", Fo);
  const int cap = bf_head_cap(H, Fp);
  PYGAT_REQUIRE(head_group >= 0 && head_group <= cap,
                "gat_forward_bf16: head_group=%d: a pass takes at most %d heads of padded width %d (rows of 1024 floats; 64 heads at width 4)",
                head_group, cap, Fp);
  PYGAT_REQUIRE(aligned16(Whq) && aligned16(part) && aligned16(a_pad) && (!sk || aligned16(sk)) && (!hattn || aligned16(hattn)) &&
                    (!out || Fo != Fp || aligned16(out)),
                "gat_forward_bf16: the bf16 table and the row tables must be 16-byte aligned");
  BfArgs a;
  const int rc = check_graph(g, &a.g, 0);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int CWv = bf_chunk_width(Fp);
  const int hg = head_group > 0 ? (head_group < H ? head_group : H) : (cap < H ? cap : H);
  const int64_t nslots = a.g.kn;
  for (int h0 = 0; h0 < H; h0 += hg) {
    const int hc = (H - h0 < hg) ? H - h0 : hg;
    a.H = hc; a.Fo = Fo; a.Fp = Fp; a.fp_shift = ilog2(Fp);
    a.R = hc * Fp; a.nch = a.R / CWv; a.lph = Fp / CWv > 1 ? Fp / CWv : 1;
    a.ldr = (int64_t)H * Fp; a.ldh = H; a.ldo = (int64_t)H * Fo;
    a.ps = bf_part_stride(hc, Fp);
    a.alpha = alpha; a.flags = flags;
    a.Whq = static_cast<const uint16_t*>(Whq) + (int64_t)h0 * Fp;
    a.s = s + h0;
    a.a_pad = a_pad + (int64_t)h0 * 2 * Fp;
    a.sk = sk ? sk + (int64_t)h0 * Fp : nullptr;
    a.out = out ? out + (int64_t)h0 * Fo : nullptr;
    a.hattn = hattn ? hattn + (int64_t)h0 * Fp : nullptr;
    a.part = static_cast<float*>(part);   // reused by the windows: the launches are ordered on the stream
    int lpr, vec;
    bf_pick_lanes(a.nch, &lpr, &vec);
    const MainGrid mg = main_grid(nslots, lpr, vec);
    PYGAT_BF_DISPATCH(CWv, lpr, vec, hipLaunchKernelGGL((bf_fwd_kernel<CW, LPR, VEC>), dim3(mg.blocks), dim3(mg.bt), 0, st, a));
    PYGAT_CHECK_LAUNCH("gat_forward_bf16");
    const FixGrid fg = fixup_grid(a.g, lpr, /*wave_rows=*/true);   // a wave per list entry, or per FIX_SCREEN slots
    if (fg.blocks == 0) continue;
    PYGAT_BF_DISPATCH(CWv, lpr, vec, hipLaunchKernelGGL((bf_fixup_kernel<CW, LPR, VEC>), dim3(fg.blocks), dim3(64 * fg.waves), 0, st, a));
    PYGAT_CHECK_LAUNCH("gat_forward_bf16_fixup");
  }
  return PYGAT_OK;
}
