// K15 -- the GAT level with a per-edge logit term (gat_level(..., edge_logit=u), opt-in).  u [E x H] in the CALLER's edge order
// enters the score in front of the LeakyReLU,
//   z_ij = (s_i + t_j) + u_ij,  e_ij = LeakyReLU(z_ij),  att_ij = exp(e_ij - m_i) / Z_i,  h'_i = sum_j att_ij Wh_j,
// and the backward hands back du_ij = dz_ij = l_ij att_ij (dp_ij - D_i), the per-edge quantity the plain backward sums away
// (dp_ij = Gp_i . Wh_j per head, D_i = Gp_i . h'_i, l_ij = z_ij > 0 ? 1 : slope).  Three passes share one skeleton:
//   forward   walks the rows of the pattern: online softmax over (m, Z, sum p Wh_j), u read as a consecutive stream;
//   rows      walks them again: Gp_i and D_i from (G, out, h'_i), du_ij written per edge, ds_i = sum_j du_ij;
//   cols      walks the TRANSPOSED pattern: dt_j = sum_i du_ij (du and u of transposed edge k at row perm_t[k]),
//             dWh_j = sum_i att_ij Gp_i + ds_j a_src + dt_j a_dst, att recomputed from (s_i, m_i, Z_i, t_j, u_ij).
// Lane mapping of attn_common.h: a group of LPR lanes holds one row (VEC 16-byte chunks per lane), the lanes of a head are
// consecutive, the per-head dot products are DPP sums.  A long row (column) goes through partial records (the rule of
// long_rows.h), one wave per chunk: its 64 / LPR lane groups walk the piece of a long row edge-interleaved and are merged in a
// fixed butterfly; a record is [R sums | m | Z], merged by el_merge.  No float atomics, every sum in a fixed order: the same bits.
// A row with exactly one edge has att = 1: its u is never read, its du is exactly 0; the forward marks it with Z = 0 for later passes.
#include "attn_common.h"
#include "long_rows.h"
#include <string.h>

namespace pygat {

enum { EL_FWD = 0, EL_ROWS = 1, EL_COLS = 2 };

struct ElArgs {
  int n, concat;
  int64_t nnz;
  float slope, inv_h;
  RowShape rs;
  const int32_t* rowptr;       // the walked pattern: forward, or transposed (cols)
  const int2* rc;              // (owner, other end) per walked edge
  const int32_t* perm;         // cols: walked edge -> row of u / du
  const float *Wh, *sk, *a_pad;
  const float *s, *t, *m, *Z;  // node tables [n x H]
  const float* u;              // [nnz x H]
  const float *G, *y, *hat;    // rows: dL/dout, the saved output (concat), h' [n x R]
  const float *Gp_in, *du_in, *ds_in;   // cols
  float *out, *hattn, *mo, *Zo;         // forward
  float *Gp, *du, *ds;                  // rows
  float *dt, *dWh;                      // cols
  float* part;                          // [long_records(nnz) x pstride]: R sums, then H maxima, then H scalar sums
  int64_t pstride;
};

static inline int64_t el_pstride(int H, int Fp) { return (int64_t)H * Fp + ((2 * H + 3) & ~3); }

template <int VEC>
struct ElState {   // forward: running max, sum of p, sum of p Wh_j; rows: z = sum dz; cols: z = sum du, a = sum att Gp_i
  float m[VEC], z[VEC];
  float4 a[VEC];
};
template <int VEC>
struct ElOwner {   // what a lane keeps of the row (column) it works for: forward s_i; rows s_i, m_i, Z_i, D_i, Gp_i; cols t_j
  float s[VEC], m[VEC], z[VEC], d[VEC];
  float4 g[VEC];
};

__device__ __forceinline__ float el_leaky(float z, float slope) { return z > 0.f ? z : slope * z; }
__device__ __forceinline__ float4 el_axpy(float p, float4 w, float4 a) {
  return make_float4(fmaf(p, w.x, a.x), fmaf(p, w.y, a.y), fmaf(p, w.z, a.z), fmaf(p, w.w, a.w));
}
__device__ __forceinline__ float4 el_scale(float4 a, float f) { return make_float4(a.x * f, a.y * f, a.z * f, a.w * f); }

template <int OP, int VEC>
__device__ __forceinline__ void el_init(ElState<VEC>& st) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    st.m[v] = OP == EL_FWD ? NEG_BIG : 0.f;
    st.z[v] = 0.f;
    st.a[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// st <- st (+) o, the earlier edges on the left
template <int OP, int VEC>
__device__ __forceinline__ void el_merge(ElState<VEC>& st, const ElState<VEC>& o) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if constexpr (OP == EL_FWD) {
      const float mn = fmaxf(st.m[v], o.m[v]);
      const float f1 = __expf(st.m[v] - mn), f2 = __expf(o.m[v] - mn);
      st.z[v] = st.z[v] * f1 + o.z[v] * f2;
      st.a[v] = el_axpy(f2, o.a[v], el_scale(st.a[v], f1));
      st.m[v] = mn;
    } else {
      st.z[v] += o.z[v];
      if constexpr (OP == EL_COLS) st.a[v] = el_axpy(1.f, o.a[v], st.a[v]);
    }
  }
}

// Gp chunk of a row: dL/d(h'_i + skip_i) -- through the ELU of a concat level (from its saved output), G / H of a head mean
template <int VEC>
__device__ __forceinline__ float4 el_gp_chunk(const ElArgs& g, const LaneCols<VEC>& lc, int v, int64_t row) {
  const int f0 = lc.cofs[v] & (g.rs.Fp - 1), h = lc.head[v];
  float r[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int f = f0 + k;
    float x = 0.f;
    if (lc.valid[v] && f < g.rs.Fo) {
      if (g.concat) {
        const int64_t q = row * g.rs.ldo + (int64_t)h * g.rs.Fo + f;
        const float yv = g.y[q];
        x = g.G[q] * (yv > 0.f ? 1.f : yv + 1.f);
      } else {
        x = g.G[row * g.rs.Fo + f] * g.inv_h;
      }
    }
    r[k] = x;
  }
  return make_float4(r[0], r[1], r[2], r[3]);
}

template <int OP, int VEC>
__device__ __forceinline__ void el_load_owner(const ElArgs& g, const LaneCols<VEC>& lc, int64_t row, int lph, ElOwner<VEC>& o) {
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int64_t qh = row * g.rs.H + lc.head[v];
    o.m[v] = 0.f; o.z[v] = 0.f; o.d[v] = 0.f;
    o.g[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (OP == EL_COLS) {
      o.s[v] = g.t[qh];
    } else {
      o.s[v] = g.s[qh];
    }
    if constexpr (OP == EL_ROWS) {
      o.m[v] = g.m[qh]; o.z[v] = g.Z[qh];
      o.g[v] = el_gp_chunk<VEC>(g, lc, v, row);
      const float4 hv = ld4(g.hat + row * g.rs.R + lc.cofs[v]);
      o.d[v] = group_sum_rt(lc.valid[v] ? dot4(o.g[v], hv) : 0.f, lph);
    }
  }
}

// one walked edge, all heads of the lane group
template <int OP, int VEC>
__device__ __forceinline__ void el_edge(const ElArgs& g, const LaneCols<VEC>& lc, const ElOwner<VEC>& o, int64_t e, int lph,
                                        ElState<VEC>& st) {
  const int H = g.rs.H;
  const int64_t other = g.rc[e].y;
  if constexpr (OP == EL_FWD) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float4 w = ld4(g.Wh + other * g.rs.R + lc.cofs[v]);
      const float z = (o.s[v] + g.t[other * H + lc.head[v]]) + g.u[e * H + lc.head[v]];
      const float ev = el_leaky(z, g.slope);
      const float mn = fmaxf(st.m[v], ev);
      const float f = __expf(st.m[v] - mn), p = __expf(ev - mn);
      st.z[v] = st.z[v] * f + p;
      st.a[v] = el_axpy(p, w, el_scale(st.a[v], f));
      st.m[v] = mn;
    }
  } else if constexpr (OP == EL_ROWS) {
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const float4 w = ld4(g.Wh + other * g.rs.R + lc.cofs[v]);
      const float dp = group_sum_rt(lc.valid[v] ? dot4(o.g[v], w) : 0.f, lph);
      const float z = (o.s[v] + g.t[other * H + lc.head[v]]) + g.u[e * H + lc.head[v]];
      const float al = __expf(el_leaky(z, g.slope) - o.m[v]) / o.z[v];
      const float dz = (z > 0.f ? 1.f : g.slope) * al * (dp - o.d[v]);
      if (lc.valid[v] && (lc.cofs[v] & (g.rs.Fp - 1)) == 0) g.du[e * H + lc.head[v]] = dz;
      st.z[v] += dz;
    }
  } else {
    const int64_t fe = g.perm[e];
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      const int64_t qh = other * H + lc.head[v];
      const float Zi = g.Z[qh];
      float al = 1.f;                                  // a single-edge row: a constant, its u and du are not read
      if (Zi != 0.f) {
        const float z = (g.s[qh] + o.s[v]) + g.u[fe * H + lc.head[v]];
        al = __expf(el_leaky(z, g.slope) - g.m[qh]) / Zi;
        st.z[v] += g.du_in[fe * H + lc.head[v]];
      }
      st.a[v] = el_axpy(al, ld4(g.Gp_in + other * g.rs.R + lc.cofs[v]), st.a[v]);
    }
  }
}

// launch 1: one wave per chunk of walked edges; the piece of every long row inside the chunk -> one partial record
template <int OP, int LPR, int VEC>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void el_long_kernel(ElArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(g.rs);
  const int lph = g.rs.lph < 64 ? g.rs.lph : 64;
  for_long_rows(g.rowptr, g.rc[ch.c0].x, g.rc[ch.c1 - 1].x, ch, [&](int r, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    ElOwner<VEC> own;
    el_load_owner<OP, VEC>(g, lc, r, lph, own);
    ElState<VEC> st;
    el_init<OP, VEC>(st);
    for (int64_t e = e0 + grp; e < e1; e += EPW) el_edge<OP, VEC>(g, lc, own, e, lph, st);
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1) {         // lane groups of the wave, a fixed butterfly
      ElState<VEC> o;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        o.m[v] = __shfl_xor(st.m[v], off); o.z[v] = __shfl_xor(st.z[v], off);
        o.a[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (OP != EL_ROWS)
          o.a[v] = make_float4(__shfl_xor(st.a[v].x, off), __shfl_xor(st.a[v].y, off), __shfl_xor(st.a[v].z, off),
                               __shfl_xor(st.a[v].w, off));
      }
      el_merge<OP, VEC>(st, o);
    }
    if (grp == 0) {
      float* p = g.part + long_record(blockIdx.x, slot) * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        if (!lc.valid[v]) continue;
        if constexpr (OP != EL_ROWS) st4(p + lc.cofs[v], st.a[v]);
        if ((lc.cofs[v] & (g.rs.Fp - 1)) == 0) {
          p[g.rs.R + lc.head[v]] = st.m[v];
          p[g.rs.R + g.rs.H + lc.head[v]] = st.z[v];
        }
      }
    }
  });
}

// launch 2: one lane group per row (column)
template <int OP, int LPR, int VEC>
__global__ __launch_bounds__(256) void el_row_kernel(ElArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (row >= g.n) return;                              // (whole lane groups; nothing below crosses a group)
  const RowShape& rs = g.rs;
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(rs);
  const int lph = rs.lph < 64 ? rs.lph : 64, H = rs.H;
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1], deg = end - start;
  ElOwner<VEC> own;
  el_load_owner<OP, VEC>(g, lc, row, lph, own);
  ElState<VEC> st;
  el_init<OP, VEC>(st);
  const bool single = OP != EL_COLS && deg == 1;       // att = 1: u is not read
  if (deg > LONG_ROW) {
    for_long_records(start, end, [&](int64_t rec) {
      const float* p = g.part + rec * g.pstride;
      ElState<VEC> o;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        o.a[v] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (OP != EL_ROWS) o.a[v] = ld4(p + lc.cofs[v]);
        o.m[v] = p[rs.R + lc.head[v]];
        o.z[v] = p[rs.R + H + lc.head[v]];
      }
      el_merge<OP, VEC>(st, o);
    });
  } else if (!single) {
    for (int64_t e = start; e < end; ++e) el_edge<OP, VEC>(g, lc, own, e, lph, st);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    if (!lc.valid[v]) continue;
    const int f0 = lc.cofs[v] & (rs.Fp - 1), h = lc.head[v];
    const bool lead = f0 == 0;
    if constexpr (OP == EL_FWD) {
      float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
      float mz = 0.f, zz = 0.f;                        // (m, Z) = (0, 0): a row of at most one edge
      if (single) {
        hv = ld4(g.Wh + (int64_t)g.rc[start].y * rs.R + lc.cofs[v]);
      } else if (deg > 1) {
        hv = el_scale(st.a[v], 1.f / st.z[v]);
        mz = st.m[v]; zz = st.z[v];
      }
      float hr[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (f0 + k >= rs.Fo) hr[k] = 0.f;
      st4(g.hattn + row * rs.R + lc.cofs[v], make_float4(hr[0], hr[1], hr[2], hr[3]));
      if (lead) { g.mo[row * H + h] = mz; g.Zo[row * H + h] = zz; }
      if (g.concat) {
        float sr[4] = {0.f, 0.f, 0.f, 0.f};
        if (g.sk) { const float4 sv = ld4(g.sk + row * rs.R + lc.cofs[v]); sr[0] = sv.x; sr[1] = sv.y; sr[2] = sv.z; sr[3] = sv.w; }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (f0 + k < rs.Fo) g.out[row * rs.ldo + (int64_t)h * rs.Fo + f0 + k] = elu1(hr[k] + sr[k]);
      }
    } else if constexpr (OP == EL_ROWS) {
      st4(g.Gp + row * rs.R + lc.cofs[v], own.g[v]);
      if (lead) {
        g.ds[row * H + h] = deg > 1 ? st.z[v] : 0.f;
        if (single) g.du[start * H + h] = 0.f;
      }
    } else {
      const float dsv = g.ds_in[row * H + h], dtv = st.z[v];
      const float4 as = ld4(g.a_pad + (int64_t)h * 2 * rs.Fp + f0), ad = ld4(g.a_pad + (int64_t)h * 2 * rs.Fp + rs.Fp + f0);
      st4(g.dWh + row * rs.R + lc.cofs[v], el_axpy(dtv, ad, el_axpy(dsv, as, st.a[v])));
      if (lead) g.dt[row * H + h] = dtv;
    }
  }
}

// the coefficients themselves (return_attention=True): one thread per (edge, head), m and Z as the forward left them
__global__ __launch_bounds__(256) void el_att_kernel(int64_t total, int H, float slope, const int2* __restrict__ rc,
                                                     const float* __restrict__ s, const float* __restrict__ t,
                                                     const float* __restrict__ m, const float* __restrict__ Z,
                                                     const float* __restrict__ u, float* __restrict__ att) {
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= total) return;
  const int64_t e = q / H;
  const int h = (int)(q - e * H);
  const int2 p = rc[e];
  const float Zi = Z[(int64_t)p.x * H + h];
  float al = 1.f;
  if (Zi != 0.f) {
    const float z = (s[(int64_t)p.x * H + h] + t[(int64_t)p.y * H + h]) + u[q];
    al = __expf(el_leaky(z, slope) - m[(int64_t)p.x * H + h]) / Zi;
  }
  att[q] = al;
}

template <int OP, bool LONG>
static const void* el_kernel_ptr(int lpr, int vec) {
  const void* f = nullptr;
  PYGAT_DISPATCH_LANES(lpr, vec, f = LONG ? reinterpret_cast<const void*>(&el_long_kernel<OP, LPR, VEC>)
                                          : reinterpret_cast<const void*>(&el_row_kernel<OP, LPR, VEC>));
  return f;
}

template <int OP>
static void el_launch(const ElArgs& g, hipStream_t st) {
  int lpr, vec;
  pick_lanes(g.rs, &lpr, &vec);
  const unsigned chunks = (unsigned)long_chunks(g.nnz);
  const unsigned blocks = (unsigned)cdiv(g.n, 4 * (64 / lpr));
  PYGAT_DISPATCH_LANES(lpr, vec, hipLaunchKernelGGL((el_long_kernel<OP, LPR, VEC>), dim3(chunks), dim3(64), 0, st, g));
  PYGAT_DISPATCH_LANES(lpr, vec, hipLaunchKernelGGL((el_row_kernel<OP, LPR, VEC>), dim3(blocks), dim3(256), 0, st, g));
}

// pygat_kernel_footprint: k15_att, k15_{fwd,rows,cols}_{long,row}_l<LPR>v<VEC> (the lane shapes of PYGAT_DISPATCH_LANES)
int footprint_k15(const char* name, int* regs, int* scratch) {
  const void* fn = nullptr;
  if (!strcmp(name, "k15_att")) {
    fn = reinterpret_cast<const void*>(&el_att_kernel);
  } else {
    char op[8] = "", kind[8] = "";
    int lpr = 0, vec = 0;
    if (sscanf(name, "k15_%4[a-z]_%4[a-z]_l%dv%d", op, kind, &lpr, &vec) == 4 && lpr >= 1 && lpr <= 64 && (lpr & (lpr - 1)) == 0 &&
        vec >= 1 && vec <= 4 && (vec == 1 || lpr == 64) && (!strcmp(kind, "long") || !strcmp(kind, "row"))) {
      const bool lng = !strcmp(kind, "long");
      if (!strcmp(op, "fwd")) fn = lng ? el_kernel_ptr<EL_FWD, true>(lpr, vec) : el_kernel_ptr<EL_FWD, false>(lpr, vec);
      else if (!strcmp(op, "rows")) fn = lng ? el_kernel_ptr<EL_ROWS, true>(lpr, vec) : el_kernel_ptr<EL_ROWS, false>(lpr, vec);
      else if (!strcmp(op, "cols")) fn = lng ? el_kernel_ptr<EL_COLS, true>(lpr, vec) : el_kernel_ptr<EL_COLS, false>(lpr, vec);
    }
  }
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k15_att, k15_{fwd,rows,cols}_{long,row}_l<LPR>v<VEC>)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

static int el_check(const char* what, int n, int64_t nnz, int64_t u_rows, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo,
                    const float* u, const void* ws, RowShape* rs) {
  PYGAT_REQUIRE(n > 0 && nnz > 0, "%s: empty pattern (n=%d nnz=%lld)", what, n, (long long)nnz);
  PYGAT_REQUIRE(nnz < ((int64_t)1 << 31), "%s: nnz %lld exceeds int32 edge indexing", what, (long long)nnz);
  PYGAT_REQUIRE(H > 0, "%s: H=%d heads", what, H);
  PYGAT_REQUIRE(padded_width(Fo) > 0, "%s: F'=%d outside [1, 256]", what, Fo);
  PYGAT_REQUIRE(make_row_shape(H, Fo, rs), "%s: row too wide: H x padded F' = %d x %d > 1024", what, H, padded_width(Fo));
  PYGAT_REQUIRE(u, "%s: null u (the edge logits, [nnz x H])", what);
  PYGAT_REQUIRE(u_rows == nnz, "%s: u has %lld rows but the pattern has nnz = %lld edges", what, (long long)u_rows, (long long)nnz);
  PYGAT_REQUIRE(rowptr && edge_rc && ws, "%s: null rowptr / edge_rc / workspace", what);
  PYGAT_REQUIRE(((uintptr_t)edge_rc & 7u) == 0 && aligned16(ws), "%s: edge_rc must be 8-byte, the workspace 16-byte aligned", what);
  return PYGAT_OK;
}

static void el_common(ElArgs& g, int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const RowShape& rs, float alpha,
                      int flags, void* ws) {
  memset(&g, 0, sizeof(g));
  g.n = n; g.nnz = nnz; g.rs = rs; g.slope = alpha; g.concat = (flags & PYGAT_F_ELU) ? 1 : 0; g.inv_h = 1.f / (float)rs.H;
  g.rowptr = rowptr; g.rc = reinterpret_cast<const int2*>(edge_rc);
  g.part = static_cast<float*>(ws); g.pstride = el_pstride(rs.H, rs.Fp);
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_gat_edge_workspace_bytes(int64_t nnz, int H, int Fo, size_t* bytes) {
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(bytes, "gat_edge_workspace_bytes: null bytes");
  PYGAT_REQUIRE(nnz > 0 && H > 0 && Fp > 0, "gat_edge_workspace_bytes: nnz=%lld, H=%d or F'=%d out of range", (long long)nnz, H, Fo);
  *bytes = (size_t)(long_records(nnz) * el_pstride(H, Fp)) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_gat_edge_forward(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo, float alpha,
                                      int flags, const float* Wh, const float* s, const float* t, const float* sk, const float* u,
                                      int64_t u_rows, float* out, float* hattn, float* m, float* Z, void* ws, void* stream) {
  RowShape rs;
  const int rc = el_check("gat_edge_forward", n, nnz, u_rows, rowptr, edge_rc, H, Fo, u, ws, &rs);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(Wh && s && t && hattn && m && Z, "gat_edge_forward: null Wh / s / t / hattn / m / Z");
  PYGAT_REQUIRE((flags & ~(PYGAT_F_ELU | PYGAT_F_SKIP)) == 0, "gat_edge_forward: flags %d: PYGAT_F_ELU and PYGAT_F_SKIP only", flags);
  PYGAT_REQUIRE(!(flags & PYGAT_F_ELU) || out, "gat_edge_forward: PYGAT_F_ELU (a concat level) needs out");
  PYGAT_REQUIRE(!(flags & PYGAT_F_SKIP) || sk, "gat_edge_forward: PYGAT_F_SKIP needs sk");
  PYGAT_REQUIRE(aligned16(Wh) && aligned16(hattn) && (!sk || aligned16(sk)), "gat_edge_forward: Wh, sk and hattn must be 16-byte aligned");
  ElArgs g;
  el_common(g, n, nnz, rowptr, edge_rc, rs, alpha, flags, ws);
  g.Wh = Wh; g.s = s; g.t = t; g.sk = (flags & PYGAT_F_SKIP) ? sk : nullptr; g.u = u;
  g.out = out; g.hattn = hattn; g.mo = m; g.Zo = Z;
  el_launch<EL_FWD>(g, (hipStream_t)stream);
  PYGAT_CHECK_LAUNCH("gat_edge_forward");
  return PYGAT_OK;
}

extern "C" int pygat_gat_edge_alpha(int n, int64_t nnz, const int32_t* edge_rc, int H, float alpha, const float* s, const float* t,
                                        const float* m, const float* Z, const float* u, int64_t u_rows, float* att, void* stream) {
  PYGAT_REQUIRE(n > 0 && nnz > 0 && H > 0, "gat_edge_alpha: empty pattern or no heads (n=%d nnz=%lld H=%d)", n, (long long)nnz, H);
  PYGAT_REQUIRE(nnz < ((int64_t)1 << 31), "gat_edge_alpha: nnz %lld exceeds int32 edge indexing", (long long)nnz);
  PYGAT_REQUIRE(u, "gat_edge_alpha: null u (the edge logits, [nnz x H])");
  PYGAT_REQUIRE(u_rows == nnz, "gat_edge_alpha: u has %lld rows but the pattern has nnz = %lld edges", (long long)u_rows, (long long)nnz);
  PYGAT_REQUIRE(edge_rc && s && t && m && Z && att && ((uintptr_t)edge_rc & 7u) == 0,
                "gat_edge_alpha: null edge_rc / s / t / m / Z / att, or edge_rc not 8-byte aligned");
  const int64_t total = nnz * H;
  hipLaunchKernelGGL(el_att_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, total, H, alpha,
                     reinterpret_cast<const int2*>(edge_rc), s, t, m, Z, u, att);
  PYGAT_CHECK_LAUNCH("gat_edge_alpha");
  return PYGAT_OK;
}

extern "C" int pygat_gat_edge_backward_rows(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo, float alpha,
                                            int flags, const float* Wh, const float* s, const float* t, const float* m, const float* Z,
                                            const float* u, int64_t u_rows, const float* G, const float* y, const float* hattn,
                                            float* Gp, float* du, float* ds, void* ws, void* stream) {
  RowShape rs;
  const int rc = el_check("gat_edge_backward_rows", n, nnz, u_rows, rowptr, edge_rc, H, Fo, u, ws, &rs);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(Wh && s && t && m && Z && G && hattn && Gp && du && ds, "gat_edge_backward_rows: null Wh / s / t / m / Z / G / hattn / Gp / du / ds");
  PYGAT_REQUIRE(!(flags & PYGAT_F_ELU) || y, "gat_edge_backward_rows: PYGAT_F_ELU (a concat level) needs its saved output y");
  PYGAT_REQUIRE(aligned16(Wh) && aligned16(hattn) && aligned16(Gp), "gat_edge_backward_rows: Wh, hattn and Gp must be 16-byte aligned");
  ElArgs g;
  el_common(g, n, nnz, rowptr, edge_rc, rs, alpha, flags, ws);
  g.Wh = Wh; g.s = s; g.t = t; g.m = m; g.Z = Z; g.u = u; g.G = G; g.y = y; g.hat = hattn;
  g.Gp = Gp; g.du = du; g.ds = ds;
  el_launch<EL_ROWS>(g, (hipStream_t)stream);
  PYGAT_CHECK_LAUNCH("gat_edge_backward_rows");
  return PYGAT_OK;
}

extern "C" int pygat_gat_edge_backward_cols(int n, int64_t nnz, const int32_t* rowptr_t, const int32_t* edge_rc_t, const int32_t* perm_t,
                                            int H, int Fo, float alpha, const float* s, const float* t, const float* m, const float* Z,
                                            const float* u, int64_t u_rows, const float* Gp, const float* du, const float* ds,
                                            const float* a_pad, float* dt, float* dWh, void* ws, void* stream) {
  RowShape rs;
  const int rc = el_check("gat_edge_backward_cols", n, nnz, u_rows, rowptr_t, edge_rc_t, H, Fo, u, ws, &rs);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(perm_t && s && t && m && Z && Gp && du && ds && a_pad && dt && dWh,
                "gat_edge_backward_cols: null perm_t / s / t / m / Z / Gp / du / ds / a_pad / dt / dWh");
  PYGAT_REQUIRE(aligned16(Gp) && aligned16(a_pad) && aligned16(dWh), "gat_edge_backward_cols: Gp, a_pad and dWh must be 16-byte aligned");
  ElArgs g;
  el_common(g, n, nnz, rowptr_t, edge_rc_t, rs, alpha, 0, ws);
  g.perm = perm_t; g.s = s; g.t = t; g.m = m; g.Z = Z; g.u = u; g.Gp_in = Gp; g.du_in = du; g.ds_in = ds; g.a_pad = a_pad;
  g.dt = dt; g.dWh = dWh;
  el_launch<EL_COLS>(g, (hipStream_t)stream);
  PYGAT_CHECK_LAUNCH("gat_edge_backward_cols");
  return PYGAT_OK;
}
