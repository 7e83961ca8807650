// K13 -- the attention coefficients of a level, alpha_ij = exp(e_ij - m_i) / Z_i, as an [E x H] table (opt-in:
// gat_level(..., return_attention=True)).  K2 keeps no per-edge intermediates (online softmax); this pass recomputes the
// logits from the tables the forward left (Wh / WW, s, a, m, Z) and writes one coefficient per edge and head, in the
// edge order of the CALLER's pattern:
//   reference layers.py:41-43   attention (dense layer)          -> attention[adj > 0]
//             layers.py:144-150 edge_e / e_rowsum[edge[0]]       (SpGraphAttentionLayer)
//             layers.py:283-290 the same for SpGraphAttentionLayerV2
// The level may have run in an internal node order (CSRGraph.degree_ordered): `map` (caller node -> table row) is then
// applied to both ends of every edge.  There is no reduction across edges, so the work is spread over edges, not rows --
// a lane group per row would serialise the 26 779-edge hub of the R-MAT graph.  A row with exactly one edge has alpha = 1
// and none of its tables is read (the self-loop-only tail: its Wh rows may be unwritten, its m / Z hold fill values).
// The logits are formed with the operations and lane order of K2 (dot4 per 16-byte chunk, DPP sums over the lanes of a
// head), so e_ij -- and with it exp(e_ij - m_i) -- is the value K2 normalised by.
#include "attn_common.h"

namespace pygat {

__device__ __forceinline__ float lrelu13(float z, float alpha) { return z > 0.f ? z : alpha * z; }

// t_q = Wh_q . a_dst per head, rows q < t_rows: one 16-byte chunk per lane, Fp / 4 consecutive lanes per head (K2's lanes)
__global__ __launch_bounds__(256) void att_t_kernel(int64_t chunks, int R4, int H, int Fp, int lph, const float* __restrict__ Wh,
                                                    int64_t ldwh, const float* __restrict__ a_pad, float* __restrict__ t) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = c < chunks;            // whole head groups are live or not (chunks is a multiple of lph): no early exit
  const int64_t cc = live ? c : 0;         // before the lane sums
  const int64_t q = cc / R4;
  const int co = 4 * (int)(cc % R4), h = co / Fp, f0 = co & (Fp - 1);
  const float4 w = ld4(Wh + q * ldwh + co);
  const float4 ad = ld4(a_pad + (int64_t)h * 2 * Fp + Fp + f0);
  const float v = group_sum_rt(dot4(w, ad), lph);
  if (live && f0 == 0) t[q * H + h] = v;
}

// one thread per edge, all heads: alpha = exp(LeakyReLU(s_i + t_j) - m_i) / Z_i
template <bool H4>
__global__ __launch_bounds__(256) void att_v1_kernel(int64_t nnz, int H, float alpha, const int32_t* __restrict__ rowptr,
                                                     const int2* __restrict__ rc, const int32_t* __restrict__ map,
                                                     const float* __restrict__ s, const float* __restrict__ t,
                                                     const float* __restrict__ m, const float* __restrict__ Z,
                                                     float* __restrict__ att) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const int2 p = rc[e];
  float* o = att + e * H;
  if (rowptr[p.x + 1] - rowptr[p.x] == 1) {
    if constexpr (H4) {
      for (int h = 0; h < H; h += 4) st4(o + h, make_float4(1.f, 1.f, 1.f, 1.f));
    } else {
      for (int h = 0; h < H; ++h) o[h] = 1.f;
    }
    return;
  }
  const int64_t qi = map ? (int64_t)map[p.x] : (int64_t)p.x, qj = map ? (int64_t)map[p.y] : (int64_t)p.y;
  if constexpr (H4) {
    for (int h = 0; h < H; h += 4) {
      const float4 sv = ld4(s + qi * H + h), tv = ld4(t + qj * H + h);
      const float4 mv = ld4(m + qi * H + h), zv = ld4(Z + qi * H + h);
      st4(o + h, make_float4(__expf(lrelu13(sv.x + tv.x, alpha) - mv.x) / zv.x, __expf(lrelu13(sv.y + tv.y, alpha) - mv.y) / zv.y,
                             __expf(lrelu13(sv.z + tv.z, alpha) - mv.z) / zv.z, __expf(lrelu13(sv.w + tv.w, alpha) - mv.w) / zv.w));
    }
  } else {
    for (int h = 0; h < H; ++h)
      o[h] = __expf(lrelu13(s[qi * H + h] + t[qj * H + h], alpha) - m[qi * H + h]) / Z[qi * H + h];
  }
}

// GATv2: e_ij = a . LeakyReLU(Whi_i + Whj_j) per head needs the whole F'-vector of the edge.  K2's lane mapping (LPR lanes
// per edge, VEC chunks per lane, per-head DPP sums); a lane group walks EPG consecutive edges, gathers Whj_j per edge and
// keeps the Whi_i row, m_i and Z_i of the current row in registers (loaded again only when the row changes).
template <int LPR, int VEC, int EPG>
__global__ __launch_bounds__(256) void att_v2_kernel(int64_t nnz, RowShape rs, float alpha, const int32_t* __restrict__ rowptr,
                                                     const int2* __restrict__ rc, const int32_t* __restrict__ map,
                                                     const float* __restrict__ WW, const float* __restrict__ a2,
                                                     const float* __restrict__ m, const float* __restrict__ Z,
                                                     float* __restrict__ att) {
  constexpr int U = VEC == 1 ? 4 : 2;
  const int lane = threadIdx.x & 63;
  const int64_t grp = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 / LPR) + lane / LPR;
  const int64_t e0 = grp * EPG;
  if (e0 >= nnz) return;                   // lane groups are independent: no cross-group op below
  const int64_t e1 = e0 + EPG < nnz ? e0 + EPG : nnz;
  const LaneCols<VEC> lc = lane_cols<LPR, VEC>(rs);
  const int R = rs.R, H = rs.H, lph = rs.lph < 64 ? rs.lph : 64;
  const int64_t ldw = 2 * (int64_t)R;
  float4 av[VEC];
  bool lead[VEC];
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    av[v] = ld4(a2 + (int64_t)lc.head[v] * rs.Fp + (lc.cofs[v] & (rs.Fp - 1)));
    if (!lc.valid[v]) av[v] = make_float4(0.f, 0.f, 0.f, 0.f);
    lead[v] = lc.valid[v] && (lc.cofs[v] & (rs.Fp - 1)) == 0;
  }
  int cur = -1;
  bool single = false;
  float4 wi[VEC];
  float mr[VEC], zr[VEC];
  for (int64_t e = e0; e < e1; e += U) {
    int2 p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) p[u] = rc[(e + u < e1) ? e + u : e1 - 1];
    float4 wj[U][VEC];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t qj = map ? (int64_t)map[p[u].y] : (int64_t)p[u].y;
#pragma unroll
      for (int v = 0; v < VEC; ++v) wj[u][v] = ld4(WW + qj * ldw + R + lc.cofs[v]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (e + u >= e1) break;              // (uniform in the lane group)
      if (p[u].x != cur) {
        cur = p[u].x;
        single = rowptr[cur + 1] - rowptr[cur] == 1;
        if (!single) {
          const int64_t qi = map ? (int64_t)map[cur] : (int64_t)cur;
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            wi[v] = ld4(WW + qi * ldw + lc.cofs[v]);
            mr[v] = m[qi * H + lc.head[v]];
            zr[v] = Z[qi * H + lc.head[v]];
          }
        }
      }
      float* o = att + (e + u) * H;
      if (single) {
#pragma unroll
        for (int v = 0; v < VEC; ++v)
          if (lead[v]) o[lc.head[v]] = 1.f;
        continue;
      }
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        const float4 hh = make_float4(wi[v].x + wj[u][v].x, wi[v].y + wj[u][v].y, wi[v].z + wj[u][v].z, wi[v].w + wj[u][v].w);
        const float4 ll = make_float4(lrelu13(hh.x, alpha), lrelu13(hh.y, alpha), lrelu13(hh.z, alpha), lrelu13(hh.w, alpha));
        const float ev = group_sum_rt(dot4(ll, av[v]), lph);
        if (lead[v]) o[lc.head[v]] = __expf(ev - mr[v]) / zr[v];
      }
    }
  }
}

static int check_pattern(const char* what, int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo,
                         const float* m, const float* Z, float* att) {
  PYGAT_REQUIRE(n > 0 && nnz > 0 && H > 0, "%s: empty pattern or no heads (n=%d nnz=%lld H=%d)", what, n, (long long)nnz, H);
  PYGAT_REQUIRE(nnz < ((int64_t)1 << 31), "%s: nnz %lld exceeds int32 edge indexing", what, (long long)nnz);
  PYGAT_REQUIRE(padded_width(Fo) > 0, "%s: F'=%d outside [1, 256]", what, Fo);
  PYGAT_REQUIRE(rowptr && edge_rc && m && Z && att, "%s: null rowptr / edge_rc / m / Z / att", what);
  PYGAT_REQUIRE(aligned16(m) && aligned16(Z) && aligned16(att) && ((uintptr_t)edge_rc & 7u) == 0,
                "%s: m, Z and att must be 16-byte aligned, edge_rc 8-byte aligned", what);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_gat_attention(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                                   int H, int Fo, float alpha, const float* Wh, int64_t ldwh, const float* s, const float* a_pad,
                                   const float* m, const float* Z, int t_rows, float* t, float* att, void* stream) {
  const int rc = check_pattern("gat_attention", n, nnz, rowptr, edge_rc, H, Fo, m, Z, att);
  if (rc != PYGAT_OK) return rc;
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(Wh && s && a_pad && t, "gat_attention: null Wh / s / a_pad / t");
  PYGAT_REQUIRE(ldwh >= (int64_t)H * Fp && (ldwh % 4) == 0 && aligned16(Wh) && aligned16(a_pad) && aligned16(s) && aligned16(t),
                "gat_attention: Wh (ld %lld, need >= %d and a multiple of 4), s, a_pad and t must be 16-byte aligned", (long long)ldwh,
                H * Fp);
  PYGAT_REQUIRE(t_rows >= 0 && t_rows <= n, "gat_attention: t_rows=%d outside [0, n=%d]", t_rows, n);
  hipStream_t st = (hipStream_t)stream;
  if (t_rows > 0) {
    const int R4 = H * Fp / 4;
    const int64_t chunks = (int64_t)t_rows * R4;
    const int lph = Fp / 4 < 64 ? Fp / 4 : 64;
    hipLaunchKernelGGL(att_t_kernel, dim3((unsigned)cdiv(chunks, 256)), dim3(256), 0, st, chunks, R4, H, Fp, lph, Wh, ldwh, a_pad, t);
    PYGAT_CHECK_LAUNCH("gat_attention (t)");
  }
  const dim3 grid((unsigned)cdiv(nnz, 256));
  const int2* rc2 = reinterpret_cast<const int2*>(edge_rc);
  if ((H % 4) == 0)
    hipLaunchKernelGGL(att_v1_kernel<true>, grid, dim3(256), 0, st, nnz, H, alpha, rowptr, rc2, to_internal, s, t, m, Z, att);
  else
    hipLaunchKernelGGL(att_v1_kernel<false>, grid, dim3(256), 0, st, nnz, H, alpha, rowptr, rc2, to_internal, s, t, m, Z, att);
  PYGAT_CHECK_LAUNCH("gat_attention");
  return PYGAT_OK;
}

extern "C" int pygat_gatv2_attention(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                                     int H, int Fo, float alpha, const float* WW, const float* a2, const float* m, const float* Z,
                                     float* att, void* stream) {
  const int rc = check_pattern("gatv2_attention", n, nnz, rowptr, edge_rc, H, Fo, m, Z, att);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(WW && a2 && aligned16(WW) && aligned16(a2), "gatv2_attention: WW and a2 must be non-null and 16-byte aligned");
  RowShape rs;
  PYGAT_REQUIRE(make_row_shape(H, Fo, &rs), "gatv2_attention: row too wide: H x padded F' = %d x %d > 1024", H, padded_width(Fo));
  int lpr, vec;
  pick_lanes(rs, &lpr, &vec);
  constexpr int EPG = 16;
  const int64_t groups = cdiv(nnz, EPG);
  const int64_t blocks = cdiv(groups, 4 * (64 / lpr));
  const int2* rc2 = reinterpret_cast<const int2*>(edge_rc);
  PYGAT_DISPATCH_LANES(lpr, vec,
                       hipLaunchKernelGGL((att_v2_kernel<LPR, VEC, EPG>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                                          nnz, rs, alpha, rowptr, rc2, to_internal, WW, a2, m, Z, att));
  PYGAT_CHECK_LAUNCH("gatv2_attention");
  return PYGAT_OK;
}
