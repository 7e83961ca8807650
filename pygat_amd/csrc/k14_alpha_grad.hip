// K14 -- the gradient of a loss through the attention coefficients of a GAT level (gat_level(..., return_attention="grad")).
// With A = dL/d alpha [E x H] in the CALLER's edge order, z_ij = s_i + t_j, alpha_ij = exp(LeakyReLU(z_ij) - m_i) / Z_i and
// l_ij = (z_ij > 0 ? 1 : slope):
//   c_i   = sum_k alpha_ik A_ik
//   dz_ij = l_ij alpha_ij (A_ij - c_i)
//   ds'_i = sum_j dz_ij = P_i - c_i Q_i,  P_i = sum_j l_ij alpha_ij A_ij,  Q_i = sum_j l_ij alpha_ij     (row pass, ONE sweep)
//   dt'_j = sum_i dz_ij                                                                                 (column pass)
// (autograd of reference layers.py:144-150, edge_e / e_rowsum).  alpha is recomputed from (s_i, t_j, m_i, Z_i) with the
// expression of K13's att_v1_kernel, so it is the coefficient the caller was handed.  The level's tables may be in an
// internal node order: `map` (caller node -> table row) is applied to both ends of every edge, as K13 does.
//
// Work split.  One WAVE per row (column): its lanes cover (edge, head) pairs -- lane l works on head l % H, so the [E x H]
// gradient is read in consecutive floats -- and the lanes of a head are summed in a fixed order.  A long row (R-MAT: up to
// 26 779 edges) goes through partial records (the rule of long_rows.h), four waves per chunk: they walk the piece of a long row
// edge-interleaved and are added through LDS in wave order; a record is three sums per head, and records add.  No float atomics,
// every sum in a fixed order: two runs give the same bits.  A row with exactly one edge has alpha = 1, a constant: it contributes
// exactly zero and neither its tables nor its rows of A are read (the row pass marks it with Z = 0, the column pass tests that).
#include "long_rows.h"

namespace pygat {

__device__ __forceinline__ float lrelu14(float z, float alpha) { return z > 0.f ? z : alpha * z; }

struct AlphaGradArgs {
  int n, H, G;                 // G: lanes of a wave that work (the largest multiple of H <= 64)
  int64_t nnz;
  float slope;
  const int32_t* rowptr;       // the walked pattern: forward (row pass) or transposed (column pass)
  const int2* rc;              // (owner, other end) per edge of that pattern
  const int32_t* perm;         // column pass: walked edge -> row of A (forward edge)
  const int32_t* map;          // caller node -> table row, or NULL
  const float *s, *m, *Z, *t;  // node tables [n x H]
  const float* A;              // dL/d alpha [nnz x H]
  float* rec;                  // [n x H x 4] = (s, m, Z, c) per node and head; Z = 0: a row that contributes nothing
  float* out;                  // ds' (row pass) / dt' (column pass), [n x H]
  float* part;                 // [long_records(nnz) x H x 3]
};

// what a lane keeps of the row (column) it works for, for its head
struct Owner {
  float a, b, c;               // row pass: s_i, m_i, Z_i; column pass: t_j
};

template <bool COL>
__device__ __forceinline__ Owner load_owner(const AlphaGradArgs& g, int64_t q, int h) {
  Owner o;
  if constexpr (COL) {
    o.a = g.t[q * g.H + h]; o.b = 0.f; o.c = 0.f;
  } else {
    o.a = g.s[q * g.H + h]; o.b = g.m[q * g.H + h]; o.c = g.Z[q * g.H + h];
  }
  return o;
}

// one (edge, head): row pass acc = (sum alpha A, sum l alpha A, sum l alpha); column pass acc.x = sum l alpha (A - c)
template <bool COL>
__device__ __forceinline__ void add_edge(const AlphaGradArgs& g, int64_t e, int h, const Owner& o, float3& acc) {
  const int other = g.rc[e].y;
  const int64_t q = g.map ? (int64_t)g.map[other] : (int64_t)other;
  if constexpr (COL) {
    const float4 r = ld4(g.rec + (q * g.H + h) * 4);
    if (r.z == 0.f) return;                                  // a single-edge row: its A is not read
    const float av = g.A[(int64_t)g.perm[e] * g.H + h];
    const float z = r.x + o.a;
    const float al = __expf(lrelu14(z, g.slope) - r.y) / r.z;
    const float l = z > 0.f ? 1.f : g.slope;
    acc.x += l * al * (av - r.w);
  } else {
    const float av = g.A[e * g.H + h];
    const float z = o.a + g.t[q * g.H + h];
    const float al = __expf(lrelu14(z, g.slope) - o.b) / o.c;
    const float l = z > 0.f ? 1.f : g.slope;
    acc.x += al * av;
    acc.y += l * al * av;
    acc.z += l * al;
  }
}

// Sum over the lanes l < G of a wave with equal l % H; every such lane ends with the total.  All 64 lanes call it.
__device__ __forceinline__ float head_sum(float v, int lane, int H, int G) {
  if ((H & (H - 1)) == 0) {                                  // G = 64: a butterfly over the lane bits above the head's
    for (int o = 32; o >= H; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  float tot = 0.f;
  const int h = lane % H;
  for (int k = 0; k * H < G; ++k) tot += __shfl(v, h + k * H);
  return tot;
}

// launch 1: per chunk, the partial sums of every long row over its edges inside the chunk; the four waves find the same rows
template <bool COL>
__global__ __launch_bounds__(256) void alpha_grad_long_kernel(AlphaGradArgs g) {
  __shared__ float red[4][64][3];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const int H = g.H, h = lane % H;
  const int64_t step = 4 * (g.G / H);
  for_long_rows(g.rowptr, g.rc[ch.c0].x, g.rc[ch.c1 - 1].x, ch, [&](int r, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    float3 acc = make_float3(0.f, 0.f, 0.f);
    if (lane < g.G) {
      const Owner o = load_owner<COL>(g, g.map ? (int64_t)g.map[r] : (int64_t)r, h);
      for (int64_t e = e0 + (wv * g.G + lane) / H; e < e1; e += step) add_edge<COL>(g, e, h, o, acc);
    }
    acc.x = head_sum(acc.x, lane, H, g.G);
    if constexpr (!COL) {
      acc.y = head_sum(acc.y, lane, H, g.G);
      acc.z = head_sum(acc.z, lane, H, g.G);
    }
    if (lane < H) { red[wv][lane][0] = acc.x; red[wv][lane][1] = acc.y; red[wv][lane][2] = acc.z; }
    __syncthreads();
    if (tid < H) {
      float* p = g.part + (long_record(blockIdx.x, slot) * H + tid) * 3;
      for (int c = 0; c < 3; ++c) p[c] = ((red[0][tid][c] + red[1][tid][c]) + red[2][tid][c]) + red[3][tid][c];
    }
    __syncthreads();
  });
}

// launch 2: one wave per row (column)
template <bool COL>
__global__ __launch_bounds__(256) void alpha_grad_wave_kernel(AlphaGradArgs g) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= g.n) return;                                      // (a whole wave)
  const int H = g.H, h = lane % H;
  const int64_t start = g.rowptr[i], end = g.rowptr[i + 1];
  const int64_t q = g.map ? (int64_t)g.map[i] : i;
  if (!COL && end - start <= 1) {                            // alpha = 1 (or no edge): a constant, nothing is read
    if (lane < H) {
      st4(g.rec + (q * H + lane) * 4, make_float4(0.f, 0.f, 0.f, 0.f));
      g.out[q * H + lane] = 0.f;
    }
    return;
  }
  float3 acc = make_float3(0.f, 0.f, 0.f);
  Owner o;
  o.a = o.b = o.c = 0.f;
  if (end - start > LONG_ROW) {
    if (lane < H) {
      if constexpr (!COL) o = load_owner<COL>(g, q, h);
      for_long_records(start, end, [&](int64_t rec) {
        const float* p = g.part + (rec * H + lane) * 3;
        acc.x += p[0]; acc.y += p[1]; acc.z += p[2];
      });
    }
  } else {
    if (lane < g.G && end > start) {
      o = load_owner<COL>(g, q, h);
      for (int64_t e = start + lane / H; e < end; e += g.G / H) add_edge<COL>(g, e, h, o, acc);
    }
    acc.x = head_sum(acc.x, lane, H, g.G);
    if constexpr (!COL) {
      acc.y = head_sum(acc.y, lane, H, g.G);
      acc.z = head_sum(acc.z, lane, H, g.G);
    }
  }
  if (lane >= H) return;
  if constexpr (COL) {
    g.out[q * H + lane] = acc.x;
  } else {
    st4(g.rec + (q * H + lane) * 4, make_float4(o.a, o.b, o.c, acc.x));
    g.out[q * H + lane] = acc.y - acc.x * acc.z;
  }
}

// dWh_q += ds'_q a_src + dt'_q a_dst, one 16-byte chunk per thread
__global__ __launch_bounds__(256) void alpha_grad_apply_kernel(int64_t chunks, int R4, int H, int Fp, const float* __restrict__ a_pad,
                                                               const float* __restrict__ ds2, const float* __restrict__ dt2,
                                                               float* __restrict__ dWh) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= chunks) return;
  const int64_t q = c / R4;
  const int co = 4 * (int)(c % R4), h = co / Fp, f0 = co & (Fp - 1);
  const float4 as = ld4(a_pad + (int64_t)h * 2 * Fp + f0), ad = ld4(a_pad + (int64_t)h * 2 * Fp + Fp + f0);
  const float u = ds2[q * H + h], v = dt2[q * H + h];
  float* p = dWh + q * (int64_t)(4 * R4) + co;
  float4 w = ld4(p);
  w.x += u * as.x + v * ad.x; w.y += u * as.y + v * ad.y; w.z += u * as.z + v * ad.z; w.w += u * as.w + v * ad.w;
  st4(p, w);
}

static int check_common(const char* what, int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, int H, int Fo,
                        const float* A, const float* rec, const float* out, const char* out_name, const float* part) {
  PYGAT_REQUIRE(n > 0 && nnz > 0 && H > 0, "%s: empty pattern or no heads (n=%d nnz=%lld H=%d)", what, n, (long long)nnz, H);
  PYGAT_REQUIRE(H <= 64, "%s: H=%d heads, at most 64 (a wave's lanes cover the heads)", what, H);
  PYGAT_REQUIRE(nnz < ((int64_t)1 << 31), "%s: nnz %lld exceeds int32 edge indexing", what, (long long)nnz);
  PYGAT_REQUIRE(padded_width(Fo) > 0, "%s: F'=%d outside [1, 256]", what, Fo);
  PYGAT_REQUIRE(rowptr && edge_rc && A && rec && out && part, "%s: null rowptr / edge_rc / A / rec / %s / part", what, out_name);
  PYGAT_REQUIRE(aligned16(A) && aligned16(rec) && ((uintptr_t)edge_rc & 7u) == 0,
                "%s: A and rec must be 16-byte aligned, edge_rc 8-byte aligned", what);
  return PYGAT_OK;
}

template <bool COL>
static void launch_passes(const AlphaGradArgs& g, hipStream_t st) {
  hipLaunchKernelGGL(alpha_grad_long_kernel<COL>, dim3((unsigned)long_chunks(g.nnz)), dim3(256), 0, st, g);
  hipLaunchKernelGGL(alpha_grad_wave_kernel<COL>, dim3((unsigned)cdiv(g.n, 4)), dim3(256), 0, st, g);
}

// register / scratch footprint as the loaded code object reports it (pygat_kernel_footprint): 0 / 1 = the long-row launch of
// the row / column pass, 2 / 3 = their wave-per-row launch, 4 = the dWh stream
int footprint_k14(int which, int* regs, int* scratch) {
  const void* fn = which == 0   ? reinterpret_cast<const void*>(&alpha_grad_long_kernel<false>)
                   : which == 1 ? reinterpret_cast<const void*>(&alpha_grad_long_kernel<true>)
                   : which == 2 ? reinterpret_cast<const void*>(&alpha_grad_wave_kernel<false>)
                   : which == 3 ? reinterpret_cast<const void*>(&alpha_grad_wave_kernel<true>)
                                : reinterpret_cast<const void*>(&alpha_grad_apply_kernel);
  return kernel_footprint_of(fn, regs, scratch);
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_alpha_grad_workspace_bytes(int64_t nnz, int H, size_t* bytes) {
  PYGAT_REQUIRE(bytes && nnz > 0 && H > 0 && H <= 64, "alpha_grad_workspace_bytes: null bytes, or nnz=%lld / H=%d out of range", (long long)nnz, H);
  *bytes = (size_t)(long_records(nnz) * H * 3) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_alpha_grad_rows(int n, int64_t nnz, const int32_t* rowptr, const int32_t* edge_rc, const int32_t* to_internal,
                                     int H, int Fo, float alpha, const float* s, const float* t, const float* m, const float* Z,
                                     const float* A, float* rec, float* ds2, float* part, void* stream) {
  const int rc = check_common("alpha_grad_rows", n, nnz, rowptr, edge_rc, H, Fo, A, rec, ds2, "ds2", part);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(s && t && m && Z, "alpha_grad_rows: null s / t / m / Z");
  AlphaGradArgs g;
  g.n = n; g.H = H; g.G = 64 - 64 % H; g.nnz = nnz; g.slope = alpha;
  g.rowptr = rowptr; g.rc = reinterpret_cast<const int2*>(edge_rc); g.perm = nullptr; g.map = to_internal;
  g.s = s; g.m = m; g.Z = Z; g.t = t; g.A = A; g.rec = rec; g.out = ds2; g.part = part;
  launch_passes<false>(g, (hipStream_t)stream);
  PYGAT_CHECK_LAUNCH("alpha_grad_rows");
  return PYGAT_OK;
}

extern "C" int pygat_alpha_grad_cols(int n, int64_t nnz, const int32_t* rowptr_t, const int32_t* edge_rc_t, const int32_t* perm_t,
                                     const int32_t* to_internal, int H, int Fo, float alpha, const float* t, const float* rec,
                                     const float* A, float* dt2, float* part, void* stream) {
  const int rc = check_common("alpha_grad_cols", n, nnz, rowptr_t, edge_rc_t, H, Fo, A, rec, dt2, "dt2", part);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(perm_t && t, "alpha_grad_cols: null perm_t / t");
  AlphaGradArgs g;
  g.n = n; g.H = H; g.G = 64 - 64 % H; g.nnz = nnz; g.slope = alpha;
  g.rowptr = rowptr_t; g.rc = reinterpret_cast<const int2*>(edge_rc_t); g.perm = perm_t; g.map = to_internal;
  g.s = nullptr; g.m = nullptr; g.Z = nullptr; g.t = t; g.A = A; g.rec = const_cast<float*>(rec); g.out = dt2; g.part = part;
  launch_passes<true>(g, (hipStream_t)stream);
  PYGAT_CHECK_LAUNCH("alpha_grad_cols");
  return PYGAT_OK;
}

extern "C" int pygat_alpha_grad_apply(int n_rows, int H, int Fo, const float* a_pad, const float* ds2, const float* dt2, float* dWh,
                                      void* stream) {
  const int Fp = padded_width(Fo);
  PYGAT_REQUIRE(n_rows > 0 && H > 0 && Fp > 0, "alpha_grad_apply: no rows, no heads or F' outside [1, 256] (n_rows=%d H=%d F'=%d)",
                n_rows, H, Fo);
  PYGAT_REQUIRE(a_pad && ds2 && dt2 && dWh && aligned16(a_pad) && aligned16(dWh),
                "alpha_grad_apply: a_pad, ds2, dt2 and dWh must be non-null, a_pad and dWh 16-byte aligned");
  const int R4 = H * Fp / 4;
  const int64_t chunks = (int64_t)n_rows * R4;
  hipLaunchKernelGGL(alpha_grad_apply_kernel, dim3((unsigned)cdiv(chunks, 256)), dim3(256), 0, (hipStream_t)stream, chunks, R4, H, Fp,
                     a_pad, ds2, dt2, dWh);
  PYGAT_CHECK_LAUNCH("alpha_grad_apply");
  return PYGAT_OK;
}
