// K18 -- edge_softmax: the softmax of per-entry logits over the entries of every row (or column) of a sparse pattern, for H heads
// at once, and its gradient (the reference's layers.py:145-150,160 as an op of its own, attention dropout off).
//   rows        m[i, h] = max_{k in group i} l[k, h],  Z[i, h] = sum_{k in group i} exp(l[k, h] - m[i, h])     walks a CSR (rowptr, perm)
//   apply       alpha[k, h] = exp(l[k, h] - m[i_k, h]) / Z[i_k, h]                                        one element per lane
//   grad_rows   c[i, h] = sum_{k in group i} alpha[k, h] G[k, h]                                         the same walk
//   grad_apply  dl[k, h] = alpha[k, h] (G[k, h] - c[i_k, h])                                             one element per lane
// l, alpha, G, dl are [nnz x H] in the CALLER's entry order; perm[k] = the caller's entry index of CSR position k (NULL: k itself).
// Group pass.  A group of L lanes (a power of two) walks one row.  A lane holds CW consecutive heads of an entry -- CW = 4, a
// 16-byte load, where H % 4 == 0 and the tables are 16-byte aligned, else CW = 1 -- so an entry is UPE = H / CW lanes wide and the group walks
// EPL = L / UPE entries side by side (lanes beyond EPL * UPE idle: any H in 1..64).  Per head a lane keeps an online (m, Z) state,
// one __expf per element, or a running dot product.  The lanes of a head are then combined in a fixed order: the maximum first
// (exact in any order), every lane's Z rescaled to it once, then the sum -- a butterfly where UPE is a power of two, lane after lane
// otherwise.  A long row goes through partial records (the rule of long_rows.h), one wave per chunk; a record is (m, Z) per head
// or c per head, merged in chunk order.  No LDS, no float atomics, every sum in a fixed order: two runs give the same bits.
// A group without entries gets m = Z = c = 0.  A group of one entry gets Z = 1 and c = G exactly: alpha = 1 and dl = 0 exactly.
#include "long_rows.h"
#include <float.h>
#include <string.h>

namespace pygat {

constexpr unsigned ES_MAX_BLOCKS = 1u << 20;   // the entry-parallel launches stride over the rest
constexpr float ES_SEED = -FLT_MAX;            // running-max seed: finite, so no difference of two maxima is a NaN

struct EsArgs {
  int n, H, UPE;               // groups of the walked pattern; heads; lanes per entry
  int64_t nnz;
  const int32_t *rowptr, *perm;
  const float *x, *y;          // softmax: the logits; gradient: alpha and G
  float *o0, *o1;              // softmax: m and Z; gradient: c            [n x H]
  float* part;                 // [long_records(nnz) x 2 H]: m then Z of every head; the gradient uses the first H floats
};

struct EsLane {
  int l, u, eo, src0;          // lane inside its group; its unit of an entry; its entry offset; the wave lane of (unit u, offset 0)
  bool work;                   // eo < EPL
};

__device__ __forceinline__ EsLane es_lane(int L, int UPE, int EPL) {
  EsLane ln;
  const int lane = threadIdx.x & 63;
  ln.l = lane & (L - 1);
  ln.eo = ln.l / UPE;
  ln.u = ln.l - ln.eo * UPE;
  ln.src0 = lane - ln.l + ln.u;
  ln.work = ln.eo < EPL;
  return ln;
}

template <int CW>
__device__ __forceinline__ void es_load(const float* p, float (&w)[CW]) {
  if constexpr (CW == 4) {
    const float4 t = ld4(p);
    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
  } else {
    w[0] = *p;
  }
}

// online softmax state of one head, one __expf per element (K2's fold_edge)
__device__ __forceinline__ void es_fold(float& m, float& z, float ev) {
  const float d = ev - m;
  const float ex = __expf(-fabsf(d));
  const bool up = d > 0.f;
  z = up ? fmaf(z, ex, 1.f) : z + ex;
  m = up ? ev : m;
}

// (m, z) <- (m, z) (+) (m2, z2), the earlier entries on the left
__device__ __forceinline__ void es_merge(float& m, float& z, float m2, float z2) {
  const float mn = fmaxf(m, m2);
  z = z * __expf(m - mn) + z2 * __expf(m2 - mn);
  m = mn;
}

template <int CW>
__device__ __forceinline__ void es_init(float (&m)[CW], float (&z)[CW]) {
#pragma unroll
  for (int k = 0; k < CW; ++k) { m[k] = ES_SEED; z[k] = 0.f; }
}

// U walked entries e, e + step, ...: every record is loaded, then they are folded in entry order
template <int CW, bool GRAD, int U>
__device__ __forceinline__ void es_entries(const EsArgs& g, int64_t e, int64_t step, int ofs, float (&m)[CW], float (&z)[CW]) {
  float a[U][CW], b[U][CW];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t k = e + u * step;
    const int64_t rec = (g.perm ? (int64_t)g.perm[k] : k) * g.H + ofs;
    es_load<CW>(g.x + rec, a[u]);
    if constexpr (GRAD) es_load<CW>(g.y + rec, b[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int k = 0; k < CW; ++k) {
      if constexpr (GRAD) z[k] = fmaf(a[u][k], b[u][k], z[k]);
      else es_fold(m[k], z[k], a[u][k]);
    }
}

// the entries e0, e0 + step, ... < e1 of one group, in that order; four records in flight
template <int CW, bool GRAD>
__device__ __forceinline__ void es_walk(const EsArgs& g, int64_t e0, int64_t e1, int64_t step, int ofs, float (&m)[CW], float (&z)[CW]) {
  int64_t e = e0;
  for (; e + 3 * step < e1; e += 4 * step) es_entries<CW, GRAD, 4>(g, e, step, ofs, m, z);
  for (; e < e1; e += step) es_entries<CW, GRAD, 1>(g, e, step, ofs, m, z);
}

// over the lanes of a group with the same unit; all of them end with the result.  Every lane of the wave calls it.
template <bool MAX>
__device__ __forceinline__ float es_across(float v, const EsLane& ln, int L, int UPE, int EPL) {
  if ((UPE & (UPE - 1)) == 0) {                              // EPL * UPE == L: a butterfly over the lane bits above the unit's
    for (int o = UPE; o < L; o <<= 1) {
      const float t = __shfl_xor(v, o);
      v = MAX ? fmaxf(v, t) : v + t;
    }
    return v;
  }
  float tot = __shfl(v, ln.src0);
  for (int k = 1; k < EPL; ++k) {
    const float t = __shfl(v, ln.src0 + k * UPE);
    tot = MAX ? fmaxf(tot, t) : tot + t;
  }
  return tot;
}

template <int CW, bool GRAD>
__device__ __forceinline__ void es_combine(float (&m)[CW], float (&z)[CW], const EsLane& ln, int L, int UPE, int EPL) {
#pragma unroll
  for (int k = 0; k < CW; ++k) {
    if constexpr (!GRAD) {
      const float mx = es_across<true>(m[k], ln, L, UPE, EPL);
      z[k] *= __expf(m[k] - mx);                             // (a lane without entries: 0 x 0)
      m[k] = mx;
    }
    z[k] = es_across<false>(z[k], ln, L, UPE, EPL);
  }
}

// launch 1: one wave per chunk; the piece of every long row inside the chunk -> one partial record
template <int CW, bool GRAD>
__global__ __launch_bounds__(64) void es_long_kernel(EsArgs g) {
  const int EPL = 64 / g.UPE;
  const EsLane ln = es_lane(64, g.UPE, EPL);
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    float m[CW], z[CW];
    es_init<CW>(m, z);
    if (ln.work) es_walk<CW, GRAD>(g, e0 + ln.eo, e1, EPL, ln.u * CW, m, z);
    es_combine<CW, GRAD>(m, z, ln, 64, g.UPE, EPL);
    if (ln.l < g.UPE) {
      float* p = g.part + long_record(blockIdx.x, slot) * (2 * g.H) + ln.u * CW;
#pragma unroll
      for (int k = 0; k < CW; ++k) {
        if constexpr (GRAD) p[k] = z[k];
        else { p[k] = m[k]; p[g.H + k] = z[k]; }
      }
    }
  });
}

// launch 2: one group of L lanes per row
template <int CW, bool GRAD>
__global__ __launch_bounds__(256) void es_row_kernel(EsArgs g, int L) {
  const int EPL = L / g.UPE;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / L) + lane / L;
  if (row >= g.n) return;                                      // (whole lane groups; nothing below crosses a group)
  const EsLane ln = es_lane(L, g.UPE, EPL);
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
  float m[CW], z[CW];
  es_init<CW>(m, z);
  if (end - start > LONG_ROW) {
    if (ln.l < g.UPE)
      for_long_records(start, end, [&](int64_t rec) {
        const float* p = g.part + rec * (2 * g.H) + ln.u * CW;
#pragma unroll
        for (int k = 0; k < CW; ++k) {
          if constexpr (GRAD) z[k] += p[k];
          else es_merge(m[k], z[k], p[k], p[g.H + k]);
        }
      });
  } else {
    if (ln.work) es_walk<CW, GRAD>(g, start + ln.eo, end, EPL, ln.u * CW, m, z);
    es_combine<CW, GRAD>(m, z, ln, L, g.UPE, EPL);
  }
  if (ln.l >= g.UPE) return;
  const int64_t q = row * g.H + ln.u * CW;
#pragma unroll
  for (int k = 0; k < CW; ++k) {
    if constexpr (GRAD) {
      g.o0[q + k] = z[k];                                      // (a group without entries: the empty sum)
    } else {
      g.o0[q + k] = end > start ? m[k] : 0.f;
      g.o1[q + k] = z[k];
    }
  }
}

// alpha (GRAD false: x = logits, t0 = m, t1 = Z) or dlogits (GRAD true: x = alpha, y = G, t0 = c), one element per lane in the
// caller's order; the group of entry k is half `side` of edge_rc[k]
template <bool GRAD>
__global__ __launch_bounds__(256) void es_apply_kernel(int64_t total, int H, int hshift, int side, const int32_t* __restrict__ rc,
                                                       const float* __restrict__ x, const float* __restrict__ y,
                                                       const float* __restrict__ t0, const float* __restrict__ t1,
                                                       float* __restrict__ out) {
  const int64_t sweep = (int64_t)gridDim.x * 256;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += sweep) {
    int64_t k;
    int h;
    if (hshift >= 0) {
      k = idx >> hshift; h = (int)(idx & (H - 1));
    } else if (idx < ((int64_t)1 << 32)) {
      const unsigned q = (unsigned)idx / (unsigned)H;
      k = q; h = (int)((unsigned)idx - q * (unsigned)H);
    } else {
      k = idx / H; h = (int)(idx - k * H);
    }
    const int64_t q = (int64_t)rc[2 * k + side] * H + h;
    if constexpr (GRAD) out[idx] = x[idx] * (y[idx] - t0[q]);
    else out[idx] = __expf(x[idx] - t0[q]) / t1[q];
  }
}

// pygat_kernel_footprint: k18_rows_long_c<CW>, k18_rows_c<CW>, k18_grad_rows_long_c<CW>, k18_grad_rows_c<CW> (CW 1 or 4), k18_apply,
// k18_grad_apply
int footprint_k18(const char* name, int* regs, int* scratch) {
  static const struct { const char* name; const void* fn; } tab[] = {
      {"k18_rows_long_c1", reinterpret_cast<const void*>(&es_long_kernel<1, false>)},
      {"k18_rows_long_c4", reinterpret_cast<const void*>(&es_long_kernel<4, false>)},
      {"k18_rows_c1", reinterpret_cast<const void*>(&es_row_kernel<1, false>)},
      {"k18_rows_c4", reinterpret_cast<const void*>(&es_row_kernel<4, false>)},
      {"k18_grad_rows_long_c1", reinterpret_cast<const void*>(&es_long_kernel<1, true>)},
      {"k18_grad_rows_long_c4", reinterpret_cast<const void*>(&es_long_kernel<4, true>)},
      {"k18_grad_rows_c1", reinterpret_cast<const void*>(&es_row_kernel<1, true>)},
      {"k18_grad_rows_c4", reinterpret_cast<const void*>(&es_row_kernel<4, true>)},
      {"k18_apply", reinterpret_cast<const void*>(&es_apply_kernel<false>)},
      {"k18_grad_apply", reinterpret_cast<const void*>(&es_apply_kernel<true>)},
  };
  for (const auto& t : tab)
    if (!strcmp(name, t.name)) return kernel_footprint_of(t.fn, regs, scratch);
  set_error("kernel_footprint: unknown kernel '%s' (k18_rows_long_c<CW>, k18_rows_c<CW>, k18_grad_rows_long_c<CW>, "
            "k18_grad_rows_c<CW>, k18_apply, k18_grad_apply)", name);
  return PYGAT_EINVAL;
}

static int es_check_shape(const char* what, int64_t nnz, int H) {
  PYGAT_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31), "%s: nnz %lld outside [0, 2^31) (int32 entry indexing)", what, (long long)nnz);
  PYGAT_REQUIRE(H >= 1 && H <= 64, "%s: H=%d heads outside [1, 64]", what, H);
  return PYGAT_OK;
}

// the group pass of either direction: x (and y) [nnz x H] -> o0 (and o1) [n_rows x H]
template <bool GRAD>
static int es_group_pass(const char* what, int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* perm, int H, const float* x,
                         const float* y, float* o0, float* o1, void* ws, void* stream) {
  const int rc = es_check_shape(what, nnz, H);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(n_rows >= 0, "%s: n_rows=%d", what, n_rows);
  if (nnz == 0) return PYGAT_OK;
  PYGAT_REQUIRE(n_rows > 0, "%s: n_rows=0 with nnz=%lld entries", what, (long long)nnz);
  PYGAT_REQUIRE(rowptr, "%s: null rowptr", what);
  PYGAT_REQUIRE(x, "%s: null %s", what, GRAD ? "alpha" : "logits");
  if constexpr (GRAD) PYGAT_REQUIRE(y, "%s: null G", what);
  PYGAT_REQUIRE(o0, "%s: null %s", what, GRAD ? "c" : "m");
  if constexpr (!GRAD) PYGAT_REQUIRE(o1, "%s: null Z", what);
  PYGAT_REQUIRE(ws, "%s: null workspace", what);
  PYGAT_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);
  EsArgs g;
  memset(&g, 0, sizeof(g));
  const bool vec16 = H % 4 == 0 && aligned16(x) && (!GRAD || aligned16(y));     // (with or without perm: a record is H floats)
  const int cw = vec16 ? 4 : 1;
  g.n = n_rows; g.H = H; g.UPE = H / cw; g.nnz = nnz; g.rowptr = rowptr; g.perm = perm; g.x = x; g.y = y; g.o0 = o0; g.o1 = o1;
  g.part = static_cast<float*>(ws);
  int L = 1;
  while (L < 8 * g.UPE && L < 64) L <<= 1;                     // eight entries side by side where a wave has the lanes
  const unsigned chunks = (unsigned)long_chunks(nnz);
  const unsigned blocks = (unsigned)cdiv(n_rows, 4 * (64 / L));
  hipStream_t st = (hipStream_t)stream;
  if (vec16) {
    hipLaunchKernelGGL((es_long_kernel<4, GRAD>), dim3(chunks), dim3(64), 0, st, g);
    hipLaunchKernelGGL((es_row_kernel<4, GRAD>), dim3(blocks), dim3(256), 0, st, g, L);
  } else {
    hipLaunchKernelGGL((es_long_kernel<1, GRAD>), dim3(chunks), dim3(64), 0, st, g);
    hipLaunchKernelGGL((es_row_kernel<1, GRAD>), dim3(blocks), dim3(256), 0, st, g, L);
  }
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

template <bool GRAD>
static int es_entry_pass(const char* what, int64_t nnz, const int32_t* edge_rc, int side, int H, const float* x, const float* y,
                         const float* t0, const float* t1, float* out, void* stream) {
  const int rc = es_check_shape(what, nnz, H);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(side == 0 || side == 1, "%s: side=%d, 0 (the row of an entry) or 1 (its column) expected", what, side);
  if (nnz == 0) return PYGAT_OK;
  PYGAT_REQUIRE(edge_rc, "%s: null edge_rc", what);
  PYGAT_REQUIRE(x, "%s: null %s", what, GRAD ? "alpha" : "logits");
  if constexpr (GRAD) PYGAT_REQUIRE(y, "%s: null G", what);
  PYGAT_REQUIRE(t0, "%s: null %s", what, GRAD ? "c" : "m");
  if constexpr (!GRAD) PYGAT_REQUIRE(t1, "%s: null Z", what);
  PYGAT_REQUIRE(out, "%s: null %s", what, GRAD ? "dlogits" : "alpha");
  const int64_t total = nnz * H;
  int64_t blocks = cdiv(total, 256);
  if (blocks > ES_MAX_BLOCKS) blocks = ES_MAX_BLOCKS;
  const int hshift = (H & (H - 1)) == 0 ? ilog2(H) : -1;
  hipLaunchKernelGGL(es_apply_kernel<GRAD>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, total, H, hshift, side, edge_rc,
                     x, y, t0, t1, out);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_edge_softmax_workspace_bytes(int64_t nnz, int H, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "edge_softmax_workspace_bytes: null bytes");
  const int rc = es_check_shape("edge_softmax_workspace_bytes", nnz, H);
  if (rc != PYGAT_OK) return rc;
  *bytes = (size_t)(long_records(nnz) * 2 * H) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_edge_softmax_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* perm, int H, const float* logits,
                                       float* m, float* Z, void* ws, void* stream) {
  return es_group_pass<false>("edge_softmax_rows", n_rows, nnz, rowptr, perm, H, logits, nullptr, m, Z, ws, stream);
}

extern "C" int pygat_edge_softmax_apply(int64_t nnz, const int32_t* edge_rc, int side, int H, const float* logits, const float* m,
                                        const float* Z, float* alpha, void* stream) {
  return es_entry_pass<false>("edge_softmax_apply", nnz, edge_rc, side, H, logits, nullptr, m, Z, alpha, stream);
}

extern "C" int pygat_edge_softmax_grad_rows(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* perm, int H,
                                            const float* alpha, const float* G, float* c, void* ws, void* stream) {
  return es_group_pass<true>("edge_softmax_grad_rows", n_rows, nnz, rowptr, perm, H, alpha, G, c, nullptr, ws, stream);
}

extern "C" int pygat_edge_softmax_grad_apply(int64_t nnz, const int32_t* edge_rc, int side, int H, const float* alpha, const float* G,
                                             const float* c, float* dlogits, void* stream) {
  return es_entry_pass<true>("edge_softmax_grad_apply", nnz, edge_rc, side, H, alpha, G, c, nullptr, dlogits, stream);
}
