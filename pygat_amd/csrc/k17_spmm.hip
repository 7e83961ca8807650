// K17 -- the reference's SpecialSpmm (layers.py:70-95) as an op of its own: a sparse pattern with per-entry values times a dense
// table, and the gradient with respect to the values, for H heads at once.
//   spmm    out[i, h, f] = sum_{k in row i} val[perm[k], h] * b[col[k], h, f]        walks the rows of a CSR (rowptr, col); perm[k] =
//           the caller's entry index of CSR position k (NULL: k itself), val [nnz x H] in the caller's order.  The gradient with
//           respect to b is this kernel on the transposed pattern with G in place of b.
//   sddmm   dval[k, h] = sum_f G[row_k, h, f] * b[col_k, h, f]                       one lane group per (entry, head), entries in the
//           caller's order (edge_rc [nnz][2]); the lanes of a head reduce their partial dot products with DPP sums.
// Rows are H*F floats, NOT padded (the caller's tensors).  Lane mapping as K15's: a group of LPR lanes holds one row, VEC chunks of
// CW floats per lane, chunk c = c0 + 64 v.  CW = 4 (16-byte loads) where F % 4 == 0 and rows are 16-byte aligned -- a chunk then lies
// inside one head -- and CW = 1 for any other F (F = 1 and F = 7 are the reference's own uses; at most 4 floats per lane there, a
// wider row is walked in windows of 256 floats, grid dimension y).  A wave carries 64 / LPR rows, and
// every lane group loads the rows of up to four entries before it adds them, in entry order: several gathers in flight per wave.
// A long row goes through partial records (the rule of long_rows.h), one wave per chunk: its lane groups walk the piece of a long
// row entry-interleaved and are added in a fixed butterfly; a record is the row's H * F sums, and records add.  No float atomics,
// every sum in a fixed order: two runs give the same bits.  A row without entries gets exact zeros.
#include "long_rows.h"
#include <string.h>

namespace pygat {

constexpr int SP_MAX_ROW = 1024;                    // floats per row, H * F
constexpr unsigned SP_SDDMM_MAX_BLOCKS = 1u << 20;  // the entry-parallel launch strides over the rest

struct SpArgs {
  int n, H, F, NCH;            // rows of the walked pattern; heads; width of a head; chunks of CW floats per row
  int64_t nnz;
  const int32_t *rowptr, *col, *perm;
  const float *val, *b;
  int64_t ldb, ldo;
  float* out;
  float* part;                 // [long_records(nnz) x pstride]
  int64_t pstride;             // H * F rounded up to 4 floats
};

static inline int64_t sp_pstride(int H, int F) { return ((int64_t)H * F + 3) & ~(int64_t)3; }

// entries whose rows a lane group loads before it adds them (registers: U * VEC * (CW + 1) for the rows and the values)
__host__ __device__ constexpr int sp_unroll(int cw, int vec) { return vec * (cw + 1) <= 10 ? 4 : (vec * (cw + 1) <= 20 ? 2 : 1); }

template <int VEC>
struct SpLane {
  int ofs[VEC];    // float offset of the lane's chunk inside a row (0 when the chunk lies beyond the row)
  int head[VEC];
};

template <int CW, int LPR, int VEC>
__device__ __forceinline__ SpLane<VEC> sp_lane(const SpArgs& g) {
  SpLane<VEC> ln;
  const int c0 = (threadIdx.x & 63) & (LPR - 1);
#pragma unroll
  for (int v = 0; v < VEC; ++v) {
    const int c = c0 + 64 * v + 64 * VEC * blockIdx.y;
    ln.ofs[v] = c < g.NCH ? CW * c : 0;
    ln.head[v] = ln.ofs[v] / g.F;
  }
  return ln;
}
template <int LPR, int VEC>
__device__ __forceinline__ bool sp_valid(const SpArgs& g, int v) {
  return ((threadIdx.x & 63) & (LPR - 1)) + 64 * v + 64 * VEC * blockIdx.y < g.NCH;
}

template <int CW>
__device__ __forceinline__ void sp_load(const float* p, float (&w)[CW]) {
  if constexpr (CW == 4) {
    const float4 t = ld4(p);
    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
  } else {
    w[0] = *p;
  }
}
template <int CW>
__device__ __forceinline__ void sp_store(float* p, const float (&w)[CW]) {
  if constexpr (CW == 4) st4(p, make_float4(w[0], w[1], w[2], w[3]));
  else *p = w[0];
}

// U walked entries e, e + step, ...: every row and value is loaded, then they are added in entry order
template <int CW, int VEC, int U>
__device__ __forceinline__ void sp_entries(const SpArgs& g, const SpLane<VEC>& ln, int64_t e, int64_t step, float (&acc)[VEC][CW]) {
  float w[U][VEC][CW], a[U][VEC];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int64_t k = e + u * step;
    const int64_t src = g.col[k], ent = g.perm ? (int64_t)g.perm[k] : k;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
      sp_load<CW>(g.b + src * g.ldb + ln.ofs[v], w[u][v]);
      a[u][v] = g.val[ent * g.H + ln.head[v]];
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u)
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int k = 0; k < CW; ++k) acc[v][k] = fmaf(a[u][v], w[u][v][k], acc[v][k]);
}

// the entries e0, e0 + step, ... < e1 of one row, in that order
template <int CW, int VEC>
__device__ __forceinline__ void sp_walk(const SpArgs& g, const SpLane<VEC>& ln, int64_t e0, int64_t e1, int64_t step,
                                        float (&acc)[VEC][CW]) {
  constexpr int U = sp_unroll(CW, VEC);
  int64_t e = e0;
  if constexpr (U > 1)
    for (; e + (U - 1) * step < e1; e += U * step) sp_entries<CW, VEC, U>(g, ln, e, step, acc);
  for (; e < e1; e += step) sp_entries<CW, VEC, 1>(g, ln, e, step, acc);
}

// launch 1: one wave per chunk; the piece of every long row inside the chunk -> one partial record
template <int CW, int LPR, int VEC>
__global__ __launch_bounds__(64) void sp_long_kernel(SpArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63, grp = lane / LPR;
  const LongChunk ch = long_chunk_span(blockIdx.x, g.nnz);
  const SpLane<VEC> ln = sp_lane<CW, LPR, VEC>(g);
  for_long_rows(g.rowptr, row_of(g.rowptr, g.n, ch.c0), row_of(g.rowptr, g.n, ch.c1 - 1), ch,
                [&](int, int64_t, int64_t, int64_t e0, int64_t e1, int slot) {
    float acc[VEC][CW];
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int k = 0; k < CW; ++k) acc[v][k] = 0.f;
    sp_walk<CW, VEC>(g, ln, e0 + grp, e1, EPW, acc);
#pragma unroll
    for (int off = LPR; off < 64; off <<= 1)                   // lane groups of the wave, a fixed butterfly
#pragma unroll
      for (int v = 0; v < VEC; ++v)
#pragma unroll
        for (int k = 0; k < CW; ++k) acc[v][k] += __shfl_xor(acc[v][k], off);
    if (grp == 0) {
      float* p = g.part + long_record(blockIdx.x, slot) * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v)
        if (sp_valid<LPR, VEC>(g, v)) sp_store<CW>(p + ln.ofs[v], acc[v]);
    }
  });
}

// launch 2: one lane group per row
template <int CW, int LPR, int VEC>
__global__ __launch_bounds__(256) void sp_row_kernel(SpArgs g) {
  constexpr int EPW = 64 / LPR;
  const int lane = threadIdx.x & 63;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * EPW + lane / LPR;
  if (row >= g.n) return;                                      // (whole lane groups; nothing below crosses a group)
  const SpLane<VEC> ln = sp_lane<CW, LPR, VEC>(g);
  const int64_t start = g.rowptr[row], end = g.rowptr[row + 1];
  float acc[VEC][CW];
#pragma unroll
  for (int v = 0; v < VEC; ++v)
#pragma unroll
    for (int k = 0; k < CW; ++k) acc[v][k] = 0.f;
  if (end - start > LONG_ROW) {
    for_long_records(start, end, [&](int64_t rec) {
      const float* p = g.part + rec * g.pstride;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        float w[CW];
        sp_load<CW>(p + ln.ofs[v], w);
#pragma unroll
        for (int k = 0; k < CW; ++k) acc[v][k] += w[k];
      }
    });
  } else {
    sp_walk<CW, VEC>(g, ln, start, end, 1, acc);
  }
#pragma unroll
  for (int v = 0; v < VEC; ++v)
    if (sp_valid<LPR, VEC>(g, v)) sp_store<CW>(g.out + row * g.ldo + ln.ofs[v], acc[v]);
}

// dval: a group of lph lanes per (entry, head), the head's chunks dealt round-robin to its lanes
template <int CW>
__global__ __launch_bounds__(256) void sp_sddmm_kernel(int64_t units, int H, int F, int lph, int lph_shift,
                                                       const int2* __restrict__ rc, const float* __restrict__ G, int64_t ldg,
                                                       const float* __restrict__ b, int64_t ldb, float* __restrict__ dval) {
  const int64_t sweep = ((int64_t)gridDim.x * 256) >> lph_shift;
  const int l = threadIdx.x & (lph - 1), nch = F / CW;
  for (int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> lph_shift; q < units; q += sweep) {   // (whole lane groups)
    const int64_t e = q / H;
    const int h = (int)(q - e * H);
    const int2 p = rc[e];
    const float* gp = G + (int64_t)p.x * ldg + (int64_t)h * F;
    const float* bp = b + (int64_t)p.y * ldb + (int64_t)h * F;
    float acc = 0.f;
    for (int c = l; c < nch; c += lph) {
      if constexpr (CW == 4) acc += dot4(ld4(gp + 4 * c), ld4(bp + 4 * c));
      else acc = fmaf(gp[c], bp[c], acc);
    }
    acc = group_sum_rt(acc, lph);
    if (l == 0) dval[q] = acc;
  }
}

// (CW, LPR, VEC) of a row of H * F floats: 16-byte chunks (VEC <= 4) or single floats (VEC 1, 2 or 4, in `windows` of 64 * VEC)
static inline void sp_pick(int H, int F, bool vec16, int* cw, int* lpr, int* vec, int* nch, int* windows) {
  *cw = vec16 ? 4 : 1;
  *nch = H * F / *cw;
  if (*nch <= 64) {
    int l = 1;
    while (l < *nch) l <<= 1;
    *lpr = l; *vec = 1;
  } else {
    *lpr = 64; *vec = (*nch + 63) / 64;
    if (!vec16) *vec = *nch <= 128 ? 2 : 4;
  }
  *windows = (*nch + 64 * *vec - 1) / (64 * *vec);
}

#define PYGAT_SP_LPR(CWV, LPRV, ...)                                   \
  switch (LPRV) {                                                       \
    case 1: { constexpr int CW = CWV, LPR = 1, VEC = 1; __VA_ARGS__; } break;  \
    case 2: { constexpr int CW = CWV, LPR = 2, VEC = 1; __VA_ARGS__; } break;  \
    case 4: { constexpr int CW = CWV, LPR = 4, VEC = 1; __VA_ARGS__; } break;  \
    case 8: { constexpr int CW = CWV, LPR = 8, VEC = 1; __VA_ARGS__; } break;  \
    case 16: { constexpr int CW = CWV, LPR = 16, VEC = 1; __VA_ARGS__; } break; \
    case 32: { constexpr int CW = CWV, LPR = 32, VEC = 1; __VA_ARGS__; } break; \
    default: { constexpr int CW = CWV, LPR = 64, VEC = 1; __VA_ARGS__; } break; \
  }
#define PYGAT_SP_DISPATCH(CWV, LPRV, VECV, ...)                                  \
  do {                                                                            \
    if ((CWV) == 4) {                                                             \
      if ((VECV) == 1) { PYGAT_SP_LPR(4, LPRV, __VA_ARGS__) }                            \
      else if ((VECV) == 2) { constexpr int CW = 4, LPR = 64, VEC = 2; __VA_ARGS__; }    \
      else if ((VECV) == 3) { constexpr int CW = 4, LPR = 64, VEC = 3; __VA_ARGS__; }    \
      else { constexpr int CW = 4, LPR = 64, VEC = 4; __VA_ARGS__; }                     \
    } else {                                                                      \
      if ((VECV) == 1) { PYGAT_SP_LPR(1, LPRV, __VA_ARGS__) }                            \
      else if ((VECV) == 2) { constexpr int CW = 1, LPR = 64, VEC = 2; __VA_ARGS__; }    \
      else { constexpr int CW = 1, LPR = 64, VEC = 4; __VA_ARGS__; }                     \
    }                                                                             \
  } while (0)

static const void* sp_kernel_ptr(bool lng, int cw, int lpr, int vec) {
  const void* f = nullptr;
  PYGAT_SP_DISPATCH(cw, lpr, vec, f = lng ? reinterpret_cast<const void*>(&sp_long_kernel<CW, LPR, VEC>)
                                          : reinterpret_cast<const void*>(&sp_row_kernel<CW, LPR, VEC>));
  return f;
}

// pygat_kernel_footprint: k17_sddmm_c<CW>, k17_spmm_{long,row}_c<CW>l<LPR>v<VEC> (the lane shapes of PYGAT_SP_DISPATCH)
int footprint_k17(const char* name, int* regs, int* scratch) {
  const void* fn = nullptr;
  if (!strcmp(name, "k17_sddmm_c4")) {
    fn = reinterpret_cast<const void*>(&sp_sddmm_kernel<4>);
  } else if (!strcmp(name, "k17_sddmm_c1")) {
    fn = reinterpret_cast<const void*>(&sp_sddmm_kernel<1>);
  } else {
    char kind[8] = "", rest = 0;
    int cw = 0, lpr = 0, vec = 0;
    if (sscanf(name, "k17_spmm_%4[a-z]_c%dl%dv%d%c", kind, &cw, &lpr, &vec, &rest) == 4 && (cw == 1 || cw == 4) && lpr >= 1 &&
        lpr <= 64 && (lpr & (lpr - 1)) == 0 && (!strcmp(kind, "long") || !strcmp(kind, "row"))) {
      const bool wide = cw == 4 ? (vec >= 2 && vec <= 4) : (vec == 2 || vec == 4);
      if (vec == 1 || (lpr == 64 && wide)) fn = sp_kernel_ptr(!strcmp(kind, "long"), cw, lpr, vec);
    }
  }
  if (!fn) {
    set_error("kernel_footprint: unknown kernel '%s' (k17_sddmm_c<CW>, k17_spmm_{long,row}_c<CW>l<LPR>v<VEC>)", name);
    return PYGAT_EINVAL;
  }
  return kernel_footprint_of(fn, regs, scratch);
}

static int sp_check_shape(const char* what, int64_t nnz, int H, int F) {
  PYGAT_REQUIRE(nnz >= 0 && nnz < ((int64_t)1 << 31), "%s: nnz %lld outside [0, 2^31) (int32 entry indexing)", what, (long long)nnz);
  PYGAT_REQUIRE(H >= 1 && H <= 64, "%s: H=%d heads outside [1, 64]", what, H);
  PYGAT_REQUIRE(F >= 1, "%s: F=%d, a head needs F >= 1 columns", what, F);
  PYGAT_REQUIRE((int64_t)H * F <= SP_MAX_ROW, "%s: row too wide: H x F = %d x %d > %d floats", what, H, F, SP_MAX_ROW);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_spmm_workspace_bytes(int64_t nnz, int H, int F, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "spmm_workspace_bytes: null bytes");
  const int rc = sp_check_shape("spmm_workspace_bytes", nnz, H, F);
  if (rc != PYGAT_OK) return rc;
  *bytes = (size_t)(long_records(nnz) * sp_pstride(H, F)) * sizeof(float);
  return PYGAT_OK;
}

extern "C" int pygat_spmm_forward(int n_rows, int64_t nnz, const int32_t* rowptr, const int32_t* col, const int32_t* perm, int H,
                                  int F, const float* val, const float* b, int64_t ldb, float* out, int64_t ldo, void* ws,
                                  void* stream) {
  const int rc = sp_check_shape("spmm_forward", nnz, H, F);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(n_rows >= 0, "spmm_forward: n_rows=%d", n_rows);
  PYGAT_REQUIRE(ldb >= (int64_t)H * F && ldo >= (int64_t)H * F, "spmm_forward: row strides ldb=%lld, ldo=%lld below H x F = %d",
                (long long)ldb, (long long)ldo, H * F);
  if (n_rows == 0) return PYGAT_OK;
  PYGAT_REQUIRE(rowptr && out && ws, "spmm_forward: null rowptr / out / workspace");
  PYGAT_REQUIRE(nnz == 0 || (col && val && b), "spmm_forward: null col / val / b");
  PYGAT_REQUIRE(aligned16(ws), "spmm_forward: the workspace must be 16-byte aligned");
  SpArgs g;
  memset(&g, 0, sizeof(g));
  const bool vec16 = F % 4 == 0 && ldb % 4 == 0 && ldo % 4 == 0 && aligned16(b) && aligned16(out);
  int cw, lpr, vec, windows;
  sp_pick(H, F, vec16, &cw, &lpr, &vec, &g.NCH, &windows);
  g.n = n_rows; g.H = H; g.F = F; g.nnz = nnz; g.rowptr = rowptr; g.col = col; g.perm = perm; g.val = val; g.b = b;
  g.ldb = ldb; g.ldo = ldo; g.out = out; g.part = static_cast<float*>(ws); g.pstride = sp_pstride(H, F);
  const unsigned chunks = (unsigned)long_chunks(nnz);
  const unsigned blocks = (unsigned)cdiv(n_rows, 4 * (64 / lpr));
  hipStream_t st = (hipStream_t)stream;
  if (chunks)
    PYGAT_SP_DISPATCH(cw, lpr, vec, hipLaunchKernelGGL((sp_long_kernel<CW, LPR, VEC>), dim3(chunks, windows), dim3(64), 0, st, g));
  PYGAT_SP_DISPATCH(cw, lpr, vec, hipLaunchKernelGGL((sp_row_kernel<CW, LPR, VEC>), dim3(blocks, windows), dim3(256), 0, st, g));
  PYGAT_CHECK_LAUNCH("spmm_forward");
  return PYGAT_OK;
}

extern "C" int pygat_spmm_grad_values(int64_t nnz, const int32_t* edge_rc, int H, int F, const float* G, int64_t ldg, const float* b,
                                      int64_t ldb, float* dval, void* stream) {
  const int rc = sp_check_shape("spmm_grad_values", nnz, H, F);
  if (rc != PYGAT_OK) return rc;
  PYGAT_REQUIRE(ldg >= (int64_t)H * F && ldb >= (int64_t)H * F, "spmm_grad_values: row strides ldg=%lld, ldb=%lld below H x F = %d",
                (long long)ldg, (long long)ldb, H * F);
  if (nnz == 0) return PYGAT_OK;
  PYGAT_REQUIRE(edge_rc && G && b && dval, "spmm_grad_values: null edge_rc / G / b / dval");
  PYGAT_REQUIRE(((uintptr_t)edge_rc & 7u) == 0, "spmm_grad_values: edge_rc must be 8-byte aligned");
  const bool vec16 = F % 4 == 0 && ldg % 4 == 0 && ldb % 4 == 0 && aligned16(G) && aligned16(b);
  const int nch = vec16 ? F / 4 : F;
  int lph = 1, shift = 0;
  while (lph < nch && lph < 64) { lph <<= 1; ++shift; }
  const int64_t units = nnz * H;
  int64_t blocks = cdiv(units * lph, 256);
  if (blocks > SP_SDDMM_MAX_BLOCKS) blocks = SP_SDDMM_MAX_BLOCKS;
  const int2* rcp = reinterpret_cast<const int2*>(edge_rc);
  hipStream_t st = (hipStream_t)stream;
  if (vec16)
    hipLaunchKernelGGL(sp_sddmm_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, st, units, H, F, lph, shift, rcp, G, ldg, b, ldb, dval);
  else
    hipLaunchKernelGGL(sp_sddmm_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, units, H, F, lph, shift, rcp, G, ldg, b, ldb, dval);
  PYGAT_CHECK_LAUNCH("spmm_grad_values");
  return PYGAT_OK;
}
