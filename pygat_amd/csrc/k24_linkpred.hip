// K24 -- link-prediction mini-batches: the CSR position of (row, col) pairs, and seeded negative destinations per source node (gfx950).
// include/pygat_amd.h states the semantics; tests/linkpred_ref.py restates them in NumPy.
//
// pygat_find_edges (k24_find): one thread per pair, a lower-bound binary search for the column over the row's strictly ascending
// columns; pos = that position, or -1.  An id outside [0, n) on either side is never an index: pos = -1 and info[0] = 1.
//
// pygat_draw_negatives (k24_draw): one thread per draw.  For the flat draw i = w * num_neg + s of source u = src[w] the forbidden
// list c_0 < ... < c_{f-1} is the columns of row u, with u itself merged in at its sorted place if exclude_self asks for it and the
// row does not hold it; m = n - f ids are left.  With k = word (i & 3) of the Philox call of the draws 4 * (i >> 2) .. + 3 (rng.h
// neg_keys4) and r = (k * m) >> 32, the draw is the r-th smallest id outside the list: r + t*, t* = #{t : c_t - t <= r}.  c_t - t is
// the number of allowed ids below c_t and does not decrease with t, so t* is ONE upper-bound binary search over the row -- no
// rejection loop, the same work at any density, and a value that depends on (seed, hop, i) and the row alone.  The merged list is
// never written: neg_elem() reads it through the lower bound pu of u in the row.  m == 0 gives -1 and info[1] = 1; an id outside
// [0, n) is never an index, its draws are -1 and info[0] = 1.  The flags are plain stores of one value.
// The four lanes of a quad evaluate the same Philox call in the same instructions, so the call costs a wave what it would cost the
// quad's first lane alone, and every draw keeps a thread of its own for its loads (a thread per FOUR draws would run their searches
// one after the other).
//
// Both kernels are integer only, have no atomics and use no scratch.  A pair or a draw is a chain of DEPENDENT loads at random
// addresses -- rowptr[u], rowptr[u + 1] (one line), then about log2(d) columns per search (two searches for a draw with
// exclude_self) -- so both are bound by the latency of those loads, hundreds of cycles each from L2 or the Infinity Cache, and hide
// it only through the number of threads in flight.  They are not tuned beyond that occupancy.
//
// Shared with K22 and K23 (minibatch.h): is_node, the launchers' refusals and the footprint lookup.
#include "minibatch.h"
#include "rng.h"

namespace pygat {

// the row [b, e) of node u, kept inside [0, nnz) whatever rowptr holds.  Not minibatch.h's node_row with the clamp on top: that
// reads the same rows but compiles to other code, and these two kernels stay the bytes they were
__device__ __forceinline__ void lp_row(const int32_t* __restrict__ rowptr, int u, int nnz, int* b, int* e) {
  int rb = rowptr[u], re = rowptr[u + 1];
  if (rb < 0) rb = 0;
  if (re > nnz) re = nnz;
  if (re < rb) re = rb;
  *b = rb; *e = re;
}

// the first position p in [b, e) with col[p] >= c (e if there is none)
__device__ __forceinline__ int lp_lower_bound(const int32_t* __restrict__ gcol, int b, int e, int c) {
  int lo = b, hi = e;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (gcol[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void find_edges_kernel(int n, int nnz, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ gcol, int n_pairs, const int64_t* __restrict__ row,
                                                         const int64_t* __restrict__ colq, int64_t* __restrict__ pos,
                                                         int32_t* __restrict__ info) {
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gi >= n_pairs) return;
  const int i = (int)gi;
  const int64_t r = row[i], c = colq[i];
  if (r < 0 || r >= n || c < 0 || c >= n) {       // never used as an index, and the caller hears of it.  (Written out: on
                                                  // is_node the two checks compile to other code, and this kernel stays its bytes)
    info[0] = 1;
    pos[i] = -1;
    return;
  }
  int b, e;
  lp_row(rowptr, (int)r, nnz, &b, &e);
  const int p = lp_lower_bound(gcol, b, e, (int)c);
  pos[i] = (p < e && gcol[p] == (int)c) ? (int64_t)p : (int64_t)-1;
}

// element t of the forbidden list of a row [b, b + d) with u merged in at place pu (merged) or as the row stands
__device__ __forceinline__ int neg_elem(const int32_t* __restrict__ gcol, int b, int t, bool merged, int pu, int u) {
  if (!merged || t < pu) return gcol[b + t];
  return t == pu ? u : gcol[b + t - 1];
}

__global__ __launch_bounds__(256) void draw_negatives_kernel(int n, int nnz, const int32_t* __restrict__ rowptr,
                                                             const int32_t* __restrict__ gcol, int n_draws,
                                                             const int64_t* __restrict__ src, int num_neg, int exclude_self,
                                                             const uint64_t* __restrict__ seedp, uint32_t hop,
                                                             int64_t* __restrict__ neg, int32_t* __restrict__ info) {
  const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gi >= n_draws) return;
  const int i = (int)gi;
  const int64_t id = src[i / num_neg];
  if (!is_node(id, n)) {                          // never used as an index, and the caller hears of it
    info[0] = 1;
    neg[i] = -1;
    return;
  }
  const int u = (int)id;
  int b, e;
  lp_row(rowptr, u, nnz, &b, &e);
  const int d = e - b;
  int pu = 0;
  bool merged = false;
  if (exclude_self) {
    const int p = lp_lower_bound(gcol, b, e, u);
    pu = p - b;
    merged = !(p < e && gcol[p] == u);
  }
  const int f = d + (merged ? 1 : 0);
  const int m = n - f;
  if (m <= 0) {                                   // every id is forbidden
    info[1] = 1;
    neg[i] = -1;
    return;
  }
  const uint32_t k = word_of(neg_keys4(seedp[0], (uint32_t)i >> 2, hop), i & 3);
  const int r = (int)__umulhi(k, (uint32_t)m);
  int lo = 0, hi = f;                             // t* = the first t with elem(t) - t > r
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (neg_elem(gcol, b, mid, merged, pu, u) - mid <= r) lo = mid + 1;
    else hi = mid;
  }
  neg[i] = (int64_t)r + lo;
}

int footprint_k24(const char* name, int* regs, int* scratch) {
  return footprint_lookup(name, {{"k24_find", &find_edges_kernel}, {"k24_draw", &draw_negatives_kernel}}, "k24_find, k24_draw", regs, scratch);
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_find_edges(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_pairs, const int64_t* row,
                                const int64_t* colq, int64_t* pos, int32_t* info, void* stream) {
  const char* what = "find_edges";
  PYGAT_PASS(require_graph(what, n, nnz));
  PYGAT_REQUIRE(n_pairs > 0 && n_pairs < ((int64_t)1 << 31), "%s: n_pairs=%lld: 1 <= n_pairs < 2^31 pairs expected", what,
                (long long)n_pairs);
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {row, "row"}, {colq, "colq"}, {pos, "pos"}, {info, "info"}}));
  PYGAT_REQUIRE(aligned8(row) && aligned8(colq) && aligned8(pos), "%s: row, colq and pos must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  PYGAT_PASS(clear_async(what, info, sizeof(int32_t), st));
  hipLaunchKernelGGL(find_edges_kernel, dim3((unsigned)cdiv(n_pairs, 256)), dim3(256), 0, st, n, (int)nnz, rowptr, col, (int)n_pairs, row,
                     colq, pos, info);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

extern "C" int pygat_draw_negatives(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_src, const int64_t* src,
                                    int num_neg, int exclude_self, const void* seed, uint32_t hop, int64_t* neg, int32_t* info,
                                    void* stream) {
  const char* what = "draw_negatives";
  PYGAT_PASS(require_graph(what, n, nnz));
  PYGAT_REQUIRE(n_src > 0 && n_src < ((int64_t)1 << 31), "%s: n_src=%lld: 1 <= n_src < 2^31 source nodes expected", what,
                (long long)n_src);
  PYGAT_REQUIRE(num_neg > 0, "%s: num_neg=%d: num_neg >= 1 draws per source node expected", what, num_neg);
  PYGAT_REQUIRE(n_src * (int64_t)num_neg < ((int64_t)1 << 31), "%s: n_src=%lld x num_neg=%d draws: fewer than 2^31 expected", what,
                (long long)n_src, num_neg);
  PYGAT_REQUIRE(exclude_self == 0 || exclude_self == 1, "%s: exclude_self=%d: 0 or 1 expected", what, exclude_self);
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {src, "src"}, {seed, "seed"}, {neg, "neg"}, {info, "info"}}));
  PYGAT_REQUIRE(aligned8(seed), "%s: seed must be 8-byte aligned", what);
  PYGAT_REQUIRE(aligned8(src) && aligned8(neg), "%s: src and neg must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  PYGAT_PASS(clear_async(what, info, 2 * sizeof(int32_t), st));
  const int n_draws = (int)(n_src * num_neg);
  hipLaunchKernelGGL(draw_negatives_kernel, dim3((unsigned)cdiv(n_draws, 256)), dim3(256), 0, st, n, (int)nnz, rowptr, col, n_draws, src,
                     num_neg, exclude_self, (const uint64_t*)seed, hop, neg, info);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}
