// What the mini-batch ops (k22_sample.hip, k23_subgraph.hip, k24_linkpred.hip) share besides the prefix count of prefix_scan.h: the row
// of a node id that may be no node, the list of long rows, the room of a row in an output CSR, the workspace cursor, the launchers'
// refusals and the footprint lookup.  One copy of each; integer only, no atomics.  Every message is the one the launchers always gave.
#pragma once
#include "prefix_scan.h"
#include <initializer_list>
#include <string.h>

namespace pygat {

// ---- device: a node id from outside is never used as an index --------------------------------------------------------------------
__device__ __forceinline__ bool is_node(int64_t id, int n) { return id >= 0 && id < n; }

// positions [b, e) of the row of node `id` in the graph; false and an empty row if the id is no node, an empty row where re <= rb
__device__ __forceinline__ bool node_row(int n, const int32_t* __restrict__ rowptr, int64_t id, int* b, int* e) {
  *b = *e = 0;
  if (!is_node(id, n)) return false;
  const int rb = rowptr[id], re = rowptr[id + 1];
  if (re > rb) { *b = rb; *e = re; }
  return true;
}

// ---- the long rows: flagged by a count pass, their flags scanned into lptr, listed in row order, walked by LONG_BLOCKS work-groups --
constexpr int LONG_BLOCKS = 1024;
static inline dim3 long_grid(int rows) { return dim3((unsigned)(rows < LONG_BLOCKS ? rows : LONG_BLOCKS)); }

__device__ __forceinline__ void long_list_put(int rows, const int32_t* __restrict__ lflag, const int32_t* __restrict__ lptr,
                                              int32_t* __restrict__ llist, int r) {
  if (r < rows && lflag[r]) llist[lptr[r]] = r;
}
// the length of the list, never past `rows` whatever the workspace holds; walked as for (x = blockIdx.x; x < len; x += gridDim.x)
__device__ __forceinline__ int long_list_len(const int32_t* __restrict__ lptr, int rows) {
  const int n_long = lptr[rows];
  return n_long > rows ? rows : n_long;
}
// *r = entry x of the list; false if what stands there is no row below `bound`
__device__ __forceinline__ bool long_list_row(const int32_t* __restrict__ llist, int x, int bound, int* r) {
  *r = llist[x];
  return *r >= 0 && *r < bound;
}

// where row r of an output CSR writes: false (base and room untouched) if nothing is to be written -- *stop is set (K22: a repeat
// in dst was seen), an empty row, or a range that does not lie inside [0, cap), which no valid input produces
template <typename Base>
__device__ __forceinline__ bool csr_room(const int32_t* __restrict__ out_rowptr, int r, int64_t cap, Base* base, int* room,
                                         const int32_t* __restrict__ stop = nullptr) {
  if (stop && *stop) return false;
  const int ob = out_rowptr[r], oe = out_rowptr[r + 1];
  if (ob < 0 || oe <= ob || (int64_t)oe > cap) return false;
  *base = ob; *room = oe - ob;
  return true;
}

// ---- host: the workspace in int32 units, every table at a multiple of 4 -------------------------------------------------------------
struct WsCursor {
  int64_t at = 0;
  int64_t take(int64_t words) { const int64_t here = at; at += (words + 3) & ~(int64_t)3; return here; }
};

// ---- host: the launchers' preamble.  PYGAT_REQUIRE returns from the function it stands in, so each refusal is a function that
// returns an rc and the launcher passes it on through PYGAT_PASS ----------------------------------------------------------------------
#define PYGAT_PASS(call)                      \
  do {                                        \
    const int rc__ = (call);                  \
    if (rc__ != PYGAT_OK) return rc__;        \
  } while (0)

// (subgraph_count and subgraph_fill name n in sub_sizes' refusal before this one: name_n = false)
static inline int require_graph(const char* what, int n, int64_t nnz, bool name_n = true) {
  const bool ok = n > 0 && nnz > 0 && nnz < ((int64_t)1 << 31);
  PYGAT_REQUIRE(ok || !name_n, "%s: n=%d nodes, nnz=%lld: a graph with 1 <= nnz < 2^31 expected", what, n, (long long)nnz);
  PYGAT_REQUIRE(ok, "%s: nnz=%lld: a graph with 1 <= nnz < 2^31 expected", what, (long long)nnz);
  return PYGAT_OK;
}

struct NamedTable { const void* p; const char* name; };
static inline int require_tables(const char* what, std::initializer_list<NamedTable> tables) {
  for (const auto& t : tables) PYGAT_REQUIRE(t.p, "%s: null %s", what, t.name);
  return PYGAT_OK;
}

// clears `bytes` at p on the stream, or reports the HIP error
static inline int clear_async(const char* what, void* p, size_t bytes, hipStream_t st) {
  const hipError_t me = hipMemsetAsync(p, 0, bytes, st);
  if (me == hipSuccess) return PYGAT_OK;
  (void)hipGetLastError();
  set_error("%s: %s", what, hipGetErrorString(me));
  return PYGAT_EHIP;
}

// ---- host: pygat_kernel_footprint of a family -- its {name, kernel} table and the text of the names for the refusal ---------------
struct NamedKernel {
  const char* name;
  const void* fn;
  template <typename Fn>
  NamedKernel(const char* name_, Fn* kernel) : name(name_), fn(reinterpret_cast<const void*>(kernel)) {}
};
static inline int footprint_lookup(const char* name, std::initializer_list<NamedKernel> table, const char* names, int* regs, int* scratch) {
  for (const auto& k : table)
    if (!strcmp(name, k.name)) return kernel_footprint_of(k.fn, regs, scratch);
  set_error("kernel_footprint: unknown kernel '%s' (%s)", name, names);
  return PYGAT_EINVAL;
}

}  // namespace pygat
