// K23 -- the induced subgraph of a node set, written as a CSR directly, and seeded uniform random walks (gfx950).
// include/pygat_amd.h states the semantics; tests/subgraph_ref.py restates them in NumPy.
//
// The sub-pattern: local ids are ranks in ascending global id, so the relabelling is monotone and a row's kept entries, taken in CSR
// position order, already have strictly ascending local columns: no sort, and the result does not depend on the order or the
// multiplicity of the input ids.  Two calls with ONE host read between them (the caller sizes col / edge_rc / edge_ids exactly):
//
// pygat_subgraph_count, all on one stream, nothing read back in between (m = min(n_in, n) bounds the rows):
//   clear      mark[0 .. n) = 0, info = 0
//   mark       per input id: range check (info[2]), mark[id] = 1 -- plain stores, every writer stores the same value
//   scan       mark -> rank                                                             (pygat_exclusive_scan_i32)
//   nodes      sub_nodes[rank[j]] = j for marked j; index[i] = rank[nodes[i]]
//   count      per sub-row the entries whose column is marked: rows of at most SUB_THREAD_ROW entries by their own thread, rows of
//              at most SUB_WAVE_ROW by the whole wave of that thread, one after the other; longer rows are flagged
//   scan, list the flags -> the list of long rows in row order
//   count_long one work-group per long row
//   scan       counts -> sub_rowptr
//   empties    rows without a kept entry, one partial count per work-group (plain stores)
//   info       info = (rows n_sub, entries, id outside, empty rows): the partial counts summed in a fixed order
// pygat_subgraph_fill, after the read, on the same workspace (mark, rank and the list of long rows intact):
//   fill_rows  thread rows emit their kept positions in order; wave rows through a ballot prefix, SUB_WAVE = 64 positions per round
//   fill_long  one work-group per long row, SUB_BLOCK_ROUND = 1024 positions per round (four consecutive ones per thread) through
//              sample_scan<256> (prefix_scan.h, shared with K22)
//   both write, per kept position p at output index k: sub_col[k] = rank[col[p]], edge_rc[k] = (row, that), edge_ids[k] = p.
// Every store of the fill is bounded by the row's range in sub_rowptr and by sub_nnz, whatever the workspace holds.
// All arithmetic is integer, no atomics anywhere, no thread walks more than SUB_THREAD_ROW entries alone (SUB_WAVE_ROW / 64 = 4
// rounds as a lane), every loop runs over a row's positions or a list's length, and no kernel uses scratch.
//
// pygat_random_walk: one thread per walker, one Philox call per four steps (rng.h walk_keys4).  A step is three DEPENDENT loads
// (rowptr[cur], rowptr[cur + 1] -- one line --, then col[...]) at random addresses: the walk is bound by their latency, hundreds of
// cycles each from L2 or the Infinity Cache, and hides it only through the number of walkers in flight.  It is not tuned beyond that.
//
// Shared with K22 and K24 (minibatch.h): the row of an id that may be no node (node_row, is_node), the list of long rows, the room of
// a row in the sub-pattern's CSR, the workspace cursor, the launchers' refusals and the footprint lookup; prefix_scan.h: sample_scan.
#include "minibatch.h"
#include "rng.h"

namespace pygat {

constexpr int SUB_THREAD_ROW = 64;      // a row of at most this many entries is counted and filled by one thread
constexpr int SUB_WAVE_ROW = 256;       // ... of at most this many by one wave, 64 positions per round; longer rows: a work-group
constexpr int SUB_BLOCK_ROUND = 1024;   // positions a work-group takes per round (256 threads x 4 consecutive positions)
constexpr int SUB_PART_BLOCKS = 1024;   // work-groups (and partial counts) of the empty-row count

// positions [b, e) of sub-row r in the graph; false (an empty range) if r is no row or its id is no node
__device__ __forceinline__ bool sub_row(int n, const int32_t* __restrict__ rowptr, const int64_t* __restrict__ sub_nodes, int r,
                                        int n_sub, int* b, int* e) {
  *b = *e = 0;
  return is_node(r, n_sub) && node_row(n, rowptr, sub_nodes[r], b, e);
}

__global__ __launch_bounds__(256) void subgraph_mark_kernel(int n, int n_in, const int64_t* __restrict__ nodes,
                                                            int32_t* __restrict__ mark, int32_t* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_in) return;
  const int64_t id = nodes[i];
  if (!is_node(id, n)) info[2] = 1;
  else mark[id] = 1;
}

// (at most min(n_in, n) ids are marked: rank[j] of a marked j lies inside sub_nodes)
__global__ __launch_bounds__(256) void subgraph_nodes_kernel(int n, int n_in, const int64_t* __restrict__ nodes,
                                                             const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                             int64_t* __restrict__ sub_nodes, int64_t* __restrict__ index) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n && mark[j]) sub_nodes[rank[j]] = j;
  if (j < n_in) {
    const int64_t id = nodes[j];
    index[j] = is_node(id, n) ? rank[id] : -1;
  }
}

// one thread per sub-row r < m; rows at and past n_sub = rank[n] get cnt = 0, so that the scan over m rows ends at the entry count
__global__ __launch_bounds__(256) void subgraph_count_rows_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ gcol, int m,
                                                                  const int64_t* __restrict__ sub_nodes,
                                                                  const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                                  int32_t* __restrict__ cnt, int32_t* __restrict__ lflag) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 256 + threadIdx.x;
  int n_sub = rank[n];
  if (n_sub > m) n_sub = m;
  int b, e;
  sub_row(n, rowptr, sub_nodes, r, n_sub, &b, &e);
  const int d = e - b;
  int c = 0;
  if (d <= SUB_THREAD_ROW)
    for (int p = b; p < e; ++p) c += mark[gcol[p]] ? 1 : 0;
  unsigned long long wave_rows = __ballot(d > SUB_THREAD_ROW && d <= SUB_WAVE_ROW);
  while (wave_rows) {                                               // (uniform over the wave)
    const int l = __ffsll(wave_rows) - 1;
    wave_rows &= wave_rows - 1;
    const int bb = __shfl(b, l), ee = __shfl(e, l);
    int t = 0, tot;
    for (int p = bb + lane; p < ee; p += 64) t += mark[gcol[p]] ? 1 : 0;
    sample_scan<64>(t, &tot, nullptr);
    if (lane == l) c = tot;
  }
  if (r < m) {
    cnt[r] = c;
    lflag[r] = d > SUB_WAVE_ROW ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void subgraph_list_kernel(int m, const int32_t* __restrict__ lflag, const int32_t* __restrict__ lptr,
                                                            int32_t* __restrict__ llist) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  long_list_put(m, lflag, lptr, llist, r);
}

__global__ __launch_bounds__(256) void subgraph_count_long_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ gcol, int m,
                                                                  const int64_t* __restrict__ sub_nodes,
                                                                  const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                                  const int32_t* __restrict__ lptr, const int32_t* __restrict__ llist,
                                                                  int32_t* __restrict__ cnt) {
  __shared__ int wsum[4];
  int n_sub = rank[n];
  if (n_sub > m) n_sub = m;
  const int n_long = long_list_len(lptr, m);
  for (int x = blockIdx.x; x < n_long; x += gridDim.x) {       // (every condition below is uniform over the work-group)
    int r, b, e;
    if (!long_list_row(llist, x, n_sub, &r) || !node_row(n, rowptr, sub_nodes[r], &b, &e)) continue;
    int t = 0, tot;
    for (int p = b + (int)threadIdx.x; p < e; p += 256) t += mark[gcol[p]] ? 1 : 0;
    sample_scan<256>(t, &tot, wsum);
    if (threadIdx.x == 0) cnt[r] = tot;
  }
}

// part[block] = the rows r < n_sub without a kept entry among this work-group's rows
__global__ __launch_bounds__(256) void subgraph_empties_kernel(int n, int m, const int32_t* __restrict__ rank,
                                                               const int32_t* __restrict__ cnt, int32_t* __restrict__ part) {
  __shared__ int wsum[4];
  int n_sub = rank[n];
  if (n_sub > m) n_sub = m;
  int t = 0, tot;
  for (int r = blockIdx.x * 256 + threadIdx.x; r < n_sub; r += gridDim.x * 256) t += cnt[r] == 0 ? 1 : 0;
  sample_scan<256>(t, &tot, wsum);
  if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one work-group: info = (n_sub, entries, <id outside: set by mark>, empty rows)
__global__ __launch_bounds__(256) void subgraph_info_kernel(int n, int m, int nparts, const int32_t* __restrict__ rank,
                                                            const int32_t* __restrict__ sub_rowptr, const int32_t* __restrict__ part,
                                                            int32_t* __restrict__ info) {
  __shared__ int wsum[4];
  int t = 0, tot;
  for (int x = threadIdx.x; x < nparts; x += 256) t += part[x];
  sample_scan<256>(t, &tot, wsum);
  if (threadIdx.x == 0) {
    const int n_sub = rank[n];
    info[0] = n_sub > m ? m : n_sub;
    info[1] = sub_rowptr[m];
    info[3] = tot;
  }
}

struct SubOut {
  int32_t* sub_col;
  int2* edge_rc;
  int64_t* edge_ids;
};
__device__ __forceinline__ void sub_emit(const SubOut& o, int64_t k, int r, int local, int p) {
  o.sub_col[k] = local;
  o.edge_rc[k] = make_int2(r, local);
  o.edge_ids[k] = (int64_t)p;
}

__global__ __launch_bounds__(256) void subgraph_fill_rows_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ gcol, int n_sub, int64_t sub_nnz,
                                                                 const int64_t* __restrict__ sub_nodes,
                                                                 const int32_t* __restrict__ sub_rowptr,
                                                                 const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                                 SubOut out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 256 + threadIdx.x;
  int b, e, base = 0, room = 0;
  if (!sub_row(n, rowptr, sub_nodes, r, n_sub, &b, &e) || !csr_room(sub_rowptr, r, sub_nnz, &base, &room)) b = e = 0;
  const int d = e - b;
  if (d <= SUB_THREAD_ROW) {
    int k = 0;
    for (int p = b; p < e; ++p) {
      const int c = gcol[p];
      if (mark[c]) {
        if (k < room) sub_emit(out, (int64_t)base + k, r, rank[c], p);
        ++k;
      }
    }
  }
  unsigned long long wave_rows = __ballot(d > SUB_THREAD_ROW && d <= SUB_WAVE_ROW);
  while (wave_rows) {                                               // (uniform over the wave)
    const int l = __ffsll(wave_rows) - 1;
    wave_rows &= wave_rows - 1;
    const int bb = __shfl(b, l), ee = __shfl(e, l), wbase = __shfl(base, l), wroom = __shfl(room, l), wr = __shfl(r, l);
    int before = 0;
    for (int p0 = bb; p0 < ee; p0 += 64) {
      const int p = p0 + lane;
      int c = 0;
      bool keep = false;
      if (p < ee) { c = gcol[p]; keep = mark[c] != 0; }
      const unsigned long long km = __ballot(keep);
      const int idx = before + __popcll(km & ((1ull << lane) - 1ull));
      if (keep && idx < wroom) sub_emit(out, (int64_t)wbase + idx, wr, rank[c], p);
      before += __popcll(km);
    }
  }
}

__global__ __launch_bounds__(256) void subgraph_fill_long_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ gcol, int m, int n_sub, int64_t sub_nnz,
                                                                 const int64_t* __restrict__ sub_nodes,
                                                                 const int32_t* __restrict__ sub_rowptr,
                                                                 const int32_t* __restrict__ mark, const int32_t* __restrict__ rank,
                                                                 const int32_t* __restrict__ lptr, const int32_t* __restrict__ llist,
                                                                 SubOut out) {
  __shared__ int wsum[4];
  const int n_long = long_list_len(lptr, m);
  for (int x = blockIdx.x; x < n_long; x += gridDim.x) {       // (every condition below is uniform over the work-group)
    int r, b, e, base = 0, room = 0;
    if (!long_list_row(llist, x, n_sub, &r) || !node_row(n, rowptr, sub_nodes[r], &b, &e) || e - b <= SUB_WAVE_ROW ||
        !csr_room(sub_rowptr, r, sub_nnz, &base, &room))
      continue;
    int before = 0;
    for (int p0 = b; p0 < e; p0 += SUB_BLOCK_ROUND) {
      const int pt = p0 + 4 * (int)threadIdx.x;
      int c[4];
      unsigned km = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        c[j] = 0;
        if (pt + j < e) {
          c[j] = gcol[pt + j];
          km |= (mark[c[j]] ? 1u : 0u) << j;
        }
      }
      int tot;
      int idx = before + sample_scan<256>(__popc(km), &tot, wsum);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((km >> j) & 1) {
          if (idx < room) sub_emit(out, (int64_t)base + idx, r, rank[c[j]], pt + j);
          ++idx;
        }
      before += tot;
    }
  }
}

__global__ __launch_bounds__(256) void random_walk_kernel(int n, const int32_t* __restrict__ rowptr, const int32_t* __restrict__ gcol,
                                                          int64_t n_walk, const int64_t* __restrict__ start, int length,
                                                          const uint64_t* __restrict__ seedp, uint32_t hop,
                                                          int64_t* __restrict__ walks, int32_t* __restrict__ info) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n_walk) return;
  const int64_t id = start[w];
  int64_t* out = walks + w * ((int64_t)length + 1);
  out[0] = id;
  if (!is_node(id, n)) {                  // never used as an index: the walker stays, and the caller hears of it
    info[0] = 1;
    for (int t = 1; t <= length; ++t) out[t] = id;
    return;
  }
  const uint64_t seed = seedp[0];
  int cur = (int)id;
  uint4 k4 = make_uint4(0, 0, 0, 0);
  for (int t = 1; t <= length; ++t) {
    if (t == 1 || (t & 3) == 0) k4 = walk_keys4(seed, (uint32_t)w, hop, (uint32_t)t >> 2);
    const uint32_t k = word_of(k4, t & 3);
    const int b = rowptr[cur], e = rowptr[cur + 1];
    if (e > b) cur = gcol[b + (int)__umulhi(k, (uint32_t)(e - b))];
    out[t] = cur;
  }
}

// the workspace, in int32 units; every table starts at a multiple of 4.  m = min(n_in, n) bounds the rows
struct SubWs {
  int64_t mark, rank, cnt, lflag, lptr, llist, part, tiles, total;
};
static inline int sub_rows_bound(int n, int64_t n_in) { return n_in < n ? (int)n_in : n; }
static inline SubWs sub_ws(int n, int m) {
  WsCursor c;
  SubWs w;
  w.mark = c.take(n);
  w.rank = c.take((int64_t)n + 1);
  w.cnt = c.take(m);
  w.lflag = c.take(m);
  w.lptr = c.take((int64_t)m + 1);
  w.llist = c.take(m);
  w.part = c.take(SUB_PART_BLOCKS);
  w.tiles = c.take((int64_t)(pygat_scan_workspace_bytes(n) / sizeof(int32_t)));
  w.total = c.at;
  return w;
}

int footprint_k23(const char* name, int* regs, int* scratch) {
  return footprint_lookup(
      name,
      {{"k23_mark", &subgraph_mark_kernel}, {"k23_nodes", &subgraph_nodes_kernel}, {"k23_count_rows", &subgraph_count_rows_kernel},
       {"k23_list", &subgraph_list_kernel}, {"k23_count_long", &subgraph_count_long_kernel}, {"k23_empties", &subgraph_empties_kernel},
       {"k23_info", &subgraph_info_kernel}, {"k23_fill_rows", &subgraph_fill_rows_kernel}, {"k23_fill_long", &subgraph_fill_long_kernel},
       {"k23_walk", &random_walk_kernel}},
      "k23_mark, k23_nodes, k23_count_rows, k23_list, k23_count_long, k23_empties, k23_info, k23_fill_rows, k23_fill_long, k23_walk", regs,
      scratch);
}

// the refusals that the count, the fill and the workspace query share
static int sub_sizes(const char* what, int n, int64_t n_in) {
  PYGAT_REQUIRE(n > 0 && n_in > 0 && n_in < ((int64_t)1 << 31), "%s: n=%d nodes, n_in=%lld ids: n >= 1 and 1 <= n_in < 2^31 expected", what,
                n, (long long)n_in);
  return PYGAT_OK;
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_subgraph_workspace_bytes(int n, int64_t n_in, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "subgraph_workspace_bytes: null bytes");
  PYGAT_PASS(sub_sizes("subgraph_workspace_bytes", n, n_in));
  *bytes = (size_t)sub_ws(n, sub_rows_bound(n, n_in)).total * sizeof(int32_t);
  return PYGAT_OK;
}

extern "C" int pygat_subgraph_count(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_in, const int64_t* nodes,
                                    int64_t* sub_nodes, int64_t* index, int32_t* sub_rowptr, int32_t* info, void* ws, void* stream) {
  const char* what = "subgraph_count";
  PYGAT_PASS(sub_sizes(what, n, n_in));
  PYGAT_PASS(require_graph(what, n, nnz, false));
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {nodes, "nodes"}, {sub_nodes, "sub_nodes"}, {index, "index"},
                                   {sub_rowptr, "sub_rowptr"}, {info, "info"}, {ws, "workspace"}}));
  PYGAT_REQUIRE(aligned8(nodes) && aligned8(sub_nodes) && aligned8(index), "%s: nodes, sub_nodes and index must be 8-byte aligned", what);
  PYGAT_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);

  const int m = sub_rows_bound(n, n_in), ni = (int)n_in;
  const SubWs w = sub_ws(n, m);
  int32_t* base = (int32_t*)ws;
  int32_t *mark = base + w.mark, *rank = base + w.rank, *cnt = base + w.cnt, *lflag = base + w.lflag, *lptr = base + w.lptr,
          *llist = base + w.llist, *part = base + w.part;
  void* tiles = base + w.tiles;
  hipStream_t st = (hipStream_t)stream;
  const dim3 tpb(256), rows((unsigned)cdiv(m, 256)), ids((unsigned)cdiv(ni, 256)), both((unsigned)cdiv(ni > n ? ni : n, 256));
  const int nparts = (int)(cdiv(m, 256) < SUB_PART_BLOCKS ? cdiv(m, 256) : SUB_PART_BLOCKS);
  const dim3 longs = long_grid(m);

  PYGAT_PASS(clear_async(what, mark, (size_t)n * sizeof(int32_t), st));
  PYGAT_PASS(clear_async(what, info, 4 * sizeof(int32_t), st));
  hipLaunchKernelGGL(subgraph_mark_kernel, ids, tpb, 0, st, n, ni, nodes, mark, info);
  PYGAT_CHECK_LAUNCH(what);
  PYGAT_PASS(pygat_exclusive_scan_i32(mark, n, rank, tiles, stream));
  hipLaunchKernelGGL(subgraph_nodes_kernel, both, tpb, 0, st, n, ni, nodes, mark, rank, sub_nodes, index);
  hipLaunchKernelGGL(subgraph_count_rows_kernel, rows, tpb, 0, st, n, rowptr, col, m, sub_nodes, mark, rank, cnt, lflag);
  PYGAT_CHECK_LAUNCH(what);
  PYGAT_PASS(pygat_exclusive_scan_i32(lflag, m, lptr, tiles, stream));
  hipLaunchKernelGGL(subgraph_list_kernel, rows, tpb, 0, st, m, lflag, lptr, llist);
  hipLaunchKernelGGL(subgraph_count_long_kernel, longs, tpb, 0, st, n, rowptr, col, m, sub_nodes, mark, rank, lptr, llist, cnt);
  PYGAT_CHECK_LAUNCH(what);
  PYGAT_PASS(pygat_exclusive_scan_i32(cnt, m, sub_rowptr, tiles, stream));
  hipLaunchKernelGGL(subgraph_empties_kernel, dim3((unsigned)nparts), tpb, 0, st, n, m, rank, cnt, part);
  hipLaunchKernelGGL(subgraph_info_kernel, dim3(1), tpb, 0, st, n, m, nparts, rank, sub_rowptr, part, info);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

extern "C" int pygat_subgraph_fill(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_in, int n_sub,
                                   int64_t sub_nnz, const int64_t* sub_nodes, const int32_t* sub_rowptr, int32_t* sub_col,
                                   int32_t* edge_rc, int64_t* edge_ids, void* ws, void* stream) {
  const char* what = "subgraph_fill";
  PYGAT_PASS(sub_sizes(what, n, n_in));
  PYGAT_PASS(require_graph(what, n, nnz, false));
  const int m = sub_rows_bound(n, n_in);
  PYGAT_REQUIRE(n_sub > 0 && n_sub <= m, "%s: n_sub=%d rows: 1 <= n_sub <= min(n_in, n) = %d expected (info[0] of subgraph_count)", what,
                n_sub, m);
  PYGAT_REQUIRE(sub_nnz > 0 && sub_nnz <= nnz, "%s: sub_nnz=%lld entries: 1 <= sub_nnz <= nnz = %lld expected (info[1] of subgraph_count)",
                what, (long long)sub_nnz, (long long)nnz);
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {sub_nodes, "sub_nodes"}, {sub_rowptr, "sub_rowptr"},
                                   {sub_col, "sub_col"}, {edge_rc, "edge_rc"}, {edge_ids, "edge_ids"}, {ws, "workspace"}}));
  PYGAT_REQUIRE(aligned8(sub_nodes) && aligned8(edge_rc) && aligned8(edge_ids), "%s: sub_nodes, edge_rc and edge_ids must be 8-byte aligned",
                what);
  PYGAT_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);

  const SubWs w = sub_ws(n, m);
  const int32_t* base = (const int32_t*)ws;
  const int32_t *mark = base + w.mark, *rank = base + w.rank, *lptr = base + w.lptr, *llist = base + w.llist;
  hipStream_t st = (hipStream_t)stream;
  const SubOut out = {sub_col, reinterpret_cast<int2*>(edge_rc), edge_ids};
  hipLaunchKernelGGL(subgraph_fill_rows_kernel, dim3((unsigned)cdiv(n_sub, 256)), dim3(256), 0, st, n, rowptr, col, n_sub, sub_nnz,
                     sub_nodes, sub_rowptr, mark, rank, out);
  hipLaunchKernelGGL(subgraph_fill_long_kernel, long_grid(n_sub), dim3(256), 0, st, n, rowptr, col, m, n_sub, sub_nnz, sub_nodes,
                     sub_rowptr, mark, rank, lptr, llist, out);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

extern "C" int pygat_random_walk(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int64_t n_walk, const int64_t* start,
                                 int length, const void* seed, uint32_t hop, int64_t* walks, int32_t* info, void* stream) {
  const char* what = "random_walk";
  PYGAT_PASS(require_graph(what, n, nnz));
  PYGAT_REQUIRE(n_walk > 0 && n_walk < ((int64_t)1 << 31), "%s: n_walk=%lld: 1 <= n_walk < 2^31 walkers expected", what,
                (long long)n_walk);
  PYGAT_REQUIRE(length > 0, "%s: length=%d: a walk of length >= 1 expected", what, length);
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {start, "start"}, {seed, "seed"}, {walks, "walks"}, {info, "info"}}));
  PYGAT_REQUIRE(aligned8(seed), "%s: seed must be 8-byte aligned", what);
  PYGAT_REQUIRE(aligned8(start) && aligned8(walks), "%s: start and walks must be 8-byte aligned", what);
  hipStream_t st = (hipStream_t)stream;
  PYGAT_PASS(clear_async(what, info, sizeof(int32_t), st));
  hipLaunchKernelGGL(random_walk_kernel, dim3((unsigned)cdiv(n_walk, 256)), dim3(256), 0, st, n, rowptr, col, n_walk, start, length,
                     (const uint64_t*)seed, hop, walks, info);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}
