// K22 -- seeded neighbour sampling: the block (destination nodes x sampled sources) the pattern ops are fed with, written as a CSR
// directly (gfx950).  include/pygat_amd.h states the semantics; tests/sampler_ref.py restates them in NumPy.
//
// Passes of pygat_sample_block, all on one stream, nothing read back in between:
//   count     per dst row: range check, cnt = min(degree, fanout), marker[dst[r]] = r + 1, long-row flag, src_nodes[r] = dst[r]
//   verify    marker[dst[r]] != r + 1 -> some id repeats (plain stores: whichever store won, one of the two rows sees a mismatch)
//   scan x 2  cnt -> blk_rowptr; long-row flags -> positions in the list of long rows   (pygat_exclusive_scan_i32)
//   list      the long rows in row order; info[0] = entries
//   select    short rows (positions span <= 64 Philox calls): one wave per row, keys in registers, bitwise radix select by ballots;
//             long rows: one work-group per row, four 8-bit radix passes over a 256-bin LDS histogram (integer LDS atomics), keys
//             recomputed per pass.  Both end in sample_emit: the kept positions in ascending order through a prefix count, and a
//             plain store of 1 at mark[column] of each.
//   clear     mark[dst[r]] = 0
//   scan      mark -> rank
//   sources   src_nodes[n_dst + rank[j]] = j for marked j; info[1] = sources
//   relabel   per entry: row by binary search in blk_rowptr, local column = dst position (marker) or n_dst + rank; edge_rc
// The marker table is never cleared: marker[j] = m names a dst row only if 1 <= m <= n_dst and dst[m - 1] == j, which is checked.
// Every loop runs over a row's positions or a list's length; all arithmetic is integer.
//
// pygat_weighted_block is the same passes on the WEIGHTED instantiations: the key of an entry becomes sample_weighted_key(Philox word,
// weight[p]) (rng.h: the bits of an fp32 exponential clock, which order like it), and only entries of weight > 0 are candidates.  The
// weight is re-read wherever the key is recomputed.  What changes in the order of the passes: a row's count is its number of positive
// weights, which no single thread may walk along a hub, so the list of long rows is built BEFORE the counts are scanned (the long-row
// flags depend on the degrees only) and a work-group per long row counts it (count_long); info[0] is then written by a pass of its own
// (entries), and a weight that is negative or NaN raises info[4] in count / count_long.  A row is kept whole ("all") when its count is
// below the fanout; at exactly the fanout the select runs and ends at the row's largest key, which keeps the same entries.  No float
// is summed across lanes and no result depends on an order of atomics: two runs give the same bits.
//
// Shared with K23 and K24 (minibatch.h): the row of an id that may be no node (node_row, is_node), the list of long rows, the room of
// a row in the block's CSR, the workspace cursor, the launcher's refusals and the footprint lookup; prefix_scan.h: sample_scan.
#include "minibatch.h"
#include "rng.h"

namespace pygat {

constexpr int SAMPLE_WAVE_QUADS = 64;     // a row whose positions span more Philox calls than this goes to a work-group

__device__ __forceinline__ int sample_quads(int b, int e) { return ((e - 1) >> 2) - (b >> 2) + 1; }   // e > b

// WEIGHTED: d is the number of positive weights of a short row (at most 256 of them, one thread); a long row's count is left to
// sample_count_long_kernel
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void sample_count_kernel(int n, const int32_t* __restrict__ rowptr, int n_dst,
                                                           const int64_t* __restrict__ dst, int fanout,
                                                           const float* __restrict__ weight, int32_t* __restrict__ marker,
                                                           int32_t* __restrict__ cnt, int32_t* __restrict__ lflag,
                                                           int64_t* __restrict__ src_nodes, int32_t* __restrict__ info) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_dst) return;
  int b, e;
  if (node_row(n, rowptr, dst[r], &b, &e)) marker[dst[r]] = r + 1;
  else info[2] = 1;
  int d = e - b;
  const int lf = (d > 0 && sample_quads(b, e) > SAMPLE_WAVE_QUADS) ? 1 : 0;
  if constexpr (WEIGHTED) {
    d = 0;
    if (!lf) {
      bool bad = false;
      for (int p = b; p < e; ++p) {
        const float w = weight[p];
        d += w > 0.f ? 1 : 0;
        bad |= !(w >= 0.f);
      }
      if (bad) info[4] = 1;
    }
  }
  src_nodes[r] = dst[r];
  cnt[r] = d < fanout ? d : fanout;
  lflag[r] = lf;
}

__global__ __launch_bounds__(256) void sample_verify_kernel(int n, int n_dst, const int64_t* __restrict__ dst,
                                                            const int32_t* __restrict__ marker, int32_t* __restrict__ info) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_dst) return;
  const int64_t id = dst[r];
  if (is_node(id, n) && marker[id] != r + 1) info[3] = 1;
}

// WEIGHTED: the counts are not scanned yet (blk_rowptr is not read); sample_entries_kernel writes info[0] later
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void sample_list_kernel(int n_dst, const int32_t* __restrict__ lflag, const int32_t* __restrict__ lptr,
                                                          const int32_t* __restrict__ blk_rowptr, int32_t* __restrict__ llist,
                                                          int32_t* __restrict__ info) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if constexpr (!WEIGHTED)
    if (r == 0) info[0] = blk_rowptr[n_dst];
  long_list_put(n_dst, lflag, lptr, llist, r);
}

__global__ void sample_entries_kernel(int n_dst, const int32_t* __restrict__ blk_rowptr, int32_t* __restrict__ info) {
  if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = blk_rowptr[n_dst];
}

// (sample_scan, the wave and work-group prefix count used below, lives in prefix_scan.h: k23_subgraph.hip shares it)

// Writes the kept positions of the row [b, e) in ascending order at edge_ids[base ...] (at most `room` of them) and marks their
// columns: all of them (`all`), or those with key < T and the first `ties` of those with key == T.  The index of an entry is the
// number of kept entries in front of it, from one prefix count over (entries below T, entries equal to T) per THREADS Philox calls.
// WEIGHTED: only entries of weight > 0 are kept at all, and the key is sample_weighted_key of the Philox word and the weight.
template <int THREADS, bool WEIGHTED>
__device__ __forceinline__ void sample_emit(uint64_t seed, uint32_t hop, int b, int e, bool all, uint32_t T, int ties, int64_t base,
                                            int room, const int32_t* __restrict__ gcol, const float* __restrict__ weight,
                                            int64_t* __restrict__ edge_ids, int32_t* __restrict__ mark, int* wsum) {
  const int tid = THREADS == 64 ? (threadIdx.x & 63) : threadIdx.x;
  const int qb = b >> 2, qe = (e - 1) >> 2;
  int less_before = 0, eq_before = 0;
  for (int q0 = qb; q0 <= qe; q0 += THREADS) {
    const int q = q0 + tid;
    unsigned lm = 0, em = 0;
    if (q <= qe) {
      uint4 w = make_uint4(0, 0, 0, 0);
      if (!all) w = sample_keys4(seed, (uint32_t)q, hop);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint32_t p = 4u * (uint32_t)q + j;
        uint32_t key = word_of(w, j);
        if (p >= (uint32_t)b && p < (uint32_t)e) {
          if constexpr (WEIGHTED) {
            const float wt = weight[p];
            if (!(wt > 0.f)) continue;
            if (!all) key = sample_weighted_key(key, wt);
          }
          if (all || key < T) lm |= 1u << j;
          else if (key == T) em |= 1u << j;
        }
      }
    }
    int tot;
    const int ex = sample_scan<THREADS>(__popc(lm) | (__popc(em) << 16), &tot, wsum);   // <= 4 THREADS <= 1024 each: no carry
    int lb = less_before + (ex & 0xFFFF), eb = eq_before + (ex >> 16);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int idx = -1;
      if ((lm >> j) & 1) { idx = lb + (eb < ties ? eb : ties); ++lb; }
      else if ((em >> j) & 1) { if (eb < ties) idx = lb + eb; ++eb; }
      if (idx >= 0 && idx < room) {
        const uint32_t p = 4u * (uint32_t)q + j;
        edge_ids[base + idx] = (int64_t)p;
        mark[gcol[p]] = 1;
      }
    }
    less_before += tot & 0xFFFF;
    eq_before += tot >> 16;
  }
}

// ---- WEIGHTED, long rows: the number of positive weights of every row of the list, one work-group per row (integer sums) ----------
__global__ __launch_bounds__(256) void sample_count_long_kernel(int n, const int32_t* __restrict__ rowptr, int n_dst,
                                                                const int64_t* __restrict__ dst, int fanout,
                                                                const float* __restrict__ weight, const int32_t* __restrict__ lptr,
                                                                const int32_t* __restrict__ llist, int32_t* __restrict__ cnt,
                                                                int32_t* __restrict__ info) {
  __shared__ int wsum[4];
  const int n_long = long_list_len(lptr, n_dst);
  for (int x = blockIdx.x; x < n_long; x += gridDim.x) {       // (every condition below is uniform over the work-group)
    int r;
    if (!long_list_row(llist, x, n_dst, &r)) continue;
    int b, e;
    node_row(n, rowptr, dst[r], &b, &e);
    int pos = 0;
    bool bad = false;
    for (int p = b + (int)threadIdx.x; p < e; p += 256) {
      const float w = weight[p];
      pos += w > 0.f ? 1 : 0;
      bad |= !(w >= 0.f);
    }
    if (bad) info[4] = 1;
    int tot;
    sample_scan<256>(pos, &tot, wsum);
    if (threadIdx.x == 0) cnt[r] = tot < fanout ? tot : fanout;
  }
}

// ---- short rows: one wave per row, the row's keys in registers (one Philox call per lane) ---------------------------------------
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void sample_select_wave_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                 const int32_t* __restrict__ gcol, int n_dst,
                                                                 const int64_t* __restrict__ dst, int fanout,
                                                                 const float* __restrict__ weight,
                                                                 const uint64_t* __restrict__ seedp, uint32_t hop, int64_t cap,
                                                                 const int32_t* __restrict__ blk_rowptr, int64_t* __restrict__ edge_ids,
                                                                 int32_t* __restrict__ mark, const int32_t* __restrict__ info) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_dst) return;
  int b, e, room;
  int64_t base;
  node_row(n, rowptr, dst[r], &b, &e);
  if (e <= b || sample_quads(b, e) > SAMPLE_WAVE_QUADS || !csr_room(blk_rowptr, r, cap, &base, &room, info + 3)) return;
  const uint64_t seed = seedp[0];
  const bool all = WEIGHTED ? room < fanout : e - b <= fanout;     // (room = min(positive weights, fanout))
  uint32_t T = 0;
  int kk = 0;
  if (!all) {
    const int q = (b >> 2) + lane;
    const uint4 w4 = sample_keys4(seed, (uint32_t)q, hop);
    uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
    unsigned cand = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = 4u * (uint32_t)q + j;
      if (p >= (uint32_t)b && p < (uint32_t)e) {
        if constexpr (WEIGHTED) {
          const float wt = weight[p];
          if (!(wt > 0.f)) continue;
          w[j] = sample_weighted_key(w[j], wt);
        }
        cand |= 1u << j;
      }
    }
    kk = fanout;                       // the rank sought among the candidates, 1-based
    for (int bit = 31; bit >= 0; --bit) {
      unsigned z = 0;
      int c0 = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool zj = ((cand >> j) & 1) && !((w[j] >> bit) & 1);
        c0 += __popcll(__ballot(zj));
        z |= (zj ? 1u : 0u) << j;
      }
      if (kk <= c0) cand = z;
      else { kk -= c0; T |= 1u << bit; cand &= ~z; }
    }
  }
  sample_emit<64, WEIGHTED>(seed, hop, b, e, all, T, kk, base, room, gcol, weight, edge_ids, mark, nullptr);
}

// ---- long rows: one work-group per row of the list, radix select over the 32-bit key in four 8-bit passes -------------------------
template <bool WEIGHTED>
__global__ __launch_bounds__(256) void sample_select_block_kernel(int n, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ gcol, int n_dst,
                                                                  const int64_t* __restrict__ dst, int fanout,
                                                                  const float* __restrict__ weight,
                                                                  const uint64_t* __restrict__ seedp, uint32_t hop, int64_t cap,
                                                                  const int32_t* __restrict__ blk_rowptr,
                                                                  const int32_t* __restrict__ lptr, const int32_t* __restrict__ llist,
                                                                  int64_t* __restrict__ edge_ids, int32_t* __restrict__ mark,
                                                                  const int32_t* __restrict__ info) {
  __shared__ int hist[256];
  __shared__ int wsum[4];
  __shared__ int sel[2];
  const int tid = threadIdx.x;
  const uint64_t seed = seedp[0];
  const int n_long = long_list_len(lptr, n_dst);
  for (int x = blockIdx.x; x < n_long; x += gridDim.x) {       // (every condition below is uniform over the work-group)
    int r;
    if (!long_list_row(llist, x, n_dst, &r)) continue;
    int b, e, room;
    int64_t base;
    node_row(n, rowptr, dst[r], &b, &e);
    if (e <= b || !csr_room(blk_rowptr, r, cap, &base, &room, info + 3)) continue;
    const bool all = WEIGHTED ? room < fanout : e - b <= fanout;
    uint32_t T = 0;
    int kk = fanout;
    if (!all) {
      const int qb = b >> 2, qe = (e - 1) >> 2;
      for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        hist[tid] = 0;
        __syncthreads();
        for (int q = qb + tid; q <= qe; q += 256) {
          const uint4 w = sample_keys4(seed, (uint32_t)q, hop);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t p = 4u * (uint32_t)q + j;
            uint32_t key = word_of(w, j);
            bool in = p >= (uint32_t)b && p < (uint32_t)e;
            if constexpr (WEIGHTED) {
              const float wt = in ? weight[p] : 0.f;
              in = wt > 0.f;
              if (in) key = sample_weighted_key(key, wt);
            }
            in = in && (pass == 0 || ((key ^ T) >> (shift + 8)) == 0);
            if (in) atomicAdd(&hist[(key >> shift) & 255u], 1);
          }
        }
        __syncthreads();
        const int h = hist[tid];
        int tot;
        const int ex = sample_scan<256>(h, &tot, wsum);
        if (ex < kk && kk <= ex + h) { sel[0] = tid; sel[1] = kk - ex; }     // one bin holds the rank sought
        __syncthreads();
        T |= (uint32_t)sel[0] << shift;
        kk = sel[1];
        __syncthreads();
      }
    }
    sample_emit<256, WEIGHTED>(seed, hop, b, e, all, T, kk, base, room, gcol, weight, edge_ids, mark, wsum);
  }
}

__global__ __launch_bounds__(256) void sample_clear_dst_kernel(int n, int n_dst, const int64_t* __restrict__ dst,
                                                               int32_t* __restrict__ mark) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_dst) return;
  const int64_t id = dst[r];
  if (is_node(id, n)) mark[id] = 0;
}

__global__ __launch_bounds__(256) void sample_sources_kernel(int n, int n_dst, const int32_t* __restrict__ mark,
                                                             const int32_t* __restrict__ rank, int64_t src_cap,
                                                             int64_t* __restrict__ src_nodes, int32_t* __restrict__ info) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j == 0) info[1] = n_dst + rank[n];
  if (j >= n || !mark[j]) return;
  const int64_t pos = (int64_t)n_dst + rank[j];
  if (pos < src_cap) src_nodes[pos] = j;
}

__global__ __launch_bounds__(256) void sample_relabel_kernel(int64_t nnz, const int32_t* __restrict__ gcol, int n_dst,
                                                             const int64_t* __restrict__ dst, int64_t cap,
                                                             const int32_t* __restrict__ blk_rowptr, const int32_t* __restrict__ marker,
                                                             const int32_t* __restrict__ rank, const int64_t* __restrict__ edge_ids,
                                                             int32_t* __restrict__ blk_col, int32_t* __restrict__ edge_rc,
                                                             const int32_t* __restrict__ info) {
  const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (info[3] || k >= cap || k >= blk_rowptr[n_dst]) return;
  int lo = 0, hi = n_dst;                 // the last row r with blk_rowptr[r] <= k (rows without entries in between are passed over)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blk_rowptr[mid] <= k) lo = mid; else hi = mid;
  }
  const int64_t p = edge_ids[k];
  int local = -1;
  if (p >= 0 && p < nnz) {
    const int j = gcol[p];
    const int m = marker[j];
    local = (m >= 1 && m <= n_dst && dst[m - 1] == j) ? m - 1 : n_dst + rank[j];
  }
  blk_col[k] = local;
  edge_rc[2 * k] = lo;
  edge_rc[2 * k + 1] = local;
}

// the workspace, in int32 units; every table starts at a multiple of 4
struct SampleWs {
  int64_t marker, mark, rank, cnt, lflag, lptr, llist, tiles, total;
};
static inline SampleWs sample_ws(int n, int n_dst) {
  WsCursor c;
  SampleWs w;
  w.marker = c.take(n);
  w.mark = c.take(n);
  w.rank = c.take((int64_t)n + 1);
  w.cnt = c.take(n_dst);
  w.lflag = c.take(n_dst);
  w.lptr = c.take((int64_t)n_dst + 1);
  w.llist = c.take(n_dst);
  w.tiles = c.take((int64_t)(pygat_scan_workspace_bytes(n > n_dst ? n : n_dst) / sizeof(int32_t)));
  w.total = c.at;
  return w;
}

int footprint_k22(const char* name, int* regs, int* scratch) {
  return footprint_lookup(
      name,
      {{"k22_count", &sample_count_kernel<false>}, {"k22_verify", &sample_verify_kernel}, {"k22_list", &sample_list_kernel<false>},
       {"k22_select_wave", &sample_select_wave_kernel<false>}, {"k22_select_block", &sample_select_block_kernel<false>},
       {"k22_clear_dst", &sample_clear_dst_kernel}, {"k22_sources", &sample_sources_kernel}, {"k22_relabel", &sample_relabel_kernel},
       {"k22_count_weighted", &sample_count_kernel<true>}, {"k22_list_weighted", &sample_list_kernel<true>},
       {"k22_count_long_weighted", &sample_count_long_kernel}, {"k22_entries_weighted", &sample_entries_kernel},
       {"k22_select_wave_weighted", &sample_select_wave_kernel<true>}, {"k22_select_block_weighted", &sample_select_block_kernel<true>}},
      "k22_count, k22_verify, k22_list, k22_select_wave, k22_select_block, k22_clear_dst, k22_sources, k22_relabel; k22_count_weighted, "
      "k22_list_weighted, k22_count_long_weighted, k22_entries_weighted, k22_select_wave_weighted, k22_select_block_weighted",
      regs, scratch);
}

}  // namespace pygat

using namespace pygat;

extern "C" int pygat_sample_workspace_bytes(int n, int n_dst, size_t* bytes) {
  PYGAT_REQUIRE(bytes, "sample_workspace_bytes: null bytes");
  PYGAT_REQUIRE(n > 0 && n_dst > 0 && n_dst <= n, "sample_workspace_bytes: n=%d nodes, n_dst=%d: 1 <= n_dst <= n expected", n, n_dst);
  *bytes = (size_t)sample_ws(n, n_dst).total * sizeof(int32_t);
  return PYGAT_OK;
}

// the passes of pygat_sample_block (weight == nullptr) and pygat_weighted_block, in the order the head of this file gives
template <bool WEIGHTED>
static int sample_block_launch(const char* what, int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int n_dst,
                               const int64_t* dst, int fanout, const float* weight, const void* seed, uint32_t hop, int64_t cap,
                               int64_t src_cap, int32_t* blk_rowptr, int32_t* blk_col, int32_t* edge_rc, int64_t* edge_ids,
                               int64_t* src_nodes, int32_t* info, void* ws, void* stream) {
  PYGAT_PASS(require_graph(what, n, nnz));
  PYGAT_REQUIRE(n_dst > 0 && n_dst <= n, "%s: n_dst=%d: 1 <= n_dst <= n = %d expected (distinct node ids)", what, n_dst, n);
  PYGAT_REQUIRE(fanout > 0, "%s: fanout=%d: a fanout >= 1 expected (INT32_MAX keeps whole rows)", what, fanout);
  PYGAT_PASS(require_tables(what, {{rowptr, "rowptr"}, {col, "col"}, {dst, "dst"}, {seed, "seed"}, {blk_rowptr, "blk_rowptr"},
                                   {blk_col, "blk_col"}, {edge_rc, "edge_rc"}, {edge_ids, "edge_ids"}, {src_nodes, "src_nodes"},
                                   {info, "info"}, {ws, "workspace"}}));
  if constexpr (WEIGHTED) {
    PYGAT_REQUIRE(weight, "%s: null weight", what);
    PYGAT_REQUIRE((reinterpret_cast<uintptr_t>(weight) & 3u) == 0, "%s: weight must be 4-byte aligned", what);
  }
  PYGAT_REQUIRE(aligned8(seed), "%s: seed must be 8-byte aligned", what);
  PYGAT_REQUIRE(aligned8(dst) && aligned8(edge_ids) && aligned8(src_nodes), "%s: dst, edge_ids and src_nodes must be 8-byte aligned", what);
  PYGAT_REQUIRE(aligned16(ws), "%s: the workspace must be 16-byte aligned", what);
  PYGAT_REQUIRE(cap > 0 && cap < ((int64_t)1 << 31), "%s: cap=%lld: room for 1 <= cap < 2^31 entries expected", what, (long long)cap);
  PYGAT_REQUIRE(src_cap >= n_dst, "%s: src_cap=%lld is below n_dst=%d", what, (long long)src_cap, n_dst);

  const SampleWs w = sample_ws(n, n_dst);
  int32_t* base = (int32_t*)ws;
  int32_t *marker = base + w.marker, *mark = base + w.mark, *rank = base + w.rank, *cnt = base + w.cnt, *lflag = base + w.lflag,
          *lptr = base + w.lptr, *llist = base + w.llist;
  void* tiles = base + w.tiles;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t* seedp = (const uint64_t*)seed;
  const dim3 rows((unsigned)cdiv(n_dst, 256)), tpb(256);
  const dim3 longs = long_grid(n_dst);

  PYGAT_PASS(clear_async(what, mark, (size_t)n * sizeof(int32_t), st));
  PYGAT_PASS(clear_async(what, info, (WEIGHTED ? 5 : 4) * sizeof(int32_t), st));
  hipLaunchKernelGGL(sample_count_kernel<WEIGHTED>, rows, tpb, 0, st, n, rowptr, n_dst, dst, fanout, weight, marker, cnt, lflag,
                     src_nodes, info);
  hipLaunchKernelGGL(sample_verify_kernel, rows, tpb, 0, st, n, n_dst, dst, marker, info);
  PYGAT_CHECK_LAUNCH(what);
  if constexpr (WEIGHTED) {
    PYGAT_PASS(pygat_exclusive_scan_i32(lflag, n_dst, lptr, tiles, stream));
    hipLaunchKernelGGL(sample_list_kernel<true>, rows, tpb, 0, st, n_dst, lflag, lptr, blk_rowptr, llist, info);
    hipLaunchKernelGGL(sample_count_long_kernel, longs, tpb, 0, st, n, rowptr, n_dst, dst, fanout, weight, lptr, llist, cnt, info);
    PYGAT_CHECK_LAUNCH(what);
    PYGAT_PASS(pygat_exclusive_scan_i32(cnt, n_dst, blk_rowptr, tiles, stream));
    hipLaunchKernelGGL(sample_entries_kernel, dim3(1), dim3(64), 0, st, n_dst, blk_rowptr, info);
  } else {
    PYGAT_PASS(pygat_exclusive_scan_i32(cnt, n_dst, blk_rowptr, tiles, stream));
    PYGAT_PASS(pygat_exclusive_scan_i32(lflag, n_dst, lptr, tiles, stream));
    hipLaunchKernelGGL(sample_list_kernel<false>, rows, tpb, 0, st, n_dst, lflag, lptr, blk_rowptr, llist, info);
  }
  hipLaunchKernelGGL(sample_select_wave_kernel<WEIGHTED>, dim3((unsigned)cdiv(n_dst, 4)), tpb, 0, st, n, rowptr, col, n_dst, dst, fanout,
                     weight, seedp, hop, cap, blk_rowptr, edge_ids, mark, info);
  hipLaunchKernelGGL(sample_select_block_kernel<WEIGHTED>, longs, tpb, 0, st, n, rowptr, col, n_dst, dst, fanout, weight, seedp, hop, cap,
                     blk_rowptr, lptr, llist, edge_ids, mark, info);
  hipLaunchKernelGGL(sample_clear_dst_kernel, rows, tpb, 0, st, n, n_dst, dst, mark);
  PYGAT_CHECK_LAUNCH(what);
  PYGAT_PASS(pygat_exclusive_scan_i32(mark, n, rank, tiles, stream));
  hipLaunchKernelGGL(sample_sources_kernel, dim3((unsigned)cdiv(n, 256)), tpb, 0, st, n, n_dst, mark, rank, src_cap, src_nodes, info);
  hipLaunchKernelGGL(sample_relabel_kernel, dim3((unsigned)cdiv(cap, 256)), tpb, 0, st, nnz, col, n_dst, dst, cap, blk_rowptr, marker,
                     rank, edge_ids, blk_col, edge_rc, info);
  PYGAT_CHECK_LAUNCH(what);
  return PYGAT_OK;
}

extern "C" int pygat_sample_block(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int n_dst, const int64_t* dst,
                                  int fanout, const void* seed, uint32_t hop, int64_t cap, int64_t src_cap, int32_t* blk_rowptr,
                                  int32_t* blk_col, int32_t* edge_rc, int64_t* edge_ids, int64_t* src_nodes, int32_t* info, void* ws,
                                  void* stream) {
  return sample_block_launch<false>("sample_block", n, nnz, rowptr, col, n_dst, dst, fanout, nullptr, seed, hop, cap, src_cap, blk_rowptr,
                                    blk_col, edge_rc, edge_ids, src_nodes, info, ws, stream);
}

extern "C" int pygat_weighted_block(int n, int64_t nnz, const int32_t* rowptr, const int32_t* col, int n_dst, const int64_t* dst,
                                    int fanout, const float* weight, const void* seed, uint32_t hop, int64_t cap, int64_t src_cap,
                                    int32_t* blk_rowptr, int32_t* blk_col, int32_t* edge_rc, int64_t* edge_ids, int64_t* src_nodes,
                                    int32_t* info, void* ws, void* stream) {
  return sample_block_launch<true>("weighted_block", n, nnz, rowptr, col, n_dst, dst, fanout, weight, seed, hop, cap, src_cap, blk_rowptr,
                                   blk_col, edge_rc, edge_ids, src_nodes, info, ws, stream);
}
