// The long-row rule of the kernels that walk a CSR one lane group (K15, K17, K18) or one wave (K14) per row.  A row of more than
// LONG_ROW entries would serialise on its owner, so it is summed in two launches.  Launch 1 cuts the ENTRY array into chunks of
// LONG_CHUNK entries, one work-group per chunk, which sums the piece of every long row that meets its chunk into partial record
// chunk * LONG_SLOTS + slot.  At most LONG_SLOTS long rows meet a chunk: one that runs in from the chunk before (slot 0) and
// LONG_CHUNK / LONG_ROW that start inside it -- long rows start more than LONG_ROW entries apart, so the one that starts at offset
// d of the chunk has slot 1 + d / LONG_ROW to itself.  In launch 2 the owner of a long row adds the row's records in chunk order.
// A record's payload, the sum of a piece and the merge of two records are each kernel's own.  Every order is fixed: same bits.
#pragma once
#include "common.h"

namespace pygat {
constexpr int LONG_CHUNK = 2048, LONG_ROW = 512, LONG_SLOTS = LONG_CHUNK / LONG_ROW + 1;

// grid of launch 1, and the records a workspace holds (one chunk's worth for a pattern without entries: never an empty workspace)
static inline int64_t long_chunks(int64_t nnz) { return cdiv(nnz, LONG_CHUNK); }
static inline int64_t long_records(int64_t nnz) { return (nnz > 0 ? long_chunks(nnz) : 1) * LONG_SLOTS; }
#ifdef __HIPCC__
struct LongChunk { int64_t c0, c1; };   // entries [c0, c1) of a chunk
__device__ __forceinline__ LongChunk long_chunk_span(int64_t chunk, int64_t nnz) {
  const int64_t c0 = chunk * LONG_CHUNK;
  return LongChunk{c0, c0 + LONG_CHUNK < nnz ? c0 + LONG_CHUNK : nnz};
}
// slot of the piece, in the chunk that begins at entry c0, of the long row that begins at `start`; its record (x the caller's stride)
__device__ __forceinline__ int long_piece_slot(int64_t start, int64_t c0) { return start < c0 ? 0 : 1 + (int)((start - c0) / LONG_ROW); }
__device__ __forceinline__ int64_t long_record(int64_t chunk, int slot) { return chunk * LONG_SLOTS + slot; }
// the row that holds entry e: the last r with rowptr[r] <= e (rows without entries are passed over)
__device__ __forceinline__ int row_of(const int32_t* rowptr, int n, int64_t e) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// Launch 1, every wave of the chunk's work-group: the long rows among [r_first, r_last], the rows of the chunk's first and last
// entry, screened 64 per step (a lane each, one ballot).  f(row, start, end, e0, e1, slot), wave-uniform, for each long row in
// ascending order: [start, end) the row's entries, [e0, e1) those inside the chunk.  One flat loop with the screen as its refill,
// the screened row = base + lane number by mbcnt: f sits one loop deep and no vector register is held through it (K15 has none).
template <class F>
__device__ __forceinline__ void for_long_rows(const int32_t* rowptr, int r_first, int r_last, const LongChunk& c, F&& f) {
  int base = r_first - 64;
  unsigned long long todo = 0;                            // long rows among [base, base + 64) not yet handed out
  for (;;) {                                              // (uniform in the wave)
    while (!todo && (base += 64) <= r_last) {
      const int r = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, base));
      todo = __ballot(r <= r_last && rowptr[r + 1] - rowptr[r] > LONG_ROW);
    }
    if (!todo) break;
    const int row = base + (__ffsll((long long)todo) - 1);
    todo &= todo - 1;
    const int64_t start = rowptr[row], end = rowptr[row + 1];
    f(row, start, end, start > c.c0 ? start : c.c0, end < c.c1 ? end : c.c1, long_piece_slot(start, c.c0));
  }
}

// Launch 2, the owner of the long row [start, end): f(record number) for each of the row's records, in chunk order
template <class F>
__device__ __forceinline__ void for_long_records(int64_t start, int64_t end, F&& f) {
  for (int64_t c = start / LONG_CHUNK; c <= (end - 1) / LONG_CHUNK; ++c) f(long_record(c, long_piece_slot(start, c * LONG_CHUNK)));
}
#endif
}  // namespace pygat
