// Counter-based dropout decisions shared by the dropout kernels (k7_dropout.hip) and the sparse-feature projection
// (k9_sparse.hip): Philox-4x32-10 keyed by a seed in DEVICE memory.  Two counter layouts, neither part of the C ABI:
//   draw4       one mask over a [rows x cols] table: decision (row, col) = word (col & 3) of
//               Philox(counter = (col >> 2, row, stream_id, tag), key = seed) < keep * 2^32  -- four COLUMNS per call;
//   draw_heads4 the per-head input masks (layers.py:34,132: every head drops its own copy of x): decision (row, col,
//               head h) = word (h & 3) of Philox(counter = (col, row, stream_id, h >> 2)) -- four HEADS per call, so
//               that the sparse kernels, which meet the non-zeros of x one (row, col) at a time, spend one call per
//               non-zero and four heads instead of one per head (the first layout cost them 4 x the Philox work).
// tests/philox_ref.py restates the generator, the keep rule of make_rng and the layouts (the flat one of k7_dropout.hip's
// mask kernels included) in NumPy, and tests/test_gpu_dropout_seeded.py compares the kernels with it bit for bit: a change
// of a layout changes that file in the same commit.
//   sample_keys4 the selection keys of the neighbour sampler (k22_sample.hip): key of the entry at CSR position p of the graph =
//               word (p & 3) of Philox(counter = (p >> 2, hop, STREAM_SAMPLE = 4, 0), key = seed) -- four POSITIONS per call; the
//               key depends on the position alone.  No other layout uses stream 4.  tests/sampler_ref.py restates it and
//               tests/test_gpu_sample.py compares the sampled blocks with it entry for entry.  The weighted sampler orders a row
//               by sample_weighted_key(that word, weight[p]) instead.
//   walk_keys4  the step keys of the random walk (k23_subgraph.hip): key of step t of walker w = word (t & 3) of Philox(counter =
//               (w, hop, STREAM_WALK = 5, t >> 2), key = seed) -- four STEPS of one walker per call.  No other layout uses stream 5.
//               tests/subgraph_ref.py restates it and tests/test_gpu_subgraph.py compares the walks with it entry for entry.
//   neg_keys4   the draw keys of the negative sampler (k24_linkpred.hip): key of the flat draw i = w * num_neg + s (draw s of source
//               w) = word (i & 3) of Philox(counter = (i >> 2, hop, STREAM_NEG = 6, 0), key = seed) -- four consecutive flat DRAWS
//               per call.  No other layout uses stream 6.  tests/linkpred_ref.py restates it and tests/test_gpu_linkpred.py compares
//               the draws with it integer for integer.
#pragma once
#include "common.h"

namespace pygat {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u; k.y += 0xBB67AE85u;
  }
  return c;
}

struct DropRng {
  const uint64_t* seed;  // device memory, [1]
  uint32_t stream_id;    // separates the masks drawn from one seed (input / Wh / attention, level)
  uint32_t thresh;       // keep iff word < thresh  (keep = 1 - p)
  float scale;           // 1 / keep
};

__device__ __forceinline__ uint32_t word_of(const uint4& w, int q) {
  return q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
}

// 4 decisions for (row, columns 4*c4 .. 4*c4+3)
__device__ __forceinline__ uint4 draw4(const DropRng& g, uint64_t seed, uint32_t row_lo, uint32_t row_hi, uint32_t c4) {
  return philox4x32_10(make_uint4(c4, row_lo, g.stream_id, row_hi), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// 4 decisions for (row, col, heads 4*hq .. 4*hq+3)
__device__ __forceinline__ uint4 draw_heads4(const DropRng& g, uint64_t seed, uint32_t row, uint32_t col, uint32_t hq) {
  return philox4x32_10(make_uint4(col, row, g.stream_id, hq), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}
__device__ __forceinline__ uint32_t keep_nibble(const DropRng& g, const uint4& w) {
  return (w.x < g.thresh ? 1u : 0u) | (w.y < g.thresh ? 2u : 0u) | (w.z < g.thresh ? 4u : 0u) | (w.w < g.thresh ? 8u : 0u);
}

// 4 selection keys of the sampler for CSR positions 4*q .. 4*q+3 at hop `hop`
constexpr uint32_t STREAM_SAMPLE = 4;
__device__ __forceinline__ uint4 sample_keys4(uint64_t seed, uint32_t q, uint32_t hop) {
  return philox4x32_10(make_uint4(q, hop, STREAM_SAMPLE, 0u), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// 4 step keys of the random walk (k23_subgraph.hip) for steps 4*tq .. 4*tq+3 of walker w at hop `hop`
constexpr uint32_t STREAM_WALK = 5;
__device__ __forceinline__ uint4 walk_keys4(uint64_t seed, uint32_t w, uint32_t hop, uint32_t tq) {
  return philox4x32_10(make_uint4(w, hop, STREAM_WALK, tq), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// 4 draw keys of the negative sampler (k24_linkpred.hip) for the flat draws 4*q .. 4*q+3 at hop `hop`
constexpr uint32_t STREAM_NEG = 6;
__device__ __forceinline__ uint4 neg_keys4(uint64_t seed, uint32_t q, uint32_t hop) {
  return philox4x32_10(make_uint4(q, hop, STREAM_NEG, 0u), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
}

// The weighted sampler's key of an entry with Philox word k and weight w > 0 (finite or +inf): the bits of the exponential clock
// E(k) / w, E(k) = -ln(1 - (k + 0.5) / 2^32), all in fp32.  Two branches keep the logarithm's condition number at or below 1.45 at
// every k (one log1pf(-u) alone loses 1e-4 relative near u -> 1).  E > 0, so the clock is a non-negative float (+0 at w = +inf, +inf
// where E / w overflows) and its bit pattern orders like it.  tests/sampler_weighted_ref.py restates the clock in fp64.
__device__ __forceinline__ uint32_t sample_weighted_key(uint32_t k, float w) {
  const float E = k < 0x80000000u ? -log1pf(-(((float)k + 0.5f) * 0x1p-32f)) : -logf(((float)(~k) + 0.5f) * 0x1p-32f);
  return __float_as_uint(E / w);
}

static inline bool make_rng(float p, const void* seed, uint32_t stream_id, DropRng* g) {
  if (!(p >= 0.f && p <= 1.f)) return false;   // p = 1 (F.dropout accepts it): nothing is kept, everything becomes 0
  const double keep = 1.0 - (double)p;
  double t = keep * 4294967296.0;
  g->seed = (const uint64_t*)seed;
  g->stream_id = stream_id;
  g->thresh = t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
  g->scale = keep > 0.0 ? (float)(1.0 / keep) : 0.f;
  return true;
}


}  // namespace pygat
