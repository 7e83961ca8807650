// The backward stream of the self-loop-only tail (k12_tail.hip) as a device function: pygat_gat_backward_tail runs it as a
// launch of its own, pygat_gat_backward_col_finish (k4_backward_col.hip) in the work-groups behind the column pass's fix-up.
#pragma once
#include "attn_common.h"

namespace pygat {

// Levels without a skip projection, whose weight gradient is the only other reader of Gp: dWh_j = Gp_j = G_u ELU'(out_u)
// straight from the caller's rows u = user_row[j] -- the tail's rows of GR are neither written (pygat_gat_backward_prepare
// runs on the rows before the tail) nor read.  ELU' is recovered from the output exactly as K3a does (out > 0 ? 1 : out + 1).
// idx: chunk of 4 floats, counted over the tail's rows.
__device__ __forceinline__ void bwd_tail_item(int64_t idx, int row_first, int n_rows, int H, int Fo, int Fp, int flags,
                                              const float* __restrict__ G, const float* __restrict__ y,
                                              const int32_t* __restrict__ urow, float* __restrict__ dWh, int64_t ld_dwh,
                                              int zero_cols, float* __restrict__ ds, float* __restrict__ dt) {
  const int R4 = H * Fp / 4;
  if (idx >= (int64_t)n_rows * R4) return;
  const int64_t j = row_first + idx / R4;
  const int co = 4 * (int)(idx % R4), h = co / Fp, f0 = co % Fp;
  const int64_t ju = urow ? (int64_t)urow[j] : j;
  float g[4] = {0.f, 0.f, 0.f, 0.f}, o[4] = {1.f, 1.f, 1.f, 1.f};
  if (Fo == Fp) {
    const float4 g4 = ld4(G + ju * (int64_t)(H * Fo) + co), y4 = ld4(y + ju * (int64_t)(H * Fo) + co);
    g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w; o[0] = y4.x; o[1] = y4.y; o[2] = y4.z; o[3] = y4.w;
  } else {
    const int64_t b = ju * (int64_t)(H * Fo) + (int64_t)h * Fo + f0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (f0 + q < Fo) { g[q] = G[b + q]; o[q] = y[b + q]; }
  }
  if (flags & PYGAT_F_ELU) {
#pragma unroll
    for (int q = 0; q < 4; ++q) g[q] *= o[q] > 0.f ? 1.f : o[q] + 1.f;
  }
  st4(dWh + j * ld_dwh + co, make_float4(g[0], g[1], g[2], g[3]));
  if (co < zero_cols) st4(dWh + j * ld_dwh + H * Fp + co, make_float4(0.f, 0.f, 0.f, 0.f));   // (GATv2: the dWhj half of the row)
  if (f0 == 0) { if (dt) dt[j * H + h] = 0.f; if (ds) ds[j * H + h] = 0.f; }
}

}  // namespace pygat
