// Device helpers of the two "bookends" of a forward tail's CubeMLP stack: the pre-CubeMLP row arithmetic (text dropout | fwd + bwd half ->
// LayerNorm over 128 -> ReLU -> dropout, and the temporal means: Model.py:452-466) and the head reduction (Model.py:489-515).  Both exist
// as launches of their own (model_ops.hip: tail_pre_kernel, head_fwd_kernel) and as the PRE / HEAD modes of cube_fwd_fused_kernel
// (cube_fused.hip), where the workgroup of a sample already holds the data.  Every site calls THESE functions, so the two forms compile the
// same expression trees and their outputs are compared bit for bit (tests/test_gpu_cube_bookends.py).
// Row helpers: one wave per row, lane l owns columns l and l + 64; all 64 lanes active (wave_sum).
#pragma once
#include "kmix_device.h"

namespace mimrl {
namespace {

// text row r = b * T + t: x * dropout scale (stream 0, element index r * 128 + column)
__device__ __forceinline__ void pre_text_row(float x0, float x1, float p, const RngKey& key, uint32_t rstep, long r, int lane, float& y0, float& y1) {
  constexpr int D = 128;
  y0 = x0 * drop_scale_at(p, key, rstep, 0u, (uint32_t)(r * D + lane));
  y1 = x1 * drop_scale_at(p, key, rstep, 0u, (uint32_t)(r * D + lane + 64));
}
// encoder row r: v = forward half + backward half -> LayerNorm over 128 -> ReLU -> dropout scale (the modality's stream id)
__device__ __forceinline__ void pre_ln_row(float v0, float v1, float g0, float g1, float be0, float be1, float p, const RngKey& key, uint32_t rstep,
                                           uint32_t stream, long r, int lane, float& mu, float& rs, float& y0, float& y1) {
  constexpr int D = 128;
  mu = wave_sum(v0 + v1) * (1.f / D);
  const float c0 = v0 - mu, c1 = v1 - mu;
  rs = rsqrtf(wave_sum(c0 * c0 + c1 * c1) * (1.f / D) + LN_EPS);
  y0 = c0 * rs * g0 + be0; y1 = c1 * rs * g1 + be1;
  y0 = (y0 > 0.f ? y0 : 0.f) * drop_scale_at(p, key, rstep, stream, (uint32_t)(r * D + lane));
  y1 = (y1 > 0.f ? y1 : 0.f) * drop_scale_at(p, key, rstep, stream, (uint32_t)(r * D + lane + 64));
}
// temporal mean of one (slot, column) from its four time-phase sums (phase q = rows t = q, q + 4, ... added in increasing t)
__device__ __forceinline__ float pre_mean(float p0, float p1, float p2, float p3, int T) { return (p0 + p1 + p2 + p3) / T; }

// head, 512 threads = 128 columns x 4 row phases: phase q of column d adds rows i = q, q + 4, ... < n in increasing order
__device__ __forceinline__ float head_phase_sum(const float* xcol, long ld, int q, int n) {
  float s = 0.f;
#pragma unroll 8
  for (int i = q; i < n; i += 4) s += xcol[(long)i * ld];
  return s;
}
// ... then F_F[d] = ((p0 + p1) + (p2 + p3)) * scale and pred[c] = sum_d F_F[d] * w[c * 128 + d] + bias[c] for the C outputs of the head
// (pred: this sample's row of [B, C]).  Called by all 512 threads behind the barrier that publishes ph; red: >= 16 floats of LDS.  One
// block_sum per class: class 0 is the one-output head's expression tree and reduction, the further classes follow it.
__device__ __forceinline__ void head_finish(const float (*ph)[128], const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ ff_row,
                                            float* __restrict__ pred, float scale, float* red, int C) {
  const int d = threadIdx.x & 127, q = threadIdx.x >> 7;
  float part = 0.f, s = 0.f;
  if (q == 0) {
    s = ((ph[0][d] + ph[1][d]) + (ph[2][d] + ph[3][d])) * scale;
    ff_row[d] = s;
    part = s * w[d];
  }
  part = block_sum(part, red);
  if (threadIdx.x == 0) *pred = part + bias[0];
  for (int c = 1; c < C; ++c) {
    part = q == 0 ? s * w[c * 128 + d] : 0.f;
    part = block_sum(part, red);
    if (threadIdx.x == 0) pred[c] = part + bias[c];
  }
}

}  // namespace
}  // namespace mimrl
