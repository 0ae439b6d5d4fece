// The stage-2 task loss (--loss, Solver.py:172-192, applied at :334-335) and its gradient dL/dpred as a device function of ONE workgroup:
// the stand-alone task_loss_kernel (engine_kernels.hip) and the stage boundary (stage_boundary.h) -- its own launch or workgroup 0 of the
// critic clip + Adam launch -- call it.  The kind is a template parameter chosen on the host when the step is enqueued or captured: no
// per-row branch on the kind, and the MAE instantiation does the MAE-only engine's arithmetic in its order (bit-identical results).  fp32
// throughout, every reduction in the fixed order of block_sum; means and variances divide by B.  The batch-coupled kinds (RMSE, SIMSE,
// CCC) finish their reductions before the first dpred store; block_sum's barriers make every pass see the previous one.
#pragma once
#include "common.h"

namespace mimrl {

// all threads of one workgroup (blockDim.x a multiple of 64, <= 1024); `red`: 16 floats of LDS.  Writes dpred[0, B) and the loss value
// to *out (thread 0).  BOUNDARY (the stage boundary): dpred is never null, and the store of the value waits behind a workgroup barrier
// (the boundary's zeroing of the stage-2 scalars is complete before the loss lands among them); otherwise dpred may be null.
template <int KIND, bool BOUNDARY>
__device__ __forceinline__ void task_loss_body(const float* __restrict__ pred, const float* __restrict__ y, float* __restrict__ dpred,
                                               float* __restrict__ out, int B, float* red) {
  constexpr bool SYNC = BOUNDARY;
  const bool grad = BOUNDARY || dpred;
  static_assert(KIND >= MIMRL_TASK_LOSS_MAE && KIND <= MIMRL_TASK_LOSS_CCC, "task loss kind");
  if constexpr (KIND == MIMRL_TASK_LOSS_MAE) {            // nn.L1Loss
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float d = pred[b] - y[b];
      s += fabsf(d);
      if (grad) dpred[b] = (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)) / B;
    }
    s = block_sum(s, red);
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = s / B;
  } else if constexpr (KIND == MIMRL_TASK_LOSS_MSE) {     // nn.MSELoss(reduction='mean')
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float d = pred[b] - y[b];
      s += d * d;
      if (grad) dpred[b] = 2.f * d / B;
    }
    s = block_sum(s, red);
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = s / B;
  } else if constexpr (KIND == MIMRL_TASK_LOSS_RMSE) {    // Utils.py:270-275: mean(d^2) ** 0.5
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float d = pred[b] - y[b];
      s += d * d;
    }
    const float r = sqrtf(block_sum(s, red) / B);
    if (grad) {
      // autograd's chain: 0.5 * m^-0.5 (inf at m = 0), / B, * 2d -- NaN in every row at a zero residual, as torch gives
      const float g = 0.5f / r / B;
      for (int b = threadIdx.x; b < B; b += blockDim.x) dpred[b] = 2.f * (pred[b] - y[b]) * g;
    }
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = r;
  } else if constexpr (KIND == MIMRL_TASK_LOSS_SIMSE) {   // Utils.py:459-468: (sum(y - pred))^2 / B^2
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) s += y[b] - pred[b];
    const float S = block_sum(s, red), n2 = (float)B * (float)B;
    if (grad) {
      const float g = -(2.f * S / n2);
      for (int b = threadIdx.x; b < B; b += blockDim.x) dpred[b] = g;
    }
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = S * S / n2;
  } else {                                                // Utils.py:22-34: 1 - 2 cov / (var_y + var_p + (mu_y - mu_p)^2 + 1e-10)
    float so = 0.f, st = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) { so += pred[b]; st += y[b]; }
    const float mo = block_sum(so, red) / B;
    const float mt = block_sum(st, red) / B;
    float c = 0.f, vt = 0.f, vo = 0.f;                    // second, centred pass
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float eo = pred[b] - mo, et = y[b] - mt;
      c += eo * et; vt += et * et; vo += eo * eo;
    }
    const float cov = block_sum(c, red) / B;
    const float var_t = block_sum(vt, red) / B;
    const float var_o = block_sum(vo, red) / B;
    const float dm = mt - mo;
    const float den = var_t + var_o + dm * dm + 1e-10f;
    if (grad) {
      // dcov/dp_b = (y_b - mu_y) / B, dden/dp_b = 2 (p_b - mu_y) / B
      const float ga = -2.f / den / B, gb = 4.f * cov / (den * den) / B;
      for (int b = threadIdx.x; b < B; b += blockDim.x) dpred[b] = ga * (y[b] - mt) + gb * (pred[b] - mt);
    }
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = 1.f - 2.f * cov / den;
  }
}

}  // namespace mimrl
