// The stage-2 task loss (--loss, Solver.py:172-192, applied at :334-335) and its gradient dL/dpred as a device function of ONE workgroup:
// the stand-alone task_loss_kernel (engine_kernels.hip) and the stage boundary (stage_boundary.h) -- its own launch or workgroup 0 of the
// critic clip + Adam launch -- call it.  The kind is a template parameter chosen on the host when the step is enqueued or captured: no
// per-row branch on the kind, and the MAE instantiation does the MAE-only engine's arithmetic in its order (bit-identical results).  fp32
// throughout, every reduction in the fixed order of block_sum; means and variances divide by B.  The batch-coupled kinds (RMSE, SIMSE,
// CCC) finish their reductions before the first dpred store; block_sum's barriers make every pass see the previous one.
// class_loss_body below: the classification losses (MIMRL_CLASS_LOSS_*), instantiated at the same sites.
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

// The classification losses of --task classification (Solver.py:172-178, applied with the reshapes of :324-333) under the same rules: one
// workgroup, fp32, block_sum's fixed order, the BOUNDARY form's store behind a barrier, every batch-coupled reduction (Focal's mean cross
// entropy) finished before the first dlogits store.  logits [B, C] row-major, C <= MIMRL_MAX_CLASSES; y [B] the class index held as a float
// (BCE with C == 1: the target itself, 0 or 1).  A thread owns whole rows.  expf / logf / log1pf, every exponent <= 0: finite at logits of
// +-80.  A label that is no integer in [0, C) (BCE, C == 1: neither 0 nor 1) is never used as an index; its row contributes NaN to the
// loss and gets NaN gradients.
//   CE    nn.CrossEntropyLoss: mean_b(log sum_c exp(x_c - m) - (x_y - m)), m = max_c x_c (torch's log_softmax order); d = (softmax - onehot) / B
//   Focal Utils.py:638-649 puts the focal factor on the batch-MEAN cross entropy: ce as above, p = exp(-ce), L = (1 - p)^2 ce,
//         dL/dce = 2 (1 - p) p ce + (1 - p)^2, d = dL/dce (softmax - onehot) / B
//   BCE   nn.BCEWithLogitsLoss over all B C elements, target = onehot(y) (C == 2, Solver.py:327-330) or y (C == 1, :331-333):
//         max(x, 0) - x t + log1p(exp(-|x|)); d = (sigmoid(x) - t) / (B C)
template <int KIND, bool BOUNDARY>
__device__ __forceinline__ void class_loss_body(const float* __restrict__ logits, const float* __restrict__ y, float* __restrict__ dlogits,
                                                float* __restrict__ out, int B, int C, float* red) {
  constexpr bool SYNC = BOUNDARY;
  constexpr int MAXC = MIMRL_MAX_CLASSES;
  const bool grad = BOUNDARY || dlogits;
  static_assert(KIND >= MIMRL_CLASS_LOSS_CE && KIND <= MIMRL_CLASS_LOSS_BCE, "classification loss kind");
  if (C > MAXC) C = MAXC;                                   // (the host refuses it; the row registers below hold MAXC values)
  const float nan = __builtin_nanf("");
  if constexpr (KIND == MIMRL_CLASS_LOSS_BCE) {
    const float inv = 1.f / ((float)B * (float)C);
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float yv = y[b];
      const int yi = (int)(yv >= 0.f && yv < (float)MAXC ? yv : -1.f);
      const bool ok = yi >= 0 && (float)yi == yv && (C == 1 ? yi <= 1 : yi < C);
      for (int c = 0; c < C; ++c) {
        const float x = logits[(long)b * C + c];
        const float t = C == 1 ? yv : (c == yi ? 1.f : 0.f);
        const float e = expf(-fabsf(x));
        s += ok ? fmaxf(x, 0.f) - x * t + log1pf(e) : nan;
        if (grad) {
          const float sg = x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
          dlogits[(long)b * C + c] = ok ? (sg - t) * inv : nan;
        }
      }
    }
    s = block_sum(s, red);
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = s / ((float)B * (float)C);
  } else {
    float s = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
      const float yv = y[b];
      const int yi = (int)(yv >= 0.f && yv < (float)MAXC ? yv : -1.f);
      const bool ok = yi >= 0 && (float)yi == yv && yi < C;
      float m = -INFINITY, xy = 0.f;
      for (int c = 0; c < C; ++c) { const float x = logits[(long)b * C + c]; m = fmaxf(m, x); xy = c == yi ? x : xy; }
      float se = 0.f;
      for (int c = 0; c < C; ++c) se += expf(logits[(long)b * C + c] - m);
      s += ok ? logf(se) - (xy - m) : nan;
    }
    const float ce = block_sum(s, red) / B;
    float val = ce, g = 1.f / B;
    if constexpr (KIND == MIMRL_CLASS_LOSS_FOCAL) {
      const float p = expf(-ce), q = 1.f - p;
      val = q * q * ce;
      g = (2.f * q * p * ce + q * q) / B;
    }
    if (grad) {
      for (int b = threadIdx.x; b < B; b += blockDim.x) {
        const float yv = y[b];
        const int yi = (int)(yv >= 0.f && yv < (float)MAXC ? yv : -1.f);
        const bool ok = yi >= 0 && (float)yi == yv && yi < C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) m = fmaxf(m, logits[(long)b * C + c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(logits[(long)b * C + c] - m);
        const float lg = logf(se);
        for (int c = 0; c < C; ++c) {
          const float sm = expf(logits[(long)b * C + c] - m - lg);
          dlogits[(long)b * C + c] = ok ? g * (sm - (c == yi ? 1.f : 0.f)) : nan;
        }
      }
    }
    if constexpr (SYNC) __syncthreads();
    if (threadIdx.x == 0) *out = val;
  }
}

}  // namespace mimrl
