// mimrl_op_score_accum: fold one batch of predictions into a block of running score statistics (include/mimrl.h: MIMRL_SC_*), from which
// the host derives the reference's metric table (Utils.py:118-175 calc_metrics: MAE, Corr, Acc-7, Acc-5, two Acc-2 and two F1) or, for a
// classification head, accuracy and weighted F1 (Solver.py:345-356) -- without keeping the predictions of an epoch.
//
// One workgroup of 256 threads strides over the rows.  Regression takes two passes over pred / y (at most 2048 rows in the engine: both
// come from L2): pass 1 sums p, y and |p - y| in double and counts the hits, the batch means follow, pass 2 sums the centred squares and
// the centred product.  Thread 0 merges the batch into the running moments with Chan's pairwise formula.  Every sum is reduced by an
// xor butterfly inside each wave (all lanes end with the same bits), then over the four waves through LDS in wave order: no atomics, so the
// same calls give the same bits, in the default and in the deterministic build alike (det.hip: nothing to flush behind it).
// Classification counts confusion cells by ballot: lane c of every wave owns cell c.
#include "common.h"

namespace mimrl {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_MAX_ROWS = 1 << 20;
constexpr int SC_NCOUNT = 10;        // acc7, acc5, pos/neg cells 0..3, nneg/neg cells 0..3

__device__ __forceinline__ double sc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int sc_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// sum over the workgroup, the same bits in every thread; red = SC_WAVES slots of LDS (reusable once the call has returned)
template <class T>
__device__ __forceinline__ T sc_block_sum(T v, T* red) {
  v = sc_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  T r = red[0];
#pragma unroll
  for (int w = 1; w < SC_WAVES; ++w) r += red[w];
  return r;
}

__global__ void __launch_bounds__(SC_THREADS) score_accum_reg_kernel(const float* __restrict__ pred, const float* __restrict__ y, int n,
                                                                     double* accd, long long* acci) {
  __shared__ double redd[SC_WAVES];
  __shared__ int redi[SC_WAVES];
  double sp = 0.0, sy = 0.0, sa = 0.0;
  int cnt[SC_NCOUNT];
#pragma unroll
  for (int k = 0; k < SC_NCOUNT; ++k) cnt[k] = 0;
  for (int i = threadIdx.x; i < n; i += SC_THREADS) {
    const float pf = pred[i], yf = y[i];
    const double p = (double)pf, t = (double)yf;          // the host formula works on float64 images of the fp32 values
    sp += p; sy += t; sa += fabs(p - t);
    const bool pnan = pf != pf;
    // clip, then round half to even (rintf in the default rounding mode = np.round); fminf / fmaxf drop a NaN, hence the explicit test
    const bool ok = !pnan && yf == yf;
    cnt[0] += ok && rintf(fminf(fmaxf(pf, -3.f), 3.f)) == rintf(fminf(fmaxf(yf, -3.f), 3.f));
    cnt[1] += ok && rintf(fminf(fmaxf(pf, -2.f), 2.f)) == rintf(fminf(fmaxf(yf, -2.f), 2.f));
    const int tpos = yf > 0.f, tnn = yf >= 0.f;
    const int ppos = pnan ? 1 - tpos : (int)(pf > 0.f);   // a NaN prediction is the class the truth is not
    const int pnn = pnan ? 1 - tnn : (int)(pf >= 0.f);
    const int cpn = 2 * tpos + ppos, cnn = 2 * tnn + pnn;
    const bool nz = yf != 0.f;                            // -0.0 is a zero label; a NaN label is not
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      cnt[2 + k] += nz && cpn == k;
      cnt[6 + k] += cnn == k;
    }
  }
  const double mp = sc_block_sum(sp, redd) / (double)n;
  const double my = sc_block_sum(sy, redd) / (double)n;
  sa = sc_block_sum(sa, redd);
  double qp = 0.0, qy = 0.0, qc = 0.0;
  for (int i = threadIdx.x; i < n; i += SC_THREADS) {
    const double dp = (double)pred[i] - mp, dy = (double)y[i] - my;
    qp += dp * dp; qy += dy * dy; qc += dp * dy;
  }
  qp = sc_block_sum(qp, redd);
  qy = sc_block_sum(qy, redd);
  qc = sc_block_sum(qc, redd);
#pragma unroll
  for (int k = 0; k < SC_NCOUNT; ++k) cnt[k] = sc_block_sum(cnt[k], redi);
  if (threadIdx.x != 0) return;
  const long long na = acci[MIMRL_SC_N];
  if (na <= 0) {                                          // a zeroed block: the batch is the running state
    accd[MIMRL_SC_MEAN_P] = mp; accd[MIMRL_SC_MEAN_Y] = my;
    accd[MIMRL_SC_M2_P] = qp; accd[MIMRL_SC_M2_Y] = qy; accd[MIMRL_SC_C_PY] = qc;
    accd[MIMRL_SC_SUM_ABS] = sa;
  } else {                                                // Chan et al.: merge of two sets given their means and centred sums
    const double a = (double)na, b = (double)n, tot = a + b;
    const double dp = mp - accd[MIMRL_SC_MEAN_P], dy = my - accd[MIMRL_SC_MEAN_Y];
    const double w = a * b / tot;
    accd[MIMRL_SC_MEAN_P] += dp * (b / tot);
    accd[MIMRL_SC_MEAN_Y] += dy * (b / tot);
    accd[MIMRL_SC_M2_P] += qp + dp * dp * w;
    accd[MIMRL_SC_M2_Y] += qy + dy * dy * w;
    accd[MIMRL_SC_C_PY] += qc + dp * dy * w;
    accd[MIMRL_SC_SUM_ABS] += sa;
  }
  acci[MIMRL_SC_N] = (na > 0 ? na : 0) + n;
  acci[MIMRL_SC_ACC7] += cnt[0];
  acci[MIMRL_SC_ACC5] += cnt[1];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acci[MIMRL_SC_PN + k] += cnt[2 + k];
    acci[MIMRL_SC_NN + k] += cnt[6 + k];
  }
}

// C = num_class (1..8), CE = max(C, 2); cell = truth * CE + prediction < 64, cell 64 = a label outside [0, CE)
__global__ void __launch_bounds__(SC_THREADS) score_accum_cls_kernel(const float* __restrict__ logits, const float* __restrict__ y, int n,
                                                                     int C, long long* acci) {
  __shared__ int cells[SC_WAVES][MIMRL_MAX_CLASSES * MIMRL_MAX_CLASSES + 1];
  const int CE = C < 2 ? 2 : C, ncell = CE * CE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int mine = 0, ignored = 0;                              // count of cell `lane`; count of cell 64 (wave-uniform)
  for (int base = 0; base < n; base += SC_THREADS) {      // wave-uniform trip count: every lane takes part in the ballots
    const int i = base + threadIdx.x;
    int cell = -1;
    if (i < n) {
      const float r = rintf(y[i]);
      cell = 64;
      if (r >= 0.f && r < (float)CE) {                    // (false for a NaN label)
        const float* x = logits + (size_t)i * C;
        int best;
        if (C == 1) best = x[0] > 0.f;
        else {
          best = 0;
          float xb = x[0];
          for (int c = 1; c < C; ++c) {                   // the first maximum; a NaN counts as one (numpy's argmax)
            const float xc = x[c];
            if (xb == xb && (xc > xb || xc != xc)) { best = c; xb = xc; }
          }
        }
        cell = (int)r * CE + best;
      }
    }
    for (int c = 0; c < ncell; ++c) {
      const int k = __popcll(__ballot(cell == c));
      if (lane == c) mine += k;
    }
    ignored += __popcll(__ballot(cell == 64));
  }
  cells[wave][lane] = mine;
  if (lane == 0) cells[wave][64] = ignored;
  __syncthreads();
  if (threadIdx.x != 0) return;
  long long counted = 0;
  for (int c = 0; c < ncell; ++c) {
    long long s = 0;
    for (int w = 0; w < SC_WAVES; ++w) s += cells[w][c];
    acci[MIMRL_SC_CONF + c] += s;
    counted += s;
  }
  long long ig = 0;
  for (int w = 0; w < SC_WAVES; ++w) ig += cells[w][64];
  acci[MIMRL_SC_IGNORED] += ig;
  acci[MIMRL_SC_N] += counted;
}

}  // namespace mimrl

using namespace mimrl;

extern "C" int mimrl_op_score_accum(void* stream, int num_class, const float* pred, const float* y, int n, void* acc) {
  if (num_class < 0 || num_class > MIMRL_MAX_CLASSES)
    return set_error(MIMRL_ERR_ARG, "score_accum: num_class %d outside [0, %d] (0 = the regression table)", num_class, MIMRL_MAX_CLASSES);
  if (n < 1 || n > SC_MAX_ROWS) return set_error(MIMRL_ERR_ARG, "score_accum: %d rows outside [1, %d]", n, SC_MAX_ROWS);
  if (!pred || !y || !acc) return set_error(MIMRL_ERR_ARG, "score_accum: null argument");
  if (reinterpret_cast<uintptr_t>(acc) % 8 != 0 || (reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(y)) % 4 != 0)
    return set_error(MIMRL_ERR_ARG, "score_accum: acc must be 8-byte aligned, pred and y 4-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (num_class == 0)
    hipLaunchKernelGGL(score_accum_reg_kernel, dim3(1), dim3(SC_THREADS), 0, s, pred, y, n, static_cast<double*>(acc), static_cast<long long*>(acc));
  else
    hipLaunchKernelGGL(score_accum_cls_kernel, dim3(1), dim3(SC_THREADS), 0, s, pred, y, n, num_class, static_cast<long long*>(acc));
  LAUNCH_CHECK();
  return MIMRL_OK;
}
