// Stand-alone check of the L-axis descriptor builders of csrc/gemm.h (built and run by tests/test_gemm_builders.py with
// -fsanitize=address,undefined; no GPU call).  Every expected descriptor is spelled out field by field for ONE shape whose sizes are
// all distinct -- B = 4 samples, il = 5, hl = 7, ol = 3, ik = 2, id = 3 (so C = 6), padded fc2 pitch 8 -- so that a swapped argument
// shows; same() then compares EVERY field, so whatever a builder does not own must still be the GemmDesc default.
#include <cstdio>

#include "gemm.h"

using mimrl::GemmDesc;

static int failures = 0;
#define FIELD(f) \
  do { if (!(got.f == want.f)) { std::printf("FAILED %s: field %s\n", what, #f); ++failures; } } while (0)

// field by field, not memcmp: the struct has padding
static void same(const char* what, const GemmDesc& got, const GemmDesc& want) {
  FIELD(A); FIELD(B); FIELD(C); FIELD(M); FIELD(N); FIELD(K); FIELD(batch);
  FIELD(sa_m); FIELD(sa_k); FIELD(sa_b); FIELD(sb_k); FIELD(sb_n); FIELD(sb_b); FIELD(sc_m); FIELD(sc_n); FIELD(sc_b);
  FIELD(batch_in); FIELD(sa_bo); FIELD(sb_bo); FIELD(sc_bo); FIELD(bias_n_bo);
  FIELD(a_gap_at); FIELD(a_gap_rows);
  FIELD(bias_n); FIELD(bias_n_b); FIELD(bias_m); FIELD(bias_m_b);
  FIELD(alpha); FIELD(beta); FIELD(act); FIELD(pre); FIELD(gradact_u); FIELD(atomic); FIELD(colsum); FIELD(colsum_b);
  FIELD(A2); FIELD(B2); FIELD(K2); FIELD(sa2_m); FIELD(sa2_k); FIELD(sa2_b); FIELD(sb2_k); FIELD(sb2_n); FIELD(sb2_b);
  FIELD(a_pad4); FIELD(a_bf16); FIELD(b_bf16); FIELD(b_f16cvt); FIELD(f16); FIELD(c_f16); FIELD(c_bf16);
}
// a field added to GemmDesc belongs in same() too
static_assert(sizeof(GemmDesc) == 352, "GemmDesc changed: list the new field in same() and update this size");

int main() {
  // operands: only the addresses matter
  static float W1[7 * 5], W2[3 * 7], W2p[3 * 8], Wr[3 * 5], X[4 * 5 * 6], H[4 * 7 * 6], Y[4 * 3 * 6];
  static float dY[4 * 3 * 6], dU[4 * 7 * 6], dX[4 * 5 * 6], dW1[7 * 5], dW2[3 * 7], dWr[3 * 5];
  const int B = 4, il = 5, hl = 7, ol = 3;
  const long C = 6;

  {   // fc1: H_b[hl, C] = W1[hl, il] . X_b[il, C]
    GemmDesc e;
    e.A = W1; e.B = X; e.C = H; e.M = 7; e.N = 6; e.K = 5; e.batch = 4;
    e.sa_m = 5; e.sa_k = 1; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 30; e.sc_m = 6; e.sc_n = 1; e.sc_b = 42;
    same("gemm_lmul fc1", mimrl::gemm_lmul(W1, il, X, H, hl, il, C, B), e);
  }
  {   // fc2 from the padded copy (row pitch 8), then + Wr[ol, il] . X_b[il, C] as the second product
    GemmDesc e;
    e.A = W2p; e.B = H; e.C = Y; e.M = 3; e.N = 6; e.K = 7; e.batch = 4;
    e.sa_m = 8; e.sa_k = 1; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 42; e.sc_m = 6; e.sc_n = 1; e.sc_b = 18;
    GemmDesc g = mimrl::gemm_lmul(W2p, 8, H, Y, ol, hl, C, B);
    same("gemm_lmul fc2 (pitch 8)", g, e);
    e.A2 = Wr; e.B2 = X; e.K2 = 5; e.sa2_m = 5; e.sa2_k = 1; e.sa2_b = 0; e.sb2_k = 6; e.sb2_n = 1; e.sb2_b = 30;
    mimrl::gemm_lmul_add(g, Wr, X, il);
    same("gemm_lmul_add fc2 + residual", g, e);
  }
  {   // the residual product alone: Y_b[ol, C] = Wr[ol, il] . X_b[il, C]
    GemmDesc e;
    e.A = Wr; e.B = X; e.C = Y; e.M = 3; e.N = 6; e.K = 5; e.batch = 4;
    e.sa_m = 5; e.sa_k = 1; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 30; e.sc_m = 6; e.sc_n = 1; e.sc_b = 18;
    same("gemm_lmul residual", mimrl::gemm_lmul(Wr, il, X, Y, ol, il, C, B), e);
  }
  {   // dU_b[hl, C] = W2[ol, hl]^T . dY_b[ol, C], from the parameters (pitch 7) and from the padded copy (pitch 8)
    GemmDesc e;
    e.A = W2; e.B = dY; e.C = dU; e.M = 7; e.N = 6; e.K = 3; e.batch = 4;
    e.sa_m = 1; e.sa_k = 7; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 18; e.sc_m = 6; e.sc_n = 1; e.sc_b = 42;
    same("gemm_lmul_t dU", mimrl::gemm_lmul_t(W2, hl, dY, dU, hl, ol, C, B), e);
    e.A = W2p; e.sa_k = 8;
    same("gemm_lmul_t dU (pitch 8)", mimrl::gemm_lmul_t(W2p, 8, dY, dU, hl, ol, C, B), e);
  }
  {   // dX_b[il, C] = W1[hl, il]^T . dU_b[hl, C], then + Wr[ol, il]^T . dY_b[ol, C] as the second product
    GemmDesc e;
    e.A = W1; e.B = dU; e.C = dX; e.M = 5; e.N = 6; e.K = 7; e.batch = 4;
    e.sa_m = 1; e.sa_k = 5; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 42; e.sc_m = 6; e.sc_n = 1; e.sc_b = 30;
    GemmDesc g = mimrl::gemm_lmul_t(W1, il, dU, dX, il, hl, C, B);
    same("gemm_lmul_t dX", g, e);
    e.A2 = Wr; e.B2 = dY; e.K2 = 3; e.sa2_m = 1; e.sa2_k = 5; e.sa2_b = 0; e.sb2_k = 6; e.sb2_n = 1; e.sb2_b = 18;
    mimrl::gemm_lmul_t_add(g, Wr, dY, ol);
    same("gemm_lmul_t_add dX + residual", g, e);
  }
  {   // the residual product alone: dX_b[il, C] = Wr[ol, il]^T . dY_b[ol, C]
    GemmDesc e;
    e.A = Wr; e.B = dY; e.C = dX; e.M = 5; e.N = 6; e.K = 3; e.batch = 4;
    e.sa_m = 1; e.sa_k = 5; e.sa_b = 0; e.sb_k = 6; e.sb_n = 1; e.sb_b = 18; e.sc_m = 6; e.sc_n = 1; e.sc_b = 30;
    same("gemm_lmul_t residual", mimrl::gemm_lmul_t(Wr, il, dY, dX, il, ol, C, B), e);
  }
  {   // dW2[ol, hl] += sum_b dY_b[ol, C] . H_b[hl, C]^T
    GemmDesc e;
    e.A = dY; e.B = H; e.C = dW2; e.M = 3; e.N = 7; e.K = 6; e.batch = 4;
    e.sa_m = 6; e.sa_k = 1; e.sa_b = 18; e.sb_k = 1; e.sb_n = 6; e.sb_b = 42; e.sc_m = 7; e.sc_n = 1; e.sc_b = 0;
    e.atomic = 1;
    same("gemm_lmul_dw dW2", mimrl::gemm_lmul_dw(dY, H, dW2, ol, hl, C, B), e);
  }
  {   // dWr[ol, il] += sum_b dY_b[ol, C] . X_b[il, C]^T
    GemmDesc e;
    e.A = dY; e.B = X; e.C = dWr; e.M = 3; e.N = 5; e.K = 6; e.batch = 4;
    e.sa_m = 6; e.sa_k = 1; e.sa_b = 18; e.sb_k = 1; e.sb_n = 6; e.sb_b = 30; e.sc_m = 5; e.sc_n = 1; e.sc_b = 0;
    e.atomic = 1;
    same("gemm_lmul_dw dWr", mimrl::gemm_lmul_dw(dY, X, dWr, ol, il, C, B), e);
  }
  {   // dW1[hl, il] += sum_b dU_b[hl, C] . X_b[il, C]^T
    GemmDesc e;
    e.A = dU; e.B = X; e.C = dW1; e.M = 7; e.N = 5; e.K = 6; e.batch = 4;
    e.sa_m = 6; e.sa_k = 1; e.sa_b = 42; e.sb_k = 1; e.sb_n = 6; e.sb_b = 30; e.sc_m = 5; e.sc_n = 1; e.sc_b = 0;
    e.atomic = 1;
    same("gemm_lmul_dw dW1", mimrl::gemm_lmul_dw(dU, X, dW1, hl, il, C, B), e);
  }
  if (failures == 0) std::printf("gemm builders ok\n");
  return failures == 0 ? 0 : 1;
}
