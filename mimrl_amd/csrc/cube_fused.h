// Fused CubeMLP block forward (MLPProcess.py:94-122, ln_last form): one workgroup per sample keeps the [L, K, 128] tile
// in LDS (bf16) through L-axis MLP+residual -> LayerNorm(L) -> K-axis mix -> D-axis MLP+residual -> LayerNorm(D).
#pragma once
#include "common.h"
#include "model_ops.h"

namespace mimrl {

// PRE mode (block 0 of a forward tail): the set-up section builds the sample tile from the encoder outputs instead of reading `x` -- what
// tail_pre_kernel did in a launch of its own, through an fp32 cube in HBM that this kernel then read back (cube_bookends.h holds the row arithmetic of both)
struct CubePre {
  const float* tx_raw;                 // text projection [B, T, 128]                         -> slot 0
  const float* h2[2];                  // audio / video encoder outputs [B, T, 256] (two halves) -> slots 1, 2 (dropout streams 1, 2)
  const float *gamma[2], *beta[2];     // their LayerNorm parameters
  float p[3];                          // dropout probabilities: text, audio, video
  float* feats;                        // temporal means [3][B][128]
  // the fp32 cube [B, il, 3, 128] (rows t >= T zero) and the LayerNorm statistics [B * T]: what the backward pass reads.  All null in a
  // tail nobody differentiates.
  float* cube; float *mean[2], *rstd[2];
  int T;                               // 1 <= T <= il
  RngKey key;
};
// HEAD mode (last block, ol * K <= 64): the LayerNorm(D) epilogue keeps its rows in the LDS tile and the workgroup finishes head_fwd_kernel's
// reduction over them: ff[b, :] and pred[b]
struct CubeHead { const float *w, *bias; float *ff, *pred; float scale; int C; };   // C: outputs of the head (w [C, 128], pred [B, C])

struct CubeFusedArgs {
  const float* x;                                              // block input  [B, il, K, 128]
  const float *l_w1, *l_b1, *l_w2, *l_b2, *l_wr, *l_g, *l_be;  // L axis: [hl,il] [hl] [ol,hl] [ol] [ol,il] [ol] [ol]
  KMixW kw;                                                    // K axis (ik == hk == ok == K)
  const float *d_w1, *d_b1, *d_w2, *d_b2, *d_wr, *d_g, *d_be;  // D axis: 128x128 each
  // activations kept for the backward pass (all null when save == 0); same buffers/layouts as the unfused path
  float *l_u, *l_h, *l_y, *l_z, *l_mean, *l_rstd;              // [B,hl,C] [B,hl,C] [B,ol,C] [B,ol,C] [B,C] [B,C]
  float* k_z;                                                  // [B, ol, K, 128]
  float *d_u, *d_h, *d_y, *d_mean, *d_rstd;                    // [B*ol*K, 128] x3, [B*ol*K] x2
  float* d_z;                                                  // block output [B, ol, K, 128]
  int B, il, hl, ol, K, act, save;
  int dbg_phase;                                               // tuning only: stop after phase n (0 = run everything)
  int pre_on, head_on;                                         // the two modes above (two wave groups only)
  CubePre pre; CubeHead head;
};

// true if this block's configuration is covered by the fused kernel (else the engine uses the unfused path)
bool cube_fused_supported(int il, int hl, int ol, int ik, int hk, int ok, int id, int hd, int od, bool ln_first,
                          bool res_project, bool bias, const float* dropout_mlp);
int cube_block_fwd_fused(hipStream_t s, const CubeFusedArgs& a);

#ifdef MIMRL_PHASE_PROBE
int cube_fwd_read_phases(long long* out);   // 128 ticks, see cube_fused.hip
#endif

}  // namespace mimrl
