// Engine, part of the split of round 5 (see engine.h): the C ABI of include/mimrl.h.
#include "engine.h"

extern "C" {

const char* mimrl_last_error(void) { return mimrl::last_error_slot().c_str(); }
#ifdef MIMRL_PHASE_PROBE
// `make PHASE_PROBE=1` only (not part of the ABI): in-kernel phase ticks of the fused CubeMLP forward (tools/cube_phase.py)
int mimrl_dbg_cube_phases(long long* out) { return mimrl::cube_fwd_read_phases(out); }
int mimrl_dbg_cube_bwd_phases(long long* out) { return mimrl::cube_bwd_read_phases(out); }
int mimrl_dbg_kmix_phases(long long* out) { return mimrl::kmix_bwd_read_phases(out); }
int mimrl_dbg_nce_phases(long long* out) { return mimrl::nce_read_phases(out); }
int mimrl_dbg_model_ops_phases(long long* out) { return mimrl::model_ops_read_phases(out); }
int mimrl_dbg_gru_bwd_phases(long long* out) { return mimrl::gru_bwd_read_phases(out); }
int mimrl_dbg_concat_bwd_phases(long long* out) { return mimrl::concat_bwd_read_phases(out); }
#endif
int mimrl_abi_version(void) { return MIMRL_ABI_VERSION; }

int mimrl_device_check(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return set_error(MIMRL_ERR_NODEVICE, "no HIP device visible");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return set_error(MIMRL_ERR_NODEVICE, "hipGetDevice failed");
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, dev) != hipSuccess) return set_error(MIMRL_ERR_NODEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
    return set_error(MIMRL_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 (MI355X) only", dev, p.gcnArchName);
  return MIMRL_OK;
}

}  // extern "C"

// The one place where the engine reads its knobs (engine.h: struct Switches says what each field selects); mimrl_handle's constructor
// calls it.  Apart from it only MIMRL_KNOBS (mimrl_create) and MIMRL_DDP_SPLIT (mimrl_set_comm) are read in engine_*.hip.
Switches mimrl::eng::read_switches(const mimrl_cfg& cfg) {
  Switches sw;
  sw.multi_stream = knob("MIMRL_SINGLE_STREAM") == nullptr;
  sw.fused_cube = knob("MIMRL_NO_FUSED_CUBE") == nullptr;
  sw.fused_cube_bwd = knob("MIMRL_NO_FUSED_CUBE_BWD") == nullptr;
  {
    const char* v = knob("MIMRL_NO_FUSED_TAIL_PRE");
    const bool keep_launches = v && v[0] == '2' && v[1] == 0;
    sw.fused_pre = v == nullptr || keep_launches;
    sw.cube_bookends = v == nullptr;
  }
  sw.fused_mlp = knob("MIMRL_NO_FUSED_MLP") == nullptr;
  sw.fused_mlp_bwd = knob("MIMRL_NO_FUSED_MLP_BWD") == nullptr;
  sw.fused_mi = knob("MIMRL_NO_FUSED_MI") == nullptr;
  sw.mi_nce_tiled = knob("MIMRL_NO_MI_NCE_TILED") == nullptr;
  sw.fused_concat = knob("MIMRL_NO_FUSED_CONCAT") == nullptr;
  sw.concat_dq = knob("MIMRL_NO_CONCAT_DQ") == nullptr;
  sw.concat_dw = knob("MIMRL_NO_CONCAT_DW") == nullptr;
  sw.fold_unpack = knob("MIMRL_NO_FOLD_UNPACK") == nullptr;
  sw.h16 = knob("MIMRL_NO_H16") == nullptr;
  sw.xin = knob("MIMRL_NO_XIN") == nullptr;
  sw.rec16 = knob_int("MIMRL_REC16", 1) != 0;
  sw.dwih_h16 = knob_int("MIMRL_DWIH_H16", 1) != 0;
  sw.laxis_long = knob_int("MIMRL_LAXIS_LONG", 1) != 0;
  sw.laxis_bwd_long = knob_int("MIMRL_LAXIS_BWD_LONG", 1) != 0;
  sw.adam_frag = knob_int("MIMRL_ADAM_FRAG", 1) != 0;
  sw.gru_wgrad = knob("MIMRL_NO_GRU_WGRAD") == nullptr;
  sw.shared_prefix = knob("MIMRL_NO_SHARED_PREFIX") == nullptr;
  sw.dual_tail_pre = knob("MIMRL_NO_DUAL_TAIL_PRE") == nullptr;
  sw.step_graph = knob("MIMRL_NO_STEP_GRAPH") == nullptr;
  sw.fwd_f16 = knob("MIMRL_FWD_BF16") == nullptr;
  sw.l0_packed = knob_int("MIMRL_L0_PACK", 1) != 0;
  const bool gru = cfg.encoder == MIMRL_ENCODER_GRU;
  sw.dg_bf16 = gru && (cfg.precision & MIMRL_PREC_BF16_GRU_BWD) && (cfg.precision & MIMRL_PREC_BF16_GEMM_BWD) && knob("MIMRL_DG_FP32") == nullptr;
  sw.gx_f16 = gru && (cfg.precision & MIMRL_PREC_BF16_GRU_FWD) && (cfg.precision & MIMRL_PREC_BF16_GEMM_FWD) && knob_int("MIMRL_GX_F16", 0) != 0;
  {
    const char* spec = knob("MIMRL_DBG_DELAY_TAG");
    const char* colon = spec ? strchr(spec, ':') : nullptr;
    sw.dbg_delay_tag = spec ? atoi(spec) : -1;
    sw.dbg_delay_us = colon ? atoi(colon + 1) : 50;
  }
  if (const char* dot = knob("MIMRL_GRAPH_DOT")) sw.graph_dot = dot;
  return sw;
}

extern "C" {

int mimrl_create(const mimrl_cfg* cfg, void* hip_stream, mimrl_handle** out) {
  if (!cfg || !out) return set_error(MIMRL_ERR_ARG, "null argument");
  *out = nullptr;
  MX(validate_cfg(*cfg));
  if (cfg->batch > MIMRL_MAX_BATCH)
    return set_error(MIMRL_ERR_ARG, "batch per rank %d exceeds MIMRL_MAX_BATCH (%d)", cfg->batch, MIMRL_MAX_BATCH);
  if (cfg->critic_type == MIMRL_CRITIC_CONCAT && cfg->batch > MIMRL_MAX_BATCH_CONCAT)
    return set_error(MIMRL_ERR_ARG, "batch per rank %d exceeds MIMRL_MAX_BATCH_CONCAT (%d): the concat critic's pair activations "
                     "grow as B^2 (6 x 5 x B^2 x 256 floats)", cfg->batch, MIMRL_MAX_BATCH_CONCAT);
#ifndef MIMRL_DEBUG_KNOBS
  // result-changing debug knobs do not exist in this build; a run that sets one expects something this library will not do
  for (int i = 0; kDebugKnobs[i]; ++i)
    if (getenv(kDebugKnobs[i]))
      return set_error(MIMRL_ERR_ARG, "%s is set, but result-changing debug knobs are compiled out of this build "
                       "(rebuild with `make DEBUG_KNOBS=1` for timing experiments; never for real runs)", kDebugKnobs[i]);
#endif
  MX(mimrl_device_check());
  if (knob_on("MIMRL_KNOBS")) knobs_print(stderr);
  mimrl_handle* h = new (std::nothrow) mimrl_handle(*cfg);   // (its constructor reads the environment: read_switches)
  if (!h) return set_error(MIMRL_ERR_STATE, "out of host memory");
  if (h->ncls() >= 2) h->task_loss = MIMRL_CLASS_LOSS_CE;   // (a regression loss has no meaning on [B, num_class] logits)
  if (h->cfg.beta1 == 0.f) h->cfg.beta1 = 0.9f;
  if (h->cfg.beta2 == 0.f) h->cfg.beta2 = 0.999f;
  if (h->cfg.adam_eps == 0.f) h->cfg.adam_eps = 1e-8f;
  h->stream = h->user_stream = reinterpret_cast<hipStream_t>(hip_stream);
  h->multi_stream = h->sw.multi_stream;
#ifdef MIMRL_DET
  h->multi_stream = false;   // deterministic build: one stream, so the flush behind a launch never meets a half-finished producer (det.h)
  MX(det_init());
#endif
  if (cfg->encoder == MIMRL_ENCODER_GRU && ((cfg->precision & MIMRL_PREC_BF16_GRU_FWD) != 0) != ((cfg->precision & MIMRL_PREC_BF16_GRU_BWD) != 0)) {
    mimrl_destroy(h);   // the forward kernel writes the gate slab in the format (bf16 / fp32 records) the BPTT kernel of the SAME mode reads
    return set_error(MIMRL_ERR_ARG, "MIMRL_PREC_BF16_GRU_FWD and MIMRL_PREC_BF16_GRU_BWD must be set together");
  }
  for (int i = 0; i < mimrl_handle::NSIDE; ++i)
    if (hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking) != hipSuccess) { mimrl_destroy(h); return set_error(MIMRL_ERR_HIP, "hipStreamCreate failed"); }
  gru_probe_setup();
  h->prec = cfg->precision;
  h->bf16 = h->bf16_fwd();
  std::memset(&h->bufs, 0, sizeof h->bufs);
  int r = build_layout(h->cfg, &h->layout);
  if (r == 0) r = h->resolve();
  if (r == 0) r = h->alloc_workspace();
  if (r != 0) { mimrl_destroy(h); return r; }
  *out = h;
  return MIMRL_OK;
}

int mimrl_bind(mimrl_handle* h, const mimrl_buffers* b) {
  if (!h || !b) return set_error(MIMRL_ERR_ARG, "null argument");
  const void* need[] = {b->main_p, b->main_g, b->main_m, b->main_v, b->crit_p, b->crit_g, b->crit_m, b->crit_v,
                        b->text, b->audio, b->video, b->labels, b->lr_main, b->lr_critic, b->pred, b->feats, b->scalars};
  for (const void* p : need)
    if (!p) return set_error(MIMRL_ERR_ARG, "mimrl_bind: a required buffer is null");
  h->bufs = *b;
  h->bound = true;
  {   // deterministic build (det.h: DetDefer): the tensors whose accumulated sums nobody reads before the end of a gradient pass -- the two
      // gradient buckets (NOT the packed layer-0 scratch: l0_unpack_grads reads it inside the pass)
    h->det_ranges.lo[0] = b->main_g; h->det_ranges.lo[1] = b->crit_g;
    h->det_ranges.bytes[0] = sizeof(float) * (size_t)h->layout.floats[MIMRL_GROUP_MAIN];
    h->det_ranges.bytes[1] = sizeof(float) * (size_t)h->layout.floats[MIMRL_GROUP_CRITIC];
    h->det_ranges.n = 2;       // (per handle, handed to every DetDefer scope this handle opens: no process-global table)
  }
  h->part0_done = false;
  h->cur_set = 0;
  for (int q = 0; q < 2; ++q) for (int i = 0; i < 4; ++i) h->gsets[q].in[i] = nullptr;
  h->gsets[0].in[0] = b->text; h->gsets[0].in[1] = b->audio; h->gsets[0].in[2] = b->video; h->gsets[0].in[3] = b->labels;
  h->img_valid = false;
  h->imgT_valid = false;
  h->d_ints = b->counters ? b->counters : h->d_ints_own;   // graphs are rebuilt below, so the new address is baked in
  h->drop_graphs();
  return MIMRL_OK;
}

int mimrl_set_inputs(mimrl_handle* h, int set, const float* text, const float* audio, const float* video, const float* labels) {
  if (!h || set < 0 || set > 1 || !text || !audio || !video || !labels) return set_error(MIMRL_ERR_ARG, "mimrl_set_inputs: bad argument");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  const void* p[4] = {text, audio, video, labels};
  mimrl_handle::GraphSet& g = h->gsets[set];
  if (g.in[0] && (g.in[0] != p[0] || g.in[1] != p[1] || g.in[2] != p[2] || g.in[3] != p[3])) {
    HIPX(hipStreamSynchronize(h->user_stream));
    h->drop_graphs(set);                      // this set's graphs were captured with other addresses
  }
  for (int i = 0; i < 4; ++i) g.in[i] = p[i];
  h->cur_set = set;
  h->part0_done = false;                      // another batch: a pending part-0 hand-over is void
  h->bufs.text = text; h->bufs.audio = audio; h->bufs.video = video; h->bufs.labels = labels;
  return MIMRL_OK;
}

int mimrl_stage1_pipe_prime(mimrl_handle* h) { return h ? h->run_stage1_pipe_prime() : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_stage1_pipe(mimrl_handle* h, int next_valid) { return h ? h->run_stage1_pipe(next_valid != 0) : set_error(MIMRL_ERR_ARG, "null handle"); }

int mimrl_set_bank_rows(mimrl_handle* h, int rows) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (rows < 0 || rows > h->cfg.bank_capacity) return set_error(MIMRL_ERR_ARG, "bank rows %d outside [0,%d]", rows, h->cfg.bank_capacity);
  if (rows > 0) {
    if (!h->bufs.bank_c || !h->bufs.bank_f || !h->bufs.bank_t || !h->bufs.bank_a || !h->bufs.bank_v || !h->bufs.anchors)
      return set_error(MIMRL_ERR_STATE, "banks/anchors must be bound before enabling them");
    if (rows - h->m_anchor() < h->cfg.k_neighbor)
      return set_error(MIMRL_ERR_ARG, "bank of %d rows is too small for %d anchors and k=%d", rows, h->m_anchor(), h->cfg.k_neighbor);
  }
  h->bank_rows = rows;
  return MIMRL_OK;
}

int mimrl_stage1_step(mimrl_handle* h) { return h ? h->run(1, 0) : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_stage2_step(mimrl_handle* h) { return h ? h->run(2, 0) : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_two_stage_step(mimrl_handle* h) { return h ? h->run_step() : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_stage_grads(mimrl_handle* h, int stage) { return h ? h->run(stage, 1) : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_stage_apply(mimrl_handle* h, int stage) { return h ? h->run(stage, 2) : set_error(MIMRL_ERR_ARG, "null handle"); }
int mimrl_stage_grads_part(mimrl_handle* h, int stage, int part) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (stage != 2 || (part != 0 && part != 1)) return set_error(MIMRL_ERR_ARG, "mimrl_stage_grads_part: stage 2, part 0 or 1");
  if (h->cfg.encoder != MIMRL_ENCODER_GRU) return set_error(MIMRL_ERR_ARG, "mimrl_stage_grads_part: GRU encoders only");
  return h->run(2, part == 0 ? 3 : 4);
}

int mimrl_forward(mimrl_handle* h, int train_mode, int with_losses) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  MX(h->ensure_images());
  h->pipe_primed = false;
  launch_begin_stage(h->stream, h->d_ints, (int*)nullptr, h->bufs.scalars, 32, 32);
  LAUNCH_CHECK();
  h->ev_next = 0;
  MX(h->model_forward(train_mode != 0, false));
  if (!with_losses) return MIMRL_OK;
  launch_task_loss(h->stream, h->task_loss, h->bufs.pred, h->bufs.labels, (float*)nullptr,
                     h->bufs.scalars + MIMRL_S2_TASK, h->cfg.batch, h->ncls());
  LAUNCH_CHECK();
  h->ev_next = 0;
  if (h->bank_rows > 0) { MX(h->fork(4, 4)); MX(h->knn_launch(2, h->S(4))); MX(h->estimators_all(2, false, false)); }
  launch_finalize_stage2(h->stream, h->bufs.scalars, h->mi_raw, h->cmi_raw,
                     h->coef2(), h->bank_rows > 0 ? 1 : 0);
  LAUNCH_CHECK();
  return MIMRL_OK;
}

int mimrl_estimate(mimrl_handle* h, int stage) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  if (stage != 1 && stage != 2) return set_error(MIMRL_ERR_ARG, "stage must be 1 or 2");
  if (h->bank_rows <= 0) return set_error(MIMRL_ERR_STATE, "mimrl_estimate needs non-empty banks");
  MX(h->ensure_images());
  h->ev_next = 0;
  MX(h->fork(4, 4));
  MX(h->knn_launch(stage, h->S(4)));
  MX(h->estimators_all(stage, false, false));
  if (stage == 1) {
    launch_finalize_stage1(h->stream, h->bufs.scalars, h->mi_raw, h->cmi_raw,
                       h->bce_raw, h->coef1());
  } else {
    launch_task_loss(h->stream, h->task_loss, h->bufs.pred, h->bufs.labels, (float*)nullptr,
                       h->bufs.scalars + MIMRL_S2_TASK, h->cfg.batch, h->ncls());
    launch_finalize_stage2(h->stream, h->bufs.scalars, h->mi_raw, h->cmi_raw,
                       h->coef2(), 1);
  }
  LAUNCH_CHECK();
  return MIMRL_OK;
}

// ---- test probes: one sub-block of the step, run by the engine's OWN code path (same kernels, buffers and precision mode as a step of
//      this handle) on caller-supplied operands.  The fused bf16 kernels (cube_fwd_fused, daxis / kmix / laxis_bwd, concat_fwd / concat_bwd,
//      mlp_img8 + mi_sep_nce) have no stand-alone entry: these are how tests/test_gpu_fused_oracle.py compares them with the oracle.
int mimrl_probe_cube(mimrl_handle* h, const float* x, float* out, const float* dout, float* dx) {
  if (!h || !x || !out) return set_error(MIMRL_ERR_ARG, "null argument");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  if (dout && !dx) return set_error(MIMRL_ERR_ARG, "dout without dx");
  const mimrl_cfg& c = h->cfg;
  const int nb = c.n_blocks;
  const size_t nin = h->shape(0).in_count(c.batch), nout = h->shape(nb - 1).out_count(c.batch);
  h->ev_next = 0;
  HIPX(hipMemcpyAsync(h->cube0, x, sizeof(float) * nin, hipMemcpyDeviceToDevice, h->stream));
  h->bf16 = h->bf16_fwd();
  MX(h->cube_forward(false, dout != nullptr));
  HIPX(hipMemcpyAsync(out, h->bb[nb - 1].d.z, sizeof(float) * nout, hipMemcpyDeviceToDevice, h->stream));
  if (!dout) return MIMRL_OK;
  if (nout > h->gbuf_floats) return set_error(MIMRL_ERR_STATE, "probe: gradient buffer too small");
  HIPX(hipMemsetAsync(h->bufs.main_g, 0, sizeof(float) * h->layout.floats[MIMRL_GROUP_MAIN], h->stream));
  HIPX(hipMemcpyAsync(h->gbuf[0], dout, sizeof(float) * nout, hipMemcpyDeviceToDevice, h->stream));
  int ci = 0, r;
  {
    Hold bwd(h->bf16, h->bf16_bwd());
    Hold in_place(h->wtT_prebuilt, false);   // (the combined step builds the D-axis weight images beside the encoders; here: in place)
    h->deferred.clear();
    r = h->cube_backward(0, &ci);
    if (r == 0) r = h->flush_deferred();
  }
  h->kmix_pg_on_side3 = false;
  MX(r);
  MX(h->join(0, 5));
  HIPX(hipMemcpyAsync(dx, h->gbuf[ci], sizeof(float) * nin, hipMemcpyDeviceToDevice, h->stream));
  h->grads_clean[2] = false;
  return MIMRL_OK;
}

int mimrl_probe_encoders(mimrl_handle* h, float* cube_x, const float* dcube, const float* dmean) {
  if (!h || !cube_x) return set_error(MIMRL_ERR_ARG, "null argument");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  const mimrl_cfg& c = h->cfg;
  const size_t nin = (size_t)c.batch * c.time_len * 3 * c.d_common, nf = (size_t)c.batch * c.d_common;
  MX(h->ensure_images());
  h->ev_next = 0;
  h->bf16 = h->bf16_fwd();
  {
    Hold keep(h->keep_cube0, true);        // (a pass nobody differentiates does not write the fp32 cube otherwise: engine_forward.hip)
    MX(h->model_forward(true, dcube != nullptr, 0, 0));
  }
  HIPX(hipMemcpyAsync(cube_x, h->cube0, sizeof(float) * nin, hipMemcpyDeviceToDevice, h->stream));
  if (!dcube) return MIMRL_OK;
  if (nin > h->gbuf_floats) return set_error(MIMRL_ERR_STATE, "probe: gradient buffer too small");
  HIPX(hipMemsetAsync(h->bufs.main_g, 0, sizeof(float) * h->layout.floats[MIMRL_GROUP_MAIN], h->stream));
  HIPX(hipMemcpyAsync(h->gbuf[0], dcube, sizeof(float) * nin, hipMemcpyDeviceToDevice, h->stream));
  if (dmean) HIPX(hipMemcpyAsync(h->dfeat + nf, dmean, sizeof(float) * 3 * nf, hipMemcpyDeviceToDevice, h->stream));
  else HIPX(hipMemsetAsync(h->dfeat, 0, sizeof(float) * 4 * nf, h->stream));
  h->deferred.clear();
  h->head_gather_on = false; h->ev_dmean = nullptr; h->kmix_pg_on_side3 = false;
  h->grads_clean[2] = false;
  Hold bwd(h->bf16, h->bf16_bwd());
  return h->encoders_backward(h->gbuf[0]);
}

int mimrl_probe_mi(mimrl_handle* h, int stage, float* mi, float* scores, float* dtin_out) {
  if (!h || !mi) return set_error(MIMRL_ERR_ARG, "null argument");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  if (stage != 1 && stage != 2) return set_error(MIMRL_ERR_ARG, "stage must be 1 or 2");
  const int B = h->cfg.batch;
  const bool bf_bwd = h->bf16_bwd();
  h->ev_next = 0;
  MX(h->ensure_images());
  h->imgT_ready = false;
  if (bf_bwd && h->sw.fused_mlp && h->crit_imgT && h->ttab.n > 0) {   // as estimators_all does, but in line
    MX(bf16_transposed_images(h->stream, h->bufs.crit_p, h->crit_imgT, h->ttab));
    h->imgT_ready = true;
  }
  if (stage == 1) HIPX(hipMemsetAsync(h->bufs.crit_g, 0, sizeof(float) * h->layout.floats[MIMRL_GROUP_CRITIC], h->stream));
  h->bf16 = h->bf16_fwd();
  MX(h->mi_forward(stage, true));
  {
    Hold bwd(h->bf16, bf_bwd);
    h->wg_helper = -1;
    MX(h->mi_backward(stage));
  }
  MX(h->join(0, 5));
  HIPX(hipMemcpyAsync(mi, h->mi_raw, sizeof(float) * 2 * NE_MI, hipMemcpyDeviceToDevice, h->stream));
  if (scores) {
    if (h->cfg.critic_type != MIMRL_CRITIC_CONCAT) return set_error(MIMRL_ERR_ARG, "probe: the separable fused path does not materialise scores");
    HIPX(hipMemcpyAsync(scores, h->scores, sizeof(float) * NE_MI * B * B, hipMemcpyDeviceToDevice, h->stream));
  }
  if (dtin_out) {
    if (stage != 2) return set_error(MIMRL_ERR_ARG, "probe: tower-input gradients exist in stage 2 only");
    HIPX(hipMemcpyAsync(dtin_out, h->dtin, sizeof(float) * 2 * NE_MI * B * EMB, hipMemcpyDeviceToDevice, h->stream));
  }
  if (stage == 1) h->grads_clean[1] = false;
  return MIMRL_OK;
}

int mimrl_probe_cmi(mimrl_handle* h, int stage, const float* cmi_in_, float* logits_out, float* vals, float* dcin_out) {
  if (!h || !cmi_in_ || !logits_out || !vals) return set_error(MIMRL_ERR_ARG, "null argument");
  if (!h->bound) return set_error(MIMRL_ERR_STATE, "mimrl_bind must be called first");
  if (stage != 1 && stage != 2) return set_error(MIMRL_ERR_ARG, "stage must be 1 or 2");
  const int n = h->nprod();
  const bool bf_bwd = h->bf16_bwd();
  h->ev_next = 0;
  MX(h->ensure_images());
  h->imgT_ready = false;
  if (bf_bwd && h->sw.fused_mlp && h->crit_imgT && h->ttab.n > 0) {
    MX(bf16_transposed_images(h->stream, h->bufs.crit_p, h->crit_imgT, h->ttab));
    h->imgT_ready = true;
  }
  if (stage == 1) HIPX(hipMemsetAsync(h->bufs.crit_g, 0, sizeof(float) * h->layout.floats[MIMRL_GROUP_CRITIC], h->stream));
  HIPX(hipMemcpyAsync(h->cmi_in, cmi_in_, sizeof(float) * NE_CMI * 2 * n * 384, hipMemcpyDeviceToDevice, h->stream));
  // cmi_forward minus the kNN / assemble part (Model.py:185-219 on a caller-assembled batch) ...
  h->bf16 = h->bf16_fwd();
  const int cdims[5] = {3 * EMB, HID, HID, HID, 2};
  MX(h->mlp_stack_forward(NE_CMI, 2 * n, 2 * n, h->cmi0, h->cmi_stride, 4, h->cmi_l, cdims, h->cmi_in, h->cc, h->logits));
  MX(cmi_loss_fwd_bwd(h->stream, h->logits, h->dlogits, h->bce_raw, h->cmi_raw, h->g_bce(stage), h->g_cmi(stage), NE_CMI, n, h->cfg.cmi_hardtanh));
  {   // ... and cmi_backward as a step runs it
    Hold bwd(h->bf16, bf_bwd);
    h->wg_helper = -1;
    MX(h->cmi_backward(stage));
  }
  MX(h->join(0, 5));
  HIPX(hipMemcpyAsync(logits_out, h->logits, sizeof(float) * NE_CMI * 2 * n * 2, hipMemcpyDeviceToDevice, h->stream));
  HIPX(hipMemcpyAsync(vals, h->bce_raw, sizeof(float) * NE_CMI, hipMemcpyDeviceToDevice, h->stream));
  HIPX(hipMemcpyAsync(vals + NE_CMI, h->cmi_raw, sizeof(float) * NE_CMI, hipMemcpyDeviceToDevice, h->stream));
  if (dcin_out) {
    if (stage != 2) return set_error(MIMRL_ERR_ARG, "probe: classifier-input gradients exist in stage 2 only");
    HIPX(hipMemcpyAsync(dcin_out, h->dcin, sizeof(float) * NE_CMI * 2 * n * 384, hipMemcpyDeviceToDevice, h->stream));
  }
  if (stage == 1) h->grads_clean[1] = false;
  return MIMRL_OK;
}

int mimrl_set_kernel_stamps(mimrl_handle* h, unsigned long long* ring, int slots) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (ring && (slots < 1 || (slots & (slots - 1)))) return set_error(MIMRL_ERR_ARG, "stamp ring: slots must be a power of two");
  h->kstamp.ring = ring; h->kstamp.step = h->d_ints; h->kstamp.slots = ring ? slots : 0;
  h->drop_graphs();     // captured launches bake the kernel arguments in
  return MIMRL_OK;
}

int mimrl_profile_enable(mimrl_handle* h, int on) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  h->prof_on = on != 0;
  return MIMRL_OK;
}

int mimrl_profile_read(mimrl_handle* h, float* ms_sum, int32_t* launches) {
  if (!h || !ms_sum || !launches) return set_error(MIMRL_ERR_ARG, "null argument");
  HIPX(hipStreamSynchronize(h->stream));
  for (int p = 0; p < MIMRL_NPHASES; ++p) {
    double acc = 0.0;
    for (auto& ev : h->prof_ev[p]) {
      float ms = 0.f;
      HIPX(hipEventElapsedTime(&ms, ev.first, ev.second));
      acc += ms;
      h->prof_pool.push_back(ev);
    }
    ms_sum[p] = (float)acc;
    launches[p] = (int32_t)h->prof_ev[p].size();
    h->prof_ev[p].clear();
  }
  return MIMRL_OK;
}

int mimrl_profile_read_gemm(mimrl_handle* h, double out[4]) {
  if (!h || !out) return set_error(MIMRL_ERR_ARG, "null argument");
  HIPX(hipStreamSynchronize(h->stream));
  HIPX(hipDeviceSynchronize());
  out[0] = out[1] = out[2] = 0.0; out[3] = (double)h->prof_gemm.size();
  for (auto& g : h->prof_gemm) {
    float ms = 0.f;
    HIPX(hipEventElapsedTime(&ms, g.a, g.b));
    out[0] += g.flops; out[1] += g.bytes; out[2] += ms;
    h->prof_pool.push_back({g.a, g.b});
  }
  h->prof_gemm.clear();
  return MIMRL_OK;
}

int mimrl_params_changed(mimrl_handle* h) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  h->img_valid = false;
  h->imgT_valid = false;
  return MIMRL_OK;
}

int mimrl_set_knn_override_mask(mimrl_handle* h, int stage, unsigned call_mask) {
  if (!h || (stage != 1 && stage != 2)) return set_error(MIMRL_ERR_ARG, "bad handle / stage");
  if (call_mask && !h->bufs.knn_override) return set_error(MIMRL_ERR_STATE, "mimrl_buffers.knn_override is not bound");
  if (h->knn_ovr_mask[stage - 1] == (call_mask & 63u)) return MIMRL_OK;
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  h->knn_ovr_mask[stage - 1] = call_mask & 63u;
  return MIMRL_OK;
}

int mimrl_stage2_forward_tail(mimrl_handle* h) { return h ? h->run_fwd2_tail() : set_error(MIMRL_ERR_ARG, "null handle"); }

int mimrl_set_grad_scale(mimrl_handle* h, float scale) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (scale == h->grad_scale) return MIMRL_OK;
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  h->grad_scale = scale;
  return MIMRL_OK;
}

int mimrl_comm_unique_id(void* out128) { return mimrl::comm_unique_id(out128); }

int mimrl_set_comm(mimrl_handle* h, const void* unique_id128, int world, int rank) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  if (h->comm) { MX(mimrl::comm_destroy(h->comm)); h->comm = nullptr; }
  h->comm_world = 1; h->comm_rank = 0;
  if (!unique_id128) return MIMRL_OK;                       // NULL: back to a replica without collectives
  MX(mimrl::comm_init(&h->comm, unique_id128, world, rank));
  h->comm_world = world; h->comm_rank = rank;
  if (!h->comm_s) HIPX(hipStreamCreateWithFlags(&h->comm_s, hipStreamNonBlocking));
  const char* sp = knob("MIMRL_DDP_SPLIT");
  h->comm_split = !(sp && sp[0] == '0');
  // one eager collective now: RCCL's lazy set-up (buffers, proxy threads) must not happen inside a stream capture
  if (h->bound) {
    HIPX(hipMemsetAsync(h->bufs.scalars, 0, sizeof(float), h->user_stream));
    MX(mimrl::comm_allreduce_sum(h->comm, h->bufs.scalars, 1, h->user_stream));
    MX(mimrl::comm_allreduce_sum(h->comm, h->bufs.scalars, 1, h->comm_s));
    HIPX(hipStreamSynchronize(h->user_stream)); HIPX(hipStreamSynchronize(h->comm_s));
  }
  return MIMRL_OK;
}

int mimrl_set_comm_critic_bf16(mimrl_handle* h, int on) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if ((on != 0) == h->comm_crit_bf16) return MIMRL_OK;
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  if (on && !h->comm_crit16) HIPX(hipMalloc(&h->comm_crit16, sizeof(uint16_t) * (size_t)h->layout.floats[MIMRL_GROUP_CRITIC]));
  h->comm_crit_bf16 = on != 0;
  if (on && h->comm && h->bound) {   // RCCL's set-up for the new datatype outside any capture
    HIPX(hipMemsetAsync(h->comm_crit16, 0, 16, h->user_stream));
    MX(mimrl::comm_allreduce_sum_bf16(h->comm, h->comm_crit16, 8, h->user_stream));
    HIPX(hipStreamSynchronize(h->user_stream));
  }
  return MIMRL_OK;
}

int mimrl_set_task_loss(mimrl_handle* h, int kind) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (kind < MIMRL_TASK_LOSS_MAE || kind > MIMRL_TASK_LOSS_CCC) return set_error(MIMRL_ERR_ARG, "task loss kind %d unknown", kind);
  if (h->ncls() >= 2) return set_error(MIMRL_ERR_ARG, "a regression task loss needs the one-output head (num_class %d)", h->cfg.num_class);
  if (kind == h->task_loss) return MIMRL_OK;
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  h->task_loss = kind;
  return MIMRL_OK;
}

int mimrl_set_class_loss(mimrl_handle* h, int kind) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
  if (kind < MIMRL_CLASS_LOSS_CE || kind > MIMRL_CLASS_LOSS_BCE) return set_error(MIMRL_ERR_ARG, "classification loss kind %d unknown", kind);
  if (kind != MIMRL_CLASS_LOSS_BCE && h->ncls() < 2) return set_error(MIMRL_ERR_ARG, "CE / Focal need num_class >= 2 (got %d)", h->cfg.num_class);
  if (kind == MIMRL_CLASS_LOSS_BCE && h->ncls() > 2) return set_error(MIMRL_ERR_ARG, "BCE needs num_class 1 or 2 (got %d; Solver.py:327-337)", h->cfg.num_class);
  if (kind == h->task_loss) return MIMRL_OK;
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  h->task_loss = kind;
  return MIMRL_OK;
}

int64_t mimrl_main_late_offset(const mimrl_handle* h) { return h ? (int64_t)h->layout.late_offset : 0; }

int mimrl_set_stage2_prefetch(mimrl_handle* h, int on) {
  if (!h) return set_error(MIMRL_ERR_ARG, "null handle");
#ifdef MIMRL_DET
  on = 0;                    // deterministic build: no second forward pass on its own stream (same results, sequential schedule)
#endif
  if ((on != 0) == h->prefetch && (on == 2) == h->defer_tail) return MIMRL_OK;
  if (on && !h->pre_stream) HIPX(hipStreamCreateWithFlags(&h->pre_stream, hipStreamNonBlocking));
  HIPX(hipStreamSynchronize(h->user_stream));
  h->drop_graphs();
  h->prefetch = on != 0;
  h->defer_tail = on == 2;
  h->fwd2_pending = false;
  h->tail2_needed = false;
  return MIMRL_OK;
}

int64_t mimrl_workspace_bytes(const mimrl_handle* h) { return h ? (int64_t)h->ws_bytes : 0; }

void mimrl_destroy(mimrl_handle* h) {
  if (!h) return;
  h->drop_graphs();
  for (auto g : h->retired) (void)hipGraphExecDestroy(g);
  h->retired.clear();
  for (int p = 0; p < MIMRL_NPHASES; ++p)
    for (auto& ev : h->prof_ev[p]) h->prof_pool.push_back(ev);
  for (auto& g : h->prof_gemm) h->prof_pool.push_back({g.a, g.b});
  for (auto& ev : h->prof_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  for (int i = 0; i < mimrl_handle::NSIDE; ++i)
    if (h->side[i]) (void)hipStreamDestroy(h->side[i]);
  for (auto e : h->ev_pool) (void)hipEventDestroy(e);
  if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
  if (h->pre_stream) (void)hipStreamDestroy(h->pre_stream);
  if (h->comm) (void)mimrl::comm_destroy(h->comm);
  if (h->comm_s) (void)hipStreamDestroy(h->comm_s);
  if (h->comm_crit16) (void)hipFree(h->comm_crit16);
  if (h->ws) (void)hipFree(h->ws);
  delete h;
}

// ---- operator-level entry points ------------------------------------------------------------
int mimrl_op_gemm(void* stream, const float* A, const float* B, float* C, int M, int N, int K, int batch,
                  const int64_t st[9], const float* bias_n, const float* bias_m, float alpha, float beta, int act,
                  int precision) {
  if (!st) return set_error(MIMRL_ERR_ARG, "null strides");
  GemmDesc d;
  d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K; d.batch = batch;
  d.sa_m = st[0]; d.sa_k = st[1]; d.sa_b = st[2]; d.sb_k = st[3]; d.sb_n = st[4]; d.sb_b = st[5];
  d.sc_m = st[6]; d.sc_n = st[7]; d.sc_b = st[8];
  d.bias_n = bias_n; d.bias_m = bias_m; d.alpha = alpha; d.beta = beta; d.act = act & 0xff;
  d.atomic = (act >> 8) & 1;   // bit 8: accumulate with atomics (enables split-K / batch-group reduction)
  return gemm(reinterpret_cast<hipStream_t>(stream), d, (precision & 1) != 0);
}

int mimrl_op_gemm_ex(void* stream, const float* A, const float* B, float* C, int M, int N, int K, int batch, const int64_t st[9],
                     const float* A2, const float* B2, int K2, const int64_t st2[6], int a_gap_at, int a_gap_rows, const float* bias_n,
                     const float* gradact_u, float* colsum, int act, int precision) {
  if (!st || (A2 && !st2)) return set_error(MIMRL_ERR_ARG, "null strides");
  GemmDesc d;
  d.A = A; d.B = B; d.C = C; d.M = M; d.N = N; d.K = K; d.batch = batch;
  d.sa_m = st[0]; d.sa_k = st[1]; d.sa_b = st[2]; d.sb_k = st[3]; d.sb_n = st[4]; d.sb_b = st[5];
  d.sc_m = st[6]; d.sc_n = st[7]; d.sc_b = st[8];
  if (A2) {
    d.A2 = A2; d.B2 = B2; d.K2 = K2;
    d.sa2_m = st2[0]; d.sa2_k = st2[1]; d.sa2_b = st2[2]; d.sb2_k = st2[3]; d.sb2_n = st2[4]; d.sb2_b = st2[5];
  }
  d.a_gap_at = a_gap_at; d.a_gap_rows = a_gap_rows;
  d.bias_n = bias_n; d.gradact_u = gradact_u; d.colsum = colsum; d.act = act & 0xff; d.atomic = (act >> 8) & 1;
  return gemm(reinterpret_cast<hipStream_t>(stream), d, (precision & 1) != 0);
}

int mimrl_op_gemm16(void* stream, const void* A, const void* B, void* C, int M, int N, int K, int batch, const int64_t st[9],
                    const void* A2, const void* B2, int K2, const int64_t st2[6], int batch_in, const int64_t st_bo[5],
                    const float* bias_n, int flags) {
  if (!st || (A2 && !st2) || (batch_in > 0 && !st_bo)) return set_error(MIMRL_ERR_ARG, "null strides");
  if (batch_in < 0 || (batch_in > 0 && batch % batch_in != 0)) return set_error(MIMRL_ERR_ARG, "batch_in must divide batch");
  GemmDesc d;
  d.A = static_cast<const float*>(A); d.B = static_cast<const float*>(B); d.C = static_cast<float*>(C);
  d.M = M; d.N = N; d.K = K; d.batch = batch;
  d.sa_m = st[0]; d.sa_k = st[1]; d.sa_b = st[2]; d.sb_k = st[3]; d.sb_n = st[4]; d.sb_b = st[5];
  d.sc_m = st[6]; d.sc_n = st[7]; d.sc_b = st[8];
  if (A2) {
    d.A2 = static_cast<const float*>(A2); d.B2 = static_cast<const float*>(B2); d.K2 = K2;
    d.sa2_m = st2[0]; d.sa2_k = st2[1]; d.sa2_b = st2[2]; d.sb2_k = st2[3]; d.sb2_n = st2[4]; d.sb2_b = st2[5];
  }
  if (batch_in > 0) { d.batch_in = batch_in; d.sa_bo = st_bo[0]; d.sb_bo = st_bo[1]; d.sc_bo = st_bo[2]; d.bias_n_bo = st_bo[3]; }
  if (st_bo) d.bias_n_b = st_bo[4];
  d.bias_n = bias_n;
  d.a_bf16 = flags & 1; d.b_bf16 = (flags >> 1) & 1; d.f16 = (flags >> 2) & 1; d.c_f16 = (flags >> 3) & 1; d.atomic = (flags >> 4) & 1;
  if (flags >> 8) { d.a_gap_at = (flags >> 8) & 0xfff; d.a_gap_rows = (flags >> 20) & 0xfff; }
  return gemm(reinterpret_cast<hipStream_t>(stream), d, true);
}

int mimrl_op_gemm_wgrad_group(void* stream, int n, const float* const* A, const float* const* B, float* const* C, const int32_t* dims,
                              const int64_t* st, int precision) {
  if (n <= 0 || n > 12 || !A || !B || !C || !dims || !st) return set_error(MIMRL_ERR_ARG, "gemm_wgrad_group: 1..12 problems");
  GemmDesc d[12];
  for (int i = 0; i < n; ++i) {
    d[i].A = A[i]; d[i].B = B[i]; d[i].C = C[i];
    d[i].M = dims[4 * i]; d[i].N = dims[4 * i + 1]; d[i].K = dims[4 * i + 2]; d[i].batch = dims[4 * i + 3];
    const int64_t* q = st + 9 * i;
    d[i].sa_m = q[0]; d[i].sa_k = q[1]; d[i].sa_b = q[2]; d[i].sb_k = q[3]; d[i].sb_n = q[4]; d[i].sb_b = q[5];
    d[i].sc_m = q[6]; d[i].sc_n = q[7]; d[i].sc_b = q[8];
    d[i].atomic = 1;
  }
  return gemm_group_splitk(reinterpret_cast<hipStream_t>(stream), d, n, (precision & 1) != 0);
}

int64_t mimrl_op_gru_saved_floats(int B, int T) { return gru_saved_floats(B, T); }

int mimrl_op_gru_forward(void* stream, const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r,
                         const float* bhh_f, const float* bhh_r, const int32_t* lens, float* out, float* saved_f,
                         float* saved_r, int B, int T, int precision) {
  GruFwdArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = B; a.T = T; a.out_ld = 2 * H; a.nmod = 1; a.btv = gru_pick_btv(B, 1);
  a.lens[0] = lens; a.lens[1] = lens;
  a.seq[0][0] = GruSeq{gx_f, whh_f, bhh_f, out, saved_f};
  a.seq[0][1] = GruSeq{gx_r, whh_r, bhh_r, out, saved_r};
  return gru_forward(reinterpret_cast<hipStream_t>(stream), a, (precision & 1) != 0);
}

int mimrl_op_gru_backward(void* stream, const float* whh_f, const float* whh_r, const float* saved_f,
                          const float* saved_r, const int32_t* lens, const float* out, const float* dout, float* dg_f,
                          float* dg_r, float* hprev_f, float* hprev_r, int B, int T, int precision) {
  GruBwdArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = B; a.T = T; a.out_ld = 2 * H; a.dout_ld = 2 * H; a.dout_off = H; a.nmod = 1; a.btv = gru_pick_btv(B, 1);
  a.lens[0] = lens; a.lens[1] = lens;
  a.seq[0][0] = GruSeqBwd{whh_f, saved_f, out, dout, dg_f, hprev_f, nullptr, nullptr};
  a.seq[0][1] = GruSeqBwd{whh_r, saved_r, out, dout, dg_r, hprev_r, nullptr, nullptr};
  return gru_backward(reinterpret_cast<hipStream_t>(stream), a, (precision & 1) != 0);
}

int mimrl_op_recur_btv(int B, int nmod) {
  if (B < 1 || nmod < 1 || nmod > 2) return set_error(MIMRL_ERR_ARG, "mimrl_op_recur_btv: B >= 1, nmod 1 or 2");
  const int g = gru_pick_btv(B, nmod), l = lstm_btv(B, nmod);
  if (g != l) return set_error(MIMRL_ERR_STATE, "mimrl_op_recur_btv: the GRU (%d) and LSTM (%d) picks differ: give this entry point an encoder argument", g, l);
  return g;
}

int mimrl_op_lstm_forward(void* stream, const float* gx_f, const float* gx_r, const float* whh_f, const float* whh_r,
                          const float* bhh_f, const float* bhh_r, const int32_t* lens, float* out, float* saved_f,
                          float* saved_r, int B, int T, int kernel) {
  if (!gx_f || !gx_r || !whh_f || !whh_r || !bhh_f || !bhh_r || !lens || !out) return set_error(MIMRL_ERR_ARG, "mimrl_op_lstm_forward: null argument");
  if ((saved_f != nullptr) != (saved_r != nullptr)) return set_error(MIMRL_ERR_ARG, "mimrl_op_lstm_forward: both saved records or neither");
  LstmFwdArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = B; a.T = T; a.out_ld = 2 * H; a.nmod = 1;
  a.lens[0] = lens; a.lens[1] = lens;
  a.seq[0][0] = LstmSeq{gx_f, whh_f, bhh_f, out, saved_f};
  a.seq[0][1] = LstmSeq{gx_r, whh_r, bhh_r, out, saved_r};
  return lstm_forward_kernels(reinterpret_cast<hipStream_t>(stream), a, kernel);
}

int mimrl_op_lstm_backward(void* stream, const float* whh_f, const float* whh_r, const float* saved_f,
                           const float* saved_r, const int32_t* lens, const float* out, const float* dout, float* dg_f,
                           float* dg_r, float* hprev_f, float* hprev_r, int B, int T, int kernel) {
  if (!whh_f || !whh_r || !saved_f || !saved_r || !lens || !out || !dout || !dg_f || !dg_r || !hprev_f || !hprev_r)
    return set_error(MIMRL_ERR_ARG, "mimrl_op_lstm_backward: null argument");
  LstmBwdArgs a;
  std::memset(&a, 0, sizeof a);
  a.B = B; a.T = T; a.out_ld = 2 * H; a.dout_ld = 2 * H; a.nmod = 1;
  a.lens[0] = lens; a.lens[1] = lens;
  a.seq[0][0] = LstmSeqBwd{whh_f, saved_f, out, dout, dg_f, hprev_f};
  a.seq[0][1] = LstmSeqBwd{whh_r, saved_r, out, dout + H, dg_r, hprev_r};     // each direction reads its own half of dout
  return lstm_backward_kernels(reinterpret_cast<hipStream_t>(stream), a, kernel);
}

int mimrl_op_concat_dw(void* stream, const void* dz2, const void* a1, float* dw2, const void* dz1, const void* a0, float* dw1, int E, int64_t rows,
                       int64_t dw_stride, const float* ds, const void* a2h, float* dw3, const uint32_t* m2, const float* w3, const float* P,
                       const float* Q, int B) {
  if ((!dz2 && !m2) || !a1 || !dw2) return set_error(MIMRL_ERR_ARG, "mimrl_op_concat_dw: null argument");
  if ((dz1 != nullptr) != (a0 != nullptr || P != nullptr) || (dz1 != nullptr) != (dw1 != nullptr)) return set_error(MIMRL_ERR_ARG, "mimrl_op_concat_dw: the second layer comes as a set");
  if (!concat_dw_ok(E, rows, 256)) return set_error(MIMRL_ERR_ARG, "mimrl_op_concat_dw: E >= 1, rows >= 1");
  ConcatDwArgs a;
  a.dz[0] = static_cast<const __bf16*>(dz2); a.act[0] = static_cast<const __bf16*>(a1); a.dw[0] = dw2;
  a.dz[1] = static_cast<const __bf16*>(dz1); a.act[1] = static_cast<const __bf16*>(a0); a.dw[1] = dw1;
  a.nlayer = dz1 ? 2 : 1; a.E = E; a.rows = rows; a.dw_stride = dw_stride;
  a.ds = ds; a.a2 = static_cast<const _Float16*>(a2h); a.dw3 = dw3; a.m2 = m2; a.w3 = w3; a.P = P; a.Q = Q; a.B = B;
  return concat_dw(reinterpret_cast<hipStream_t>(stream), a);
}

int mimrl_op_gru_wgrad(void* stream, const void* const* dg, const void* const* x, const void* const* hp, float* const* dw_ih,
                       float* const* dw_hh, int64_t rows, int kp) {
  if (!dg || !x || !hp || !dw_ih || !dw_hh) return set_error(MIMRL_ERR_ARG, "mimrl_op_gru_wgrad: null argument");
  GruWgradArgs a;
  for (int s = 0; s < 4; ++s) {
    if (!dg[s] || !x[s] || !hp[s] || !dw_ih[s] || !dw_hh[s]) return set_error(MIMRL_ERR_ARG, "mimrl_op_gru_wgrad: null array for sequence %d", s);
    a.seq[s] = GruWgradSeq{static_cast<const __bf16*>(dg[s]), static_cast<const __bf16*>(x[s]), static_cast<const __bf16*>(hp[s]), dw_ih[s], dw_hh[s]};
  }
  a.rows = rows; a.kp = kp;
  return gru_wgrad(reinterpret_cast<hipStream_t>(stream), a);
}

int mimrl_op_mi_bound(void* stream, const float* scores, float* dscores, float* mi, const float* gscale, int E, int B,
                      int bound) {
  return mi_bound_fwd_bwd(reinterpret_cast<hipStream_t>(stream), scores, dscores, mi, nullptr, gscale, E, B, bound, 0u);
}
int mimrl_op_mi_bound_baseline(void* stream, float* scores, float* dscores, float* mi, const float* gscale, const float* lb,
                               float* dlb, int E, int B, int bound) {
  return mi_bound_fwd_bwd(reinterpret_cast<hipStream_t>(stream), scores, dscores, mi, nullptr, gscale, E, B, bound, 0u, lb, dlb, B);
}
int mimrl_op_mi_bound_ex(void* stream, const float* scores, float* dscores, float* mi, float* mi_loss, const float* gscale,
                         int E, int B, int bound, uint32_t lossform) {
  return mi_bound_fwd_bwd(reinterpret_cast<hipStream_t>(stream), scores, dscores, mi, mi_loss, gscale, E, B, bound, lossform);
}

int mimrl_op_mi_infonce_rows(void* stream, const float* scores, float* dscores, float* mi, float* mi_loss, const float* gscale,
                             int E, int B, float* ws) {
  static_assert(MIMRL_NCE_WS_FLOATS >= NCE_WS_WIDE_FLOATS && NCE_WS_WIDE_FLOATS >= NCE_WS_FLOATS, "MIMRL_NCE_WS_FLOATS too small");
  if (!scores || !mi || !ws || E < 1 || E > 16) return set_error(MIMRL_ERR_ARG, "mi_infonce_rows: null array or E = %d outside [1, 16]", E);
  return mi_bound_fwd_bwd(reinterpret_cast<hipStream_t>(stream), scores, dscores, mi, mi_loss, gscale, E, B, BOUND_INFONCE, 0u, nullptr,
                          nullptr, 0, ws);
}
int mimrl_op_mi_sep_infonce(void* stream, const float* tout, float* dtout, float* mi, float* mi_loss, const float* gscale, int E,
                            int B, int tiled) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!tiled) return mi_sep_fused(st, tout, dtout, mi, mi_loss, gscale, E, B, BOUND_INFONCE, 0x1fu, dtout ? 1 : 0);
  return mi_sep_nce_tiled(st, tout, dtout, mi, mi_loss, gscale, E, B, dtout ? 1 : 0);   // accumulates: caller zeroes mi / mi_loss / dtout
}

int mimrl_op_knn(void* stream, const float* Z, int dz, int N, const int32_t* anchors, int m, int k, int32_t* idx_out) {
  KnnArgs a;
  std::memset(&a, 0, sizeof a);
  a.call[0] = KnnCall{Z, dz, anchors, idx_out};
  a.N = N; a.m = m; a.k = k; a.ncall = 1;
  return knn_sample(reinterpret_cast<hipStream_t>(stream), a);
}

int mimrl_probe_knn(mimrl_handle* h, int stage, int32_t* idx_out) {
  if (!h || !idx_out) return set_error(MIMRL_ERR_ARG, "mimrl_probe_knn: null argument");
  if (stage != 1 && stage != 2) return set_error(MIMRL_ERR_ARG, "stage must be 1 or 2");
  HIPX(hipMemcpyAsync(idx_out, stage == 2 ? h->knn_idx2 : h->knn_idx, sizeof(int32_t) * NE_CMI * h->nprod(), hipMemcpyDeviceToDevice, h->user_stream));
  return MIMRL_OK;
}

int mimrl_op_sample_anchors(void* stream, int32_t* anchors_out, int ncall, int m, int N, uint64_t seed, const int32_t* step,
                            uint32_t stream_id, int step_add) {
  if (!anchors_out || !step || ncall < 1 || ncall > KNN_MAX_CALLS) return set_error(MIMRL_ERR_ARG, "mimrl_op_sample_anchors: bad argument");
  AnchorDraws d;
  d.n = ncall;
  for (int c = 0; c < ncall; ++c) { d.out[c] = anchors_out + (size_t)c * m; d.call[c] = c; d.stream_id[c] = stream_id; d.step_add[c] = step_add; }
  return sample_anchors(reinterpret_cast<hipStream_t>(stream), d, m, N, (uint32_t)seed, (uint32_t)(seed >> 32), step);
}

int mimrl_op_cmi_loss(void* stream, const float* logits, float* dlogits, float* bce, float* cmi, const float* g_bce,
                      const float* g_cmi, int E, int n, int hardtanh) {
  return cmi_loss_fwd_bwd(reinterpret_cast<hipStream_t>(stream), logits, dlogits, bce, cmi, g_bce, g_cmi, E, n, hardtanh);
}

int mimrl_op_task_loss(void* stream, int kind, const float* pred, const float* y, float* dpred, float* loss, int B) {
  if (!pred || !y || !loss) return set_error(MIMRL_ERR_ARG, "task_loss: null argument");
  if (kind < MIMRL_TASK_LOSS_MAE || kind > MIMRL_TASK_LOSS_CCC) return set_error(MIMRL_ERR_ARG, "task loss kind %d unknown", kind);
  if (B < 1 || B > 1024) return set_error(MIMRL_ERR_ARG, "task_loss: batch %d outside [1, 1024]", B);
  launch_task_loss(reinterpret_cast<hipStream_t>(stream), kind, pred, y, dpred, loss, B);
  LAUNCH_CHECK();
  return MIMRL_OK;
}

int mimrl_op_class_loss(void* stream, int kind, const float* logits, const float* y, float* dlogits, float* loss, int B, int C) {
  if (!logits || !y || !loss) return set_error(MIMRL_ERR_ARG, "class_loss: null argument");
  if (kind < MIMRL_CLASS_LOSS_CE || kind > MIMRL_CLASS_LOSS_BCE) return set_error(MIMRL_ERR_ARG, "classification loss kind %d unknown", kind);
  if (B < 1 || B > 1024) return set_error(MIMRL_ERR_ARG, "class_loss: batch %d outside [1, 1024]", B);
  if (C < 1 || C > MIMRL_MAX_CLASSES) return set_error(MIMRL_ERR_ARG, "class_loss: %d classes outside [1, %d]", C, MIMRL_MAX_CLASSES);
  if (kind != MIMRL_CLASS_LOSS_BCE && C < 2) return set_error(MIMRL_ERR_ARG, "class_loss: CE / Focal need at least 2 classes");
  if (kind == MIMRL_CLASS_LOSS_BCE && C > 2) return set_error(MIMRL_ERR_ARG, "class_loss: BCE takes 1 or 2 classes (got %d)", C);
  launch_task_loss(reinterpret_cast<hipStream_t>(stream), kind, logits, y, dlogits, loss, B, C);
  LAUNCH_CHECK();
  return MIMRL_OK;
}

static int fill_mlp_args(MlpFusedArgs* fa, int nb, int rows, int brows, int nl, const int32_t* dims, const float* const* W,
                         int64_t pstride) {
  if (!dims || !W || nl < 1 || nl > MLPF_MAX_LAYERS) return set_error(MIMRL_ERR_ARG, "mlp_stack: bad arguments");
  std::memset(fa, 0, sizeof *fa);
  fa->nb = nb; fa->rows = rows; fa->brows = brows; fa->nl = nl; fa->pstride = pstride;
  for (int l = 0; l <= nl; ++l) fa->dims[l] = dims[l];
  for (int l = 0; l < nl; ++l) fa->W[l] = W[l];
  return MIMRL_OK;
}

int mimrl_op_mlp_stack_forward(void* stream, int nb, int rows, int brows, int nl, const int32_t* dims, const float* const* W,
                               const float* const* b, int64_t pstride, const float* in, float* const* act, float* out) {
  MlpFusedArgs fa;
  MX(fill_mlp_args(&fa, nb, rows, brows, nl, dims, W, pstride));
  if (!b || !in || !out || (nl > 1 && !act)) return set_error(MIMRL_ERR_ARG, "mlp_stack_forward: null argument");
  for (int l = 0; l < nl; ++l) { fa.b[l] = b[l]; if (l < nl - 1) fa.act[l] = act[l]; }
  fa.in = in; fa.out = out;
  return mlp_stack_fwd_fused(reinterpret_cast<hipStream_t>(stream), fa);
}

int mimrl_op_mlp_stack_backward(void* stream, int nb, int rows, int brows, int nl, const int32_t* dims, const float* const* W,
                                int64_t pstride, const float* const* act, const float* dout, float* const* dz, float* din,
                                float* const* db) {
  MlpFusedArgs fa;
  MX(fill_mlp_args(&fa, nb, rows, brows, nl, dims, W, pstride));
  if (!dout || (nl > 1 && (!act || !dz))) return set_error(MIMRL_ERR_ARG, "mlp_stack_backward: null argument");
  for (int l = 0; l < nl - 1; ++l) { fa.act[l] = const_cast<float*>(act[l]); fa.dz[l + 1] = dz[l + 1]; fa.db[l] = db ? db[l] : nullptr; }
  fa.dout = dout; fa.din = din;
  return mlp_stack_bwd_fused(reinterpret_cast<hipStream_t>(stream), fa);
}

int mimrl_op_adam(void* stream, float* p, float* g, float* m, float* v, int64_t n, const float* lr, const int32_t* step,
                  float beta1, float beta2, float eps, float weight_decay, float clip) {
  AdamArgs a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.lr = lr; a.step = step;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.clip = clip;
  return adam_step(reinterpret_cast<hipStream_t>(stream), a);
}

int mimrl_op_adam_ex(void* stream, float* p, float* g, float* m, float* v, int64_t n, const float* lr, const int32_t* step,
                     float beta1, float beta2, float eps, float weight_decay, float clip, float gscale, void* pimg,
                     int nfold, const int64_t* fold_lo, const int32_t* fold_rows, const int32_t* fold_d, const int32_t* fold_ld,
                     float* const* fold_src,
                     int nfrag, const int64_t* frag_off, const int32_t* frag_OUT, const int32_t* frag_RED, const int32_t* frag_nb,
                     const int64_t* frag_gstride, void* frag_dst) {
  if (!p || !g || !m || !v || !lr || !step || n < 1) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: null array or n < 1");
  AdamArgs a;
  a.p = p; a.g = g; a.m = m; a.v = v; a.n = n; a.lr = lr; a.step = step;
  a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.weight_decay = weight_decay; a.clip = clip;
  a.gscale = gscale; a.pimg = static_cast<__bf16*>(pimg);
  if (nfold < 0 || nfold > 8) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: %d parked pieces outside [0, 8]", nfold);
  if (nfold > 0 && (!fold_lo || !fold_rows || !fold_d || !fold_ld || !fold_src)) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: null fold array");
  for (int q = 0; q < nfold; ++q) {
    if (!fold_src[q] || fold_rows[q] < 1 || fold_d[q] < 1 || fold_ld[q] < fold_d[q] || fold_lo[q] < 0 ||
        fold_lo[q] + (int64_t)fold_rows[q] * fold_d[q] > n)
      return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: parked piece %d is not rows x d <= ld inside the bucket", q);
    a.fold.lo[q] = fold_lo[q]; a.fold.hi[q] = fold_lo[q] + (long)fold_rows[q] * fold_d[q];
    a.fold.src[q] = fold_src[q]; a.fold.d[q] = fold_d[q]; a.fold.ld[q] = fold_ld[q];
  }
  a.fold.n = nfold;
  if (nfold > 0) {
    a.fold.lo_all = a.fold.lo[0]; a.fold.hi_all = a.fold.hi[0];
    for (int q = 1; q < a.fold.n; ++q) { a.fold.lo_all = std::min(a.fold.lo_all, a.fold.lo[q]); a.fold.hi_all = std::max(a.fold.hi_all, a.fold.hi[q]); }
  }
  if (nfrag < 0 || nfrag > 24) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: %d image entries outside [0, 24]", nfrag);
  if (nfrag > 0) {
    if (!frag_off || !frag_OUT || !frag_RED || !frag_nb || !frag_gstride || !frag_dst) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: null image array");
    FragTable t;
    std::memset(&t, 0, sizeof t);
    t.n = nfrag;
    for (int e = 0; e < nfrag; ++e) {
      const int64_t mat = (int64_t)frag_OUT[e] * frag_RED[e];
      if (frag_OUT[e] < 32 || frag_OUT[e] % 32 != 0 || frag_RED[e] < 64 || frag_RED[e] % 64 != 0 || frag_nb[e] < 1 || frag_off[e] < 0 ||
          frag_off[e] % 8 != 0 || frag_gstride[e] % 8 != 0 || frag_gstride[e] < mat || frag_off[e] + (frag_nb[e] - 1) * frag_gstride[e] + mat > n)
        return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: image entry %d is not nb x [32k x 64k] at 16-byte offsets inside the bucket", e);
      t.off[e] = frag_off[e]; t.OUT[e] = frag_OUT[e]; t.RED[e] = frag_RED[e]; t.nb[e] = frag_nb[e]; t.gstride[e] = frag_gstride[e];
    }
    if (!adam_frag_from_table(a, t, static_cast<__bf16*>(frag_dst))) return set_error(MIMRL_ERR_ARG, "mimrl_op_adam_ex: more than 12 image entries");
  }
  return adam_step(reinterpret_cast<hipStream_t>(stream), a);
}

int mimrl_op_frag_images(void* stream, const float* src, void* dst, int n, const int64_t* off, const int32_t* OUT, const int32_t* RED,
                         const int32_t* nb, const int32_t* tr, const int64_t* gstride, const int64_t* dshift) {
  if (!src || !dst || !off || !OUT || !RED || !nb || !tr || !gstride || !dshift) return set_error(MIMRL_ERR_ARG, "mimrl_op_frag_images: null argument");
  if (n < 1 || n > 24) return set_error(MIMRL_ERR_ARG, "mimrl_op_frag_images: %d table entries outside [1, 24]", n);
  FragTable t;
  std::memset(&t, 0, sizeof t);
  t.n = n;
  for (int e = 0; e < n; ++e) {
    if (OUT[e] < 32 || RED[e] < 64 || nb[e] < 1 || off[e] < 0 || off[e] + dshift[e] < 0 || gstride[e] < (int64_t)OUT[e] * RED[e])
      return set_error(MIMRL_ERR_ARG, "mimrl_op_frag_images: entry %d has an empty matrix, a negative offset or overlapping groups", e);
    t.off[e] = off[e]; t.OUT[e] = OUT[e]; t.RED[e] = RED[e]; t.nb[e] = nb[e]; t.tr[e] = tr[e] != 0; t.gstride[e] = gstride[e]; t.dshift[e] = dshift[e];
  }
  return bf16_frag_images(reinterpret_cast<hipStream_t>(stream), src, static_cast<__bf16*>(dst), t);
}

}  // extern "C"
