// session_batch.cpp -- several sequences per step (llmi_session_seq_* / llmi_session_batch_*).
// A batch step is the batched prefill's launch sequence over B token rows (Session::prefill_layers), each row a
// position of its own KV slot, then the scorer's rows; the greedy loop adds one feedback launch per step, the
// sampled loop (section 13) the rows' full logits and the sampler's two multi-row launches.
#include "session.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace llmi {

static bool f16_finite(uint16_t h) { return (h & 0x7C00u) != 0x7C00u; }

void Session::seq_reserve(int n_seq) {
  // the refusals first: a session that cannot take batch steps says why, whatever n_seq is
  if (exact_) throw status_error(LLMI_E_ARG, "seq_reserve: exact sessions run one sequence (exact mode is out of scope)");
  if (tp_) throw status_error(LLMI_E_ARG, "seq_reserve: one device only (tensor-parallel session)");
  if (hp_.gemma4 || ple_table_.qs) throw status_error(LLMI_E_ARG, "seq_reserve: Gemma-3 layers only (Gemma-4 model)");
  for (const auto& l : L_)
    if (!l.has_kv) throw status_error(LLMI_E_ARG, "seq_reserve: Gemma-3 layers only (shared-KV layers)");
  // (their prefill hands the attention's outputs on as Q8_K blocks, a form the multi-sequence attention does not have)
  if (pf_kq_) throw status_error(LLMI_E_ARG, "seq_reserve: Q4_0 / Q8_0 layers only (this model has K-quant layers)");
  const int G = nh_ / std::max(nkv_, 1);
  for (const auto& l : L_)
    if ((l.hd != 128 && l.hd != 256) || (G != 1 && G != 2 && G != 4) || getenv("LLMI_PREFILL_ATTN_V1"))
      throw status_error(LLMI_E_ARG, "seq_reserve: needs the MFMA prefill attention at head_dim 128 or 256, GQA group 1, "
                                     "2 or 4");
  if (!prefill_ok_) throw status_error(LLMI_E_ARG, "seq_reserve: the session has no batched prefill");
  if (getenv("LLMI_NO_PREFILL")) throw status_error(LLMI_E_ARG, "seq_reserve: the batched prefill is off (LLMI_NO_PREFILL)");
  if (embd_.type != T_F16)
    throw status_error(LLMI_E_ARG, "seq_reserve: needs the fused scorer, i.e. an F16 output table (this one is quantized)");
  if (score_path() != 1) throw status_error(LLMI_E_ARG, "seq_reserve: needs the fused scorer (score_path 1)");
  if (n_seq < 1 || n_seq > LLMI_SEQ_MAX)
    throw status_error(LLMI_E_RANGE, "seq_reserve: n_seq must be in 1.." + std::to_string(LLMI_SEQ_MAX));
  ensure_usable();
  const int NL = hp_.n_layer;
  if (!bt_kvtab_) {
    bt_h_kvtab_.assign((size_t)NL * 2 * LLMI_SEQ_MAX, nullptr);
    for (int l = 0; l < NL; l++) {
      bt_h_kvtab_[(size_t)l * 2 * LLMI_SEQ_MAX] = L_[(size_t)l].kc;
      bt_h_kvtab_[(size_t)l * 2 * LLMI_SEQ_MAX + 1] = L_[(size_t)l].vc;
    }
    bt_kvtab_ = dalloc<uint16_t*>(bt_h_kvtab_.size());
    bt_rows_ = dalloc<SeqRow>(LLMI_SEQ_MAX);
    bt_trows_ = dalloc<SeqRow>(LLMI_SEQ_MAX);
    bt_tok_ = dalloc<int32_t>(LLMI_SEQ_MAX);
    bt_row0_ = dalloc<uint16_t>((size_t)LLMI_SEQ_MAX * hp_.n_embd);
    bt_r0_lse_ = dalloc<float>(2 * LLMI_SEQ_MAX);
    bt_r0_amax_ = dalloc<int32_t>(LLMI_SEQ_MAX);
  }
  // the slots below n_seq that have no cache yet: their own allocations (zeroed on the stream), so a larger reserve
  // moves nothing, and a call that failed partway leaves entries the next call keeps
  for (int q = 1; q < n_seq; q++)
    for (int l = 0; l < NL; l++)
      for (int kv = 0; kv < 2; kv++) {
        uint16_t*& e = bt_h_kvtab_[((size_t)l * LLMI_SEQ_MAX + q) * 2 + kv];
        if (!e) e = dalloc<uint16_t>((size_t)nkv_ * max_ctx_ * L_[(size_t)l].hd);
      }
  h2d(bt_kvtab_, bt_h_kvtab_.data(), bt_h_kvtab_.size() * sizeof(uint16_t*));
  n_seq_ = std::max(n_seq_, n_seq);
  seq_reserved_ = true;
}

void Session::seq_copy(int dst, int src, int n_pos) {
  if (!seq_reserved_) throw status_error(LLMI_E_ARG, "seq_copy: no KV slots reserved (call seq_reserve first)");
  if (dst < 0 || dst >= n_seq_) throw status_error(LLMI_E_RANGE, "seq_copy: slot outside [0, n_seq) (dst)");
  if (src < 0 || src >= n_seq_) throw status_error(LLMI_E_RANGE, "seq_copy: slot outside [0, n_seq) (src)");
  if (n_pos < 0 || n_pos > max_ctx_) throw status_error(LLMI_E_RANGE, "seq_copy: rows past max_ctx (n_pos)");
  ensure_usable();
  if (dst == src || n_pos == 0) return;
  for (int l = 0; l < hp_.n_layer; l++) {
    const size_t pitch = (size_t)max_ctx_ * L_[(size_t)l].hd * 2, width = (size_t)n_pos * L_[(size_t)l].hd * 2;
    for (int kv = 0; kv < 2; kv++)  // one strided copy per layer and cache: n_head_kv runs of n_pos rows
      LLMI_HIP(hipMemcpy2DAsync(bt_h_kvtab_[((size_t)l * LLMI_SEQ_MAX + dst) * 2 + kv], pitch,
                                bt_h_kvtab_[((size_t)l * LLMI_SEQ_MAX + src) * 2 + kv], pitch, width, (size_t)nkv_,
                                hipMemcpyDeviceToDevice, stream_));
  }
}

void Session::batch_check(const char* fn, const int32_t* tokens, const int32_t* slots, const int32_t* pos, int B,
                          int n_steps) const {
  const std::string f = std::string(fn) + ": ";
  if (!seq_reserved_) throw status_error(LLMI_E_ARG, f + "no KV slots reserved (call seq_reserve first)");
  if (score_path() != 1) throw status_error(LLMI_E_ARG, f + "the batched prefill is off (LLMI_NO_PREFILL)");
  if (B < 1 || B > n_seq_) throw status_error(LLMI_E_RANGE, f + "B must be in 1..n_seq (B)");
  if (n_steps < 0) throw status_error(LLMI_E_ARG, f + "negative step count (n_steps)");
  bool seen[LLMI_SEQ_MAX] = {};
  for (int b = 0; b < B; b++) {
    if (tokens[b] < 0 || tokens[b] >= vocab_) throw status_error(LLMI_E_RANGE, f + "token id out of range (tokens)");
    if (slots[b] < 0 || slots[b] >= n_seq_) throw status_error(LLMI_E_RANGE, f + "slot outside [0, n_seq) (slots)");
    if (seen[slots[b]]) throw status_error(LLMI_E_ARG, f + "duplicate slot in one call (slots)");
    seen[slots[b]] = true;
    if (pos[b] < 0 || pos[b] + std::max(n_steps, 1) > max_ctx_)
      throw status_error(LLMI_E_RANGE, f + "context overflow (pos + n_steps)");
  }
}

// A row at position 0 is a one-token prompt, which forward / score run as a decode step, not as a batched prompt
// (score's path 2 for n = 1: full logits, then the f64 row reduce): its final-norm row (as score_run's sc_row0_),
// lse and arg-max come from that step, run eagerly on the row's slot.  The batch step then rewrites the slot's
// K / V row 0 with the batched prefill's bits -- what a longer prompt leaves there.
void Session::batch_row0(int32_t token, int slot, int b) {
  uint16_t* dst = bt_row0_ + (size_t)b * hp_.n_embd;
  const int NL = hp_.n_layer, kpt = kernels_per_token_;
  for (int l = 0; l < NL; l++) {
    L_[(size_t)l].kc = bt_h_kvtab_[((size_t)l * LLMI_SEQ_MAX + slot) * 2];
    L_[(size_t)l].vc = bt_h_kvtab_[((size_t)l * LLMI_SEQ_MAX + slot) * 2 + 1];
  }
  auto restore = [&] {
    for (int l = 0; l < NL; l++) {
      L_[(size_t)l].kc = bt_h_kvtab_[(size_t)l * LLMI_SEQ_MAX * 2];
      L_[(size_t)l].vc = bt_h_kvtab_[(size_t)l * LLMI_SEQ_MAX * 2 + 1];
    }
    kernels_per_token_ = kpt;
  };
  try {
    set_token_pos(token, 0, true);
    record_step(stream_, false);  // STEP_LOGITS's launches
    launch_score_reduce_row(logits_, vocab_, -1, bt_r0_lse_ + LLMI_SEQ_MAX + b, bt_r0_lse_ + b, bt_r0_amax_ + b, stream_);
  } catch (...) {
    restore();
    throw;
  }
  restore();
  LLMI_HIP(hipMemcpyAsync(dst, act_.x16, (size_t)hp_.n_embd * 2, hipMemcpyDeviceToDevice, stream_));
}

bool Session::batch_step(int B, int max_pos, bool allow_f16, const std::vector<int>& row0, bool score) {
  hipStream_t s = stream_;
  const int E = hp_.n_embd;
  ensure_prefill_buffers(B);
  ensure_score_buffers(std::max(B, pf_cap_));
  if (!bt_apart_) {
    int maxhd = 0;
    for (const auto& l : L_) maxhd = std::max(maxhd, l.hd);
    bt_apart_ = dalloc<float>((size_t)nh_ * LLMI_SEQ_MAX * PREFILL_ATTN_KS_MAX * 64 * (maxhd / 2 + 2));
  }
  const bool f16_all = allow_f16 && prefill_f16_ok();
  // prefill_run's chunk with the last layer over every row (LLMI_PREFILL_FULL_LAST's / score's arithmetic); the
  // f16 / int8 GEMM choice per layer is prefill_layers', never a function of B
  prefill_layers(bt_tok_, B, max_pos, /*trim=*/false, /*last_chunk=*/false, f16_all, bt_rows_);
  launch_residual_norm_rows16(pf_out_, E, L_.back().post_ffw_norm, pf_resid_, E, out_norm_, sc_x16_, E, E, B, hp_.eps, s);
  for (int b : row0)
    LLMI_HIP(hipMemcpyAsync(sc_x16_ + (size_t)b * E, bt_row0_ + (size_t)b * E, (size_t)E * 2, hipMemcpyDeviceToDevice, s));
  if (!score) return f16_all;
  ScoreArgs a;
  a.x16 = sc_x16_;
  a.xstride = E;
  a.w16 = static_cast<const uint16_t*>(logits_w_.qs);
  a.T = B;
  a.V = vocab_;
  a.E = E;
  a.softcap = hp_.final_softcap;
  a.targets = nullptr;
  a.ms = sc_ms_;
  a.key = sc_key_;
  a.tl = sc_tl_;
  a.logprob = sc_lp_;
  a.lse = sc_lse_;
  a.argmax = sc_amax_;
  launch_score_rows(a, s);
  for (int b : row0) {  // (batch_row0)
    LLMI_HIP(hipMemcpyAsync(sc_lse_ + b, bt_r0_lse_ + b, 4, hipMemcpyDeviceToDevice, s));
    LLMI_HIP(hipMemcpyAsync(sc_amax_ + b, bt_r0_amax_ + b, 4, hipMemcpyDeviceToDevice, s));
  }
  sc_last_T_ = B;
  return f16_all;
}

void Session::batch_forward(const int32_t* tokens, const int32_t* slots, const int32_t* pos, int B, float* logits,
                            int32_t* argmax, float* lse) {
  batch_check("batch_forward", tokens, slots, pos, B, 1);
  ensure_usable();
  hipStream_t s = stream_;
  const int E = hp_.n_embd;
  std::vector<uint16_t> hx;
  // the rows idx[0..n) of the call as one step; results into the caller's arrays at those rows
  auto run = [&](const std::vector<int>& idx, bool allow_f16) -> bool {
    const int n = (int)idx.size();
    std::vector<SeqRow> rows((size_t)n);
    std::vector<int32_t> tok((size_t)n);
    std::vector<int> row0;
    int max_pos = 0;
    for (int i = 0; i < n; i++) {
      rows[(size_t)i] = SeqRow{slots[idx[(size_t)i]], pos[idx[(size_t)i]]};
      tok[(size_t)i] = tokens[idx[(size_t)i]];
      max_pos = std::max(max_pos, rows[(size_t)i].pos);
      if (rows[(size_t)i].pos == 0) {
        batch_row0(tok[(size_t)i], rows[(size_t)i].slot, i);
        row0.push_back(i);
      }
    }
    h2d(bt_rows_, rows.data(), (size_t)n * sizeof(SeqRow));
    h2d(bt_tok_, tok.data(), (size_t)n * 4);
    bt_last_rows_ = rows;
    const bool f16 = batch_step(n, max_pos, allow_f16, row0);
    hx.resize((size_t)n * E);
    std::vector<int32_t> am((size_t)n);
    std::vector<float> ls((size_t)n);
    LLMI_HIP(hipMemcpyAsync(hx.data(), sc_x16_, hx.size() * 2, hipMemcpyDeviceToHost, s));
    LLMI_HIP(hipMemcpyAsync(am.data(), sc_amax_, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    LLMI_HIP(hipMemcpyAsync(ls.data(), sc_lse_, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (logits) {  // forward's logits GEMV on the rows' f16 final-norm rows
      ensure_batch_logits(n, false);
      batch_logits(n, s);
      for (int i = 0; i < n; i++)
        LLMI_HIP(hipMemcpyAsync(logits + (size_t)idx[(size_t)i] * vocab_, bt_logits_ + (size_t)i * vocab_,
                                (size_t)vocab_ * 4, hipMemcpyDeviceToHost, s));
    }
    LLMI_HIP(hipStreamSynchronize(s));
    check_device_error();
    for (int i = 0; i < n; i++) {
      if (argmax) argmax[idx[(size_t)i]] = am[(size_t)i];
      if (lse) lse[idx[(size_t)i]] = ls[(size_t)i];
    }
    return f16;
  };
  std::vector<int> all((size_t)B);
  for (int b = 0; b < B; b++) all[(size_t)b] = b;
  if (!run(all, true)) return;
  // the f16 path (Session::prefill's rule, per row): a row whose final norm came out non-finite runs again on the
  // int8 path, which rewrites the same K / V row
  std::vector<int> bad;
  for (int b = 0; b < B; b++)
    for (int i = 0; i < E; i++)
      if (!f16_finite(hx[(size_t)b * E + i])) {
        bad.push_back(b);
        break;
      }
  if (!bad.empty()) {
    pf_f16_redo_++;
    run(bad, false);
  }
}

void Session::ensure_batch_logits(int B, bool surv) {  // grow-only, as the prefill's chunk buffers
  if (B > bt_logits_cap_) {
    bt_logits_ = dalloc<float>((size_t)B * vocab_);
    bt_logits_cap_ = B;
  }
  if (surv && B > bt_surv_cap_) {
    bt_surv_ = dalloc<unsigned long long>((size_t)B * SAMPLE_MAX_GROUPS * SAMPLE_MAX_K);
    bt_surv_cap_ = B;
  }
}

void Session::batch_logits(int B, hipStream_t s) {
  const int E = hp_.n_embd;
  if (logits_rows_rb(E) != 0) {
    launch_gemv_f16_rows(logits_w_, sc_x16_, E, B, bt_logits_, s);
  } else {  // one table read per row
    for (int i = 0; i < B; i++) {
      LLMI_HIP(hipMemcpyAsync(act_.x16, sc_x16_ + (size_t)i * E, (size_t)E * 2, hipMemcpyDeviceToDevice, s));
      launch_gemv(logits_w_, act_, bt_logits_ + (size_t)i * vocab_, GEMV_FAST, s, nullptr);
    }
  }
  if (hp_.final_softcap > 0.0f) launch_softcap(bt_logits_, B * vocab_, hp_.final_softcap, s);
}

void Session::batch_generate(const int32_t* first, const int32_t* slots, const int32_t* pos, int B, int n_steps,
                             const int32_t* stop, int n_stop, int32_t* out) {
  batch_loop("batch_generate", first, slots, pos, B, n_steps, stop, n_stop, nullptr, out);
}

void Session::batch_generate_sampled(const int32_t* first, const int32_t* slots, const int32_t* pos, int B,
                                     int n_steps, const int32_t* stop, int n_stop, const llmi_sampler* samplers,
                                     int32_t* out) {
  if (!samplers) throw status_error(LLMI_E_ARG, "batch_generate_sampled: null pointer (samplers)");
  batch_loop("batch_generate_sampled", first, slots, pos, B, n_steps, stop, n_stop, samplers, out);
}

void Session::batch_loop(const char* fn, const int32_t* first, const int32_t* slots, const int32_t* pos, int B,
                         int n_steps, const int32_t* stop, int n_stop, const llmi_sampler* samplers, int32_t* out) {
  const std::string f = std::string(fn) + ": ";
  batch_check(fn, first, slots, pos, B, n_steps);
  if (n_stop < 0 || n_stop > 4) throw status_error(LLMI_E_ARG, f + "at most 4 stop ids (n_stop)");
  if (n_stop > 0 && !stop) throw status_error(LLMI_E_ARG, f + "null pointer (stop)");
  BatchStops st{};
  st.n = n_stop;
  for (int i = 0; i < n_stop; i++) {
    if (stop[i] < 0 || stop[i] >= vocab_) throw status_error(LLMI_E_RANGE, f + "stop id out of range (stop)");
    st.id[i] = stop[i];
  }
  std::vector<SamplerDev> sp;
  bool any_greedy = false;
  if (samplers) {
    sp.resize((size_t)B);
    for (int b = 0; b < B; b++) {
      try {
        validate_sampler(samplers[b]);
      } catch (const status_error& e) {
        throw status_error(e.code, f + e.what() + " (samplers[" + std::to_string(b) + "])");
      }
      sp[(size_t)b] = SamplerDev{samplers[b].temperature, samplers[b].top_k == 0 ? LLMI_SAMPLE_MAX_K : samplers[b].top_k,
                                 samplers[b].top_p, 0, samplers[b].seed};
      any_greedy = any_greedy || samplers[b].temperature == 0.0f;
    }
    int ept = 0;
    if (sample_groups(vocab_, &ept) == 0) throw status_error(LLMI_E_ARG, f + "vocabulary over 1,048,576 rows");
  }
  ensure_usable();
  if (n_steps == 0) return;
  hipStream_t s = stream_;
  if ((size_t)n_steps * B > bt_ring_cap_) {  // grow-only, as the prefill's chunk buffers
    bt_ring_cap_ = (size_t)n_steps * B;
    bt_ring_ = dalloc<int32_t>(bt_ring_cap_);
  }
  if (samplers) {
    if (!bt_samplers_) bt_samplers_ = dalloc<SamplerDev>(LLMI_SEQ_MAX);
    ensure_batch_logits(B, true);
    h2d(bt_samplers_, sp.data(), (size_t)B * sizeof(SamplerDev));
  }
  std::vector<SeqRow> rows((size_t)B);
  std::vector<int> row0;
  int max_pos = 0;
  for (int b = 0; b < B; b++) {
    rows[(size_t)b] = SeqRow{slots[b], pos[b]};
    max_pos = std::max(max_pos, pos[b]);
    if (pos[b] == 0) {
      batch_row0(first[b], slots[b], b);
      row0.push_back(b);
    }
  }
  h2d(bt_rows_, rows.data(), (size_t)B * sizeof(SeqRow));
  h2d(bt_tok_, first, (size_t)B * 4);
  // every step's launches are enqueued at once: tokens, positions, the ids and the stop flags stay on the device
  // (max_pos + i bounds the longest live row: it only decides whether the attention's merge is launched)
  for (int i = 0; i < n_steps; i++) {
    batch_step(B, max_pos + i, true, i == 0 ? row0 : std::vector<int>(), !samplers || any_greedy);
    if (i + 1 == n_steps)  // time_kernel(10) / (11): the last step's rows as it ran them (pos -1: ended before it)
      LLMI_HIP(hipMemcpyAsync(rows.data(), bt_rows_, (size_t)B * sizeof(SeqRow), hipMemcpyDeviceToHost, s));
    if (!samplers) {
      launch_batch_feedback(sc_amax_, bt_rows_, bt_tok_, B, st, bt_ring_ + (size_t)i * B, s);
      continue;
    }
    // the rows' full logits (forward's, soft-capped), then the sampler's two launches; the second is the feedback
    batch_logits(B, s);
    launch_sample_select_rows(bt_logits_, vocab_, B, bt_samplers_, bt_rows_, bt_surv_, s);
    launch_sample_finalize_rows(bt_surv_, vocab_, B, bt_samplers_, sc_amax_, bt_rows_, bt_tok_, st,
                                bt_ring_ + (size_t)i * B, true, s);
  }
  LLMI_HIP(hipMemcpyAsync(out, bt_ring_, (size_t)n_steps * B * 4, hipMemcpyDeviceToHost, s));
  LLMI_HIP(hipStreamSynchronize(s));
  bt_last_rows_ = rows;
  if (samplers) {
    bt_samp_B_ = B;
    bt_samp_rows_ = rows;
  }
  check_device_error();
}

// time_kernel(11): the multi-row logits GEMV + select + finalize (no feedback) over the most recent sampled batch
// step's rows, with that call's samplers; the final-norm rows are whatever sc_x16_ holds now
void Session::time_batch_sampling(int reps, double* us, double* bytes) {
  *us = *bytes = 0.0;
  const int B = bt_samp_B_, E = hp_.n_embd;
  if (B == 0 || reps <= 0) return;
  hipStream_t s = stream_;
  h2d(bt_trows_, bt_samp_rows_.data(), (size_t)B * sizeof(SeqRow));
  const int rb = logits_rows_rb(E);
  const BatchStops st{};
  std::vector<hipEvent_t> ev(2 * (size_t)reps);
  for (auto& e : ev) LLMI_HIP(hipEventCreate(&e));
  LLMI_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < reps; r++) {
    LLMI_HIP(hipEventRecord(ev[2 * (size_t)r], s));
    batch_logits(B, s);
    launch_sample_select_rows(bt_logits_, vocab_, B, bt_samplers_, bt_trows_, bt_surv_, s);
    launch_sample_finalize_rows(bt_surv_, vocab_, B, bt_samplers_, sc_amax_, bt_trows_, bt_tok_, st, bt_ring_, false, s);
    LLMI_HIP(hipEventRecord(ev[2 * (size_t)r + 1], s));
  }
  LLMI_HIP(hipStreamSynchronize(s));
  double tot = 0;
  for (int r = 0; r < reps; r++) {
    float ms = 0;
    LLMI_HIP(hipEventElapsedTime(&ms, ev[2 * (size_t)r], ev[2 * (size_t)r + 1]));
    tot += ms;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *us = tot * 1000.0 / reps;
  const int reads = rb ? (B + rb - 1) / rb : B;
  *bytes = (double)reads * (double)logits_w_.bytes + (double)B * vocab_ * 4.0;
}

void Session::time_batch_attn(int reps, double* us, double* bytes) {
  *us = *bytes = 0.0;
  const int NL = hp_.n_layer, B = (int)bt_last_rows_.size();
  if (B == 0 || (int)bt_last_attn_.size() != NL || reps <= 0) return;
  hipStream_t s = stream_;
  h2d(bt_trows_, bt_last_rows_.data(), (size_t)B * sizeof(SeqRow));
  int max_pos = 0;
  double by = 0.0;
  for (const auto& r : bt_last_rows_) max_pos = std::max(max_pos, r.pos);
  for (int l = 0; l < NL; l++)
    for (const auto& r : bt_last_rows_) by += r.pos < 0 ? 0.0 : (double)(r.pos + 1) * 2.0 * nkv_ * L_[(size_t)l].hd * 2.0;
  std::vector<hipEvent_t> ev(2 * (size_t)reps);
  for (auto& e : ev) LLMI_HIP(hipEventCreate(&e));
  LLMI_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < reps; r++) {
    LLMI_HIP(hipEventRecord(ev[2 * (size_t)r], s));
    for (int l = 0; l < NL; l++) {  // the launches write only the step's scratch rows (the o projection's x)
      PrefillAttn at = bt_last_attn_[(size_t)l];
      at.rows = bt_trows_;
      at.pos0 = max_pos;
      launch_prefill_attn(at, B, s);
    }
    LLMI_HIP(hipEventRecord(ev[2 * (size_t)r + 1], s));
  }
  LLMI_HIP(hipStreamSynchronize(s));
  double tot = 0;
  for (int r = 0; r < reps; r++) {
    float ms = 0;
    LLMI_HIP(hipEventElapsedTime(&ms, ev[2 * (size_t)r], ev[2 * (size_t)r + 1]));
    tot += ms;
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  *us = tot * 1000.0 / reps / NL;
  *bytes = by / NL;
}

}  // namespace llmi
