// session_batch.cpp -- several sequences per step (llmi_session_seq_* / llmi_session_batch_*).
// A batch step is the batched prefill's launch sequence over B token rows (Session::prefill_layers), each row a
// position of its own KV slot, then the scorer's rows; the greedy loop adds one feedback launch per step, the
// sampled loop (section 13) the rows' full logits and the sampler's two multi-row launches.  A ragged step
// (llmi_session_batch_extend, section 14) carries spans of consecutive tokens: prompt chunks and draft tokens beside
// decode rows, the attention in its span form.  The lookup loop (llmi_session_batch_generate_lookup, section 15) runs
// such steps with the tables written on the device: n-gram drafts verified and accepted without leaving it; with a
// sampler per row (llmi_session_batch_generate_lookup_sampled, section 16) a draft is accepted against the row's seeded
// draw, from the logits of the step's live token rows only.
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
    check_slot(f, slots[b], seen);
    if (pos[b] < 0 || pos[b] + std::max(n_steps, 1) > max_ctx_)
      throw status_error(LLMI_E_RANGE, f + "context overflow (pos + n_steps)");
  }
}

void Session::check_slot(const std::string& f, int slot, bool* seen, bool span) const {
  if (slot < 0 || slot >= n_seq_)
    throw status_error(LLMI_E_RANGE, f + (span ? "slot outside [0, n_seq) (spans.slot)" : "slot outside [0, n_seq) (slots)"));
  if (seen[slot])
    throw status_error(LLMI_E_ARG, f + (span ? "duplicate slot in one call (spans.slot)" : "duplicate slot in one call (slots)"));
  seen[slot] = true;
}

void Session::stop_ids(const std::string& f, const int32_t* stop, int n_stop, int32_t* id) const {
  if (n_stop < 0 || n_stop > 4) throw status_error(LLMI_E_ARG, f + "at most 4 stop ids (n_stop)");
  if (n_stop > 0 && !stop) throw status_error(LLMI_E_ARG, f + "null pointer (stop)");
  for (int i = 0; id && i < n_stop; i++) {  // (id null: the count and the pointer only)
    if (stop[i] < 0 || stop[i] >= vocab_) throw status_error(LLMI_E_RANGE, f + "stop id out of range (stop)");
    id[i] = stop[i];
  }
}

Session::RowSamplers Session::row_samplers(const std::string& f, const llmi_sampler* samplers, int B) {
  RowSamplers r;
  r.dev.resize((size_t)B);
  for (int b = 0; b < B; b++) {
    try {
      validate_sampler(samplers[b]);
    } catch (const status_error& e) {
      throw status_error(e.code, f + e.what() + " (samplers[" + std::to_string(b) + "])");
    }
    r.dev[(size_t)b] = sampler_dev(samplers[b]);
    r.any_greedy = r.any_greedy || samplers[b].temperature == 0.0f;
    r.sampled = r.sampled || samplers[b].temperature > 0.0f;
  }
  return r;
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
  {
    ScopeExit restore{[&] {
      for (int l = 0; l < NL; l++) {
        L_[(size_t)l].kc = bt_h_kvtab_[(size_t)l * LLMI_SEQ_MAX * 2];
        L_[(size_t)l].vc = bt_h_kvtab_[(size_t)l * LLMI_SEQ_MAX * 2 + 1];
      }
      kernels_per_token_ = kpt;
    }};
    set_token_pos(token, 0, true);
    record_step(stream_, false);  // STEP_LOGITS's launches
    launch_score_reduce_row(logits_, vocab_, -1, bt_r0_lse_ + LLMI_SEQ_MAX + b, bt_r0_lse_ + b, bt_r0_amax_ + b, stream_);
  }
  LLMI_HIP(hipMemcpyAsync(dst, act_.x16, (size_t)hp_.n_embd * 2, hipMemcpyDeviceToDevice, stream_));
}

void Session::ensure_batch_apart() {
  if (!bt_apart_) bt_apart_ = dalloc<float>((size_t)nh_ * LLMI_SEQ_MAX * PREFILL_ATTN_KS_MAX * 64 * (max_hd_ / 2 + 2));
}

void Session::step_tail(uint16_t* x16, const OutRun* runs, size_t n_runs, const std::vector<OutRow0>& r0, bool score) {
  hipStream_t s = stream_;
  const int E = hp_.n_embd;
  int n = 0;
  for (size_t i = 0; i < n_runs; i++) {
    const OutRun& o = runs[i];
    launch_residual_norm_rows16(pf_out_ + (size_t)o.row0 * E, E, L_.back().post_ffw_norm, pf_resid_ + (size_t)o.row0 * E,
                                E, out_norm_, x16 + (size_t)o.o0 * E, E, E, o.n, hp_.eps, s);
    n += o.n;
  }
  for (const OutRow0& p : r0)
    LLMI_HIP(hipMemcpyAsync(x16 + (size_t)p.o * E, bt_row0_ + (size_t)p.k * E, (size_t)E * 2, hipMemcpyDeviceToDevice, s));
  if (!score) return;
  launch_score_rows(score_args(x16, n, nullptr), s);
  for (const OutRow0& p : r0) {  // (batch_row0)
    if (!p.single) continue;
    LLMI_HIP(hipMemcpyAsync(sc_lse_ + p.o, bt_r0_lse_ + p.k, 4, hipMemcpyDeviceToDevice, s));
    LLMI_HIP(hipMemcpyAsync(sc_amax_ + p.o, bt_r0_amax_ + p.k, 4, hipMemcpyDeviceToDevice, s));
  }
}

bool Session::batch_step(int B, int max_pos, bool allow_f16, const std::vector<OutRow0>& row0, bool score) {
  ensure_prefill_buffers(B);
  ensure_score_buffers(std::max(B, pf_cap_));
  ensure_batch_apart();
  const bool f16_all = allow_f16 && prefill_f16_ok();
  // prefill_run's chunk with the last layer over every row (LLMI_PREFILL_FULL_LAST's / score's arithmetic); the
  // f16 / int8 GEMM choice per layer is prefill_layers', never a function of B
  prefill_layers(bt_tok_, B, max_pos, /*trim=*/false, /*last_chunk=*/false, f16_all, bt_rows_);
  const OutRun all{0, B, 0, 0, 0};
  step_tail(sc_x16_, &all, 1, row0, score);
  if (score) sc_last_T_ = B;
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
    std::vector<OutRow0> row0;
    int max_pos = 0;
    for (int i = 0; i < n; i++) {
      rows[(size_t)i] = SeqRow{slots[idx[(size_t)i]], pos[idx[(size_t)i]]};
      tok[(size_t)i] = tokens[idx[(size_t)i]];
      max_pos = std::max(max_pos, rows[(size_t)i].pos);
      if (rows[(size_t)i].pos == 0) {
        batch_row0(tok[(size_t)i], rows[(size_t)i].slot, i);
        row0.push_back(OutRow0{i, i, true});
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

// The attention of a multi-sequence step.  The per-token form's partials (bt_apart_) hold LLMI_SEQ_MAX rows: a span
// step routed through it (LLMI_BATCH_SPAN_ROWS=1) goes that many rows at a time -- a row's bits do not depend on
// which launch carries it.
void Session::launch_batch_attn(const PrefillAttn& at, int T, hipStream_t s) {
  if (at.blocks || T <= LLMI_SEQ_MAX) return launch_prefill_attn(at, T, s);
  for (int c0 = 0; c0 < T; c0 += LLMI_SEQ_MAX) {
    PrefillAttn c = at;
    c.q += (size_t)c0 * at.n_head * at.head_dim;
    c.xq += (size_t)c0 * at.xstride;
    if (c.x16) c.x16 += (size_t)c0 * at.x16stride;
    c.rows += c0;
    launch_prefill_attn(c, std::min(LLMI_SEQ_MAX, T - c0), s);
  }
}

void Session::ensure_extend_buffers() {
  const int E = hp_.n_embd;
  if (!bx_rows_) {
    const size_t max_blocks = LLMI_SEQ_MAX + LLMI_BATCH_TOKENS_MAX / 32;
    bx_rows_ = dalloc<SeqRow>(LLMI_BATCH_TOKENS_MAX);
    bx_tok_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX);
    bx_blocks_ = dalloc<AttnBlock>(max_blocks);
    bx_apart_ = dalloc<float>((size_t)nh_ * max_blocks * PREFILL_ATTN_KS_MAX * 64 * (max_hd_ / 2 + 2));
    bx_x16_ = dalloc<uint16_t>((size_t)LLMI_BATCH_TOKENS_MAX * E);
  }
  ensure_batch_apart();  // (the per-token form's partials, as batch_step)
}

// A ragged batch step: the batched prefill's launch sequence over the spans' token rows -- the
// q/k launch with one SeqRow per token row, the attention in its span form (one query block per 32 consecutive
// tokens of a span) -- then the final norm, the scorer and the logits GEMV over the output rows only.
void Session::batch_extend(const int32_t* tokens, const llmi_span* spans, int n_spans, float* logits, int32_t* argmax,
                           float* lse) {
  const std::string f = "batch_extend: ";
  if (!seq_reserved_) throw status_error(LLMI_E_ARG, f + "no KV slots reserved (call seq_reserve first)");
  if (score_path() != 1) throw status_error(LLMI_E_ARG, f + "the batched prefill is off (LLMI_NO_PREFILL)");
  if (n_spans < 1 || n_spans > n_seq_) throw status_error(LLMI_E_RANGE, f + "n_spans must be in 1..n_seq (n_spans)");
  bool seen[LLMI_SEQ_MAX] = {};
  int total = 0, n_out_all = 0;
  std::vector<int> tok_off((size_t)n_spans), out_off((size_t)n_spans);
  for (int i = 0; i < n_spans; i++) {
    const llmi_span& sp = spans[i];
    check_slot(f, sp.slot, seen, /*span=*/true);
    if (sp.n_tokens < 1) throw status_error(LLMI_E_ARG, f + "a span needs at least one token (spans.n_tokens)");
    if (sp.out < LLMI_SPAN_LAST || sp.out > LLMI_SPAN_NONE)
      throw status_error(LLMI_E_ARG, f + "out must be LLMI_SPAN_LAST, _ALL or _NONE (spans.out)");
    if (sp.n_tokens > LLMI_BATCH_TOKENS_MAX - total)
      throw status_error(LLMI_E_RANGE, f + "more than " + std::to_string(LLMI_BATCH_TOKENS_MAX) +
                                           " token rows in one call (sum of spans.n_tokens)");
    if (sp.pos < 0 || sp.pos > max_ctx_ - sp.n_tokens)
      throw status_error(LLMI_E_RANGE, f + "context overflow (spans.pos + n_tokens)");
    tok_off[(size_t)i] = total;
    out_off[(size_t)i] = n_out_all;
    total += sp.n_tokens;
    n_out_all += sp.out == LLMI_SPAN_ALL ? sp.n_tokens : sp.out == LLMI_SPAN_LAST ? 1 : 0;
  }
  for (int t = 0; t < total; t++)
    if (tokens[t] < 0 || tokens[t] >= vocab_) throw status_error(LLMI_E_RANGE, f + "token id out of range (tokens)");
  ensure_usable();
  hipStream_t s = stream_;
  const int E = hp_.n_embd;
  ensure_extend_buffers();
  // A/B, read at the call: the step's attention through the per-token multi-sequence form, one SeqRow per token row
  // (legal because the q/k launch has appended the step's K/V before it; the same bits)
  const char* sr_env = getenv("LLMI_BATCH_SPAN_ROWS");
  const bool span_rows = sr_env && atoi(sr_env) == 1;
  std::vector<uint16_t> hx;
  std::vector<int> bad;  // the last step's spans with a non-finite output row
  // the spans idx[0..n) of the call as one step; results into the caller's arrays at those spans' output entries
  auto run = [&](const std::vector<int>& idx, bool allow_f16) -> bool {
    std::vector<SeqRow> rows;
    std::vector<int32_t> tok;
    std::vector<AttnBlock> blocks;
    std::vector<OutRun> outs;  // a span's output rows
    std::vector<OutRow0> r0;   // (single: a one-token span)
    int max_pos = 0, n_out = 0;
    for (int k = 0; k < (int)idx.size(); k++) {
      const llmi_span& sp = spans[idx[(size_t)k]];
      const int32_t* st = tokens + tok_off[(size_t)idx[(size_t)k]];
      const int t0 = (int)rows.size();
      for (int j = 0; j < sp.n_tokens; j++) {
        rows.push_back(SeqRow{sp.slot, sp.pos + j});
        tok.push_back(st[j]);
      }
      for (int j = 0; j < sp.n_tokens; j += 32)
        blocks.push_back(AttnBlock{t0 + j, std::min(32, sp.n_tokens - j), sp.slot, sp.pos + j});
      max_pos = std::max(max_pos, sp.pos + sp.n_tokens - 1);
      if (sp.out == LLMI_SPAN_NONE) continue;
      const int n = sp.out == LLMI_SPAN_ALL ? sp.n_tokens : 1;
      outs.push_back(OutRun{t0 + sp.n_tokens - n, n, n_out, idx[(size_t)k], out_off[(size_t)idx[(size_t)k]]});
      // an output row at position 0 is forward's / score's one-token step (batch_row0); the step below then rewrites
      // the slot's K / V row 0 with the batched prefill's bits.  As score() does it: a one-token span's lse / arg-max
      // are that step's (the f64 row reduce, score's one-token call); a longer span hands the step's final-norm row
      // to the fused scorer with its other rows (score_chunk's sc_row0_)
      if (sp.pos + sp.n_tokens - n == 0) {
        batch_row0(st[0], sp.slot, k);
        r0.push_back(OutRow0{n_out, k, sp.n_tokens == 1});
      }
      n_out += n;
    }
    const int T = (int)rows.size();
    // heaviest query blocks first: dispatch order is a speed matter only
    std::stable_sort(blocks.begin(), blocks.end(),
                     [](const AttnBlock& a, const AttnBlock& b) { return a.pos + a.n > b.pos + b.n; });
    h2d(bx_rows_, rows.data(), (size_t)T * sizeof(SeqRow));
    h2d(bx_tok_, tok.data(), (size_t)T * 4);
    h2d(bx_blocks_, blocks.data(), blocks.size() * sizeof(AttnBlock));
    ensure_prefill_buffers(T);
    const bool f16_all = allow_f16 && prefill_f16_ok();
    {  // the last layer over every row, as batch_step
      bx_step_ = true;
      ScopeExit off{[&] { bx_step_ = false; }};
      prefill_layers(bx_tok_, T, max_pos, /*trim=*/false, /*last_chunk=*/false, f16_all, bx_rows_,
                     span_rows ? nullptr : bx_blocks_, span_rows ? 0 : (int)blocks.size());
    }
    bx_last_rows_ = rows;
    bx_last_blocks_ = blocks;
    if (n_out == 0) {  // no final norm, no scorer, no GEMV (and no f16 check, like batch_generate)
      LLMI_HIP(hipStreamSynchronize(s));
      check_device_error();
      return false;
    }
    ensure_score_buffers(std::max(n_out, pf_cap_));
    // the output rows' final-norm rows, compact in span order, and the scorer over them
    step_tail(bx_x16_, outs.data(), outs.size(), r0, /*score=*/true);
    hx.resize((size_t)n_out * E);
    std::vector<int32_t> am((size_t)n_out);
    std::vector<float> ls((size_t)n_out);
    LLMI_HIP(hipMemcpyAsync(hx.data(), bx_x16_, hx.size() * 2, hipMemcpyDeviceToHost, s));
    LLMI_HIP(hipMemcpyAsync(am.data(), sc_amax_, (size_t)n_out * 4, hipMemcpyDeviceToHost, s));
    LLMI_HIP(hipMemcpyAsync(ls.data(), sc_lse_, (size_t)n_out * 4, hipMemcpyDeviceToHost, s));
    if (logits) {  // forward's logits GEMV on the compact rows, LLMI_SEQ_MAX of them at a time (bt_logits_'s size)
      ensure_batch_logits(std::min(n_out, LLMI_SEQ_MAX), false);
      for (const OutRun& o : outs)
        for (int c0 = 0; c0 < o.n; c0 += LLMI_SEQ_MAX) {
          const int n = std::min(LLMI_SEQ_MAX, o.n - c0);
          batch_logits(n, s, bx_x16_ + (size_t)(o.o0 + c0) * E);
          LLMI_HIP(hipMemcpyAsync(logits + (size_t)(o.dst + c0) * vocab_, bt_logits_, (size_t)n * vocab_ * 4,
                                  hipMemcpyDeviceToHost, s));
        }
    }
    LLMI_HIP(hipStreamSynchronize(s));
    check_device_error();
    for (const OutRun& o : outs)
      for (int j = 0; j < o.n; j++) {
        if (argmax) argmax[o.dst + j] = am[(size_t)(o.o0 + j)];
        if (lse) lse[o.dst + j] = ls[(size_t)(o.o0 + j)];
      }
    bad.clear();
    for (const OutRun& o : outs)
      for (size_t i = (size_t)o.o0 * E; i < (size_t)(o.o0 + o.n) * E; i++)
        if (!f16_finite(hx[i])) {
          bad.push_back(o.span);
          break;
        }
    return f16_all;
  };
  std::vector<int> all((size_t)n_spans);
  for (int i = 0; i < n_spans; i++) all[(size_t)i] = i;
  if (!run(all, true)) return;
  // the f16 path (Session::prefill's rule, per span): a span with a non-finite output row runs again as a smaller
  // step on the int8 path, all of its token rows, rewriting the same K / V rows
  if (!bad.empty()) {
    pf_f16_redo_++;
    run(std::vector<int>(bad), false);
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

void Session::batch_logits(int B, hipStream_t s, const uint16_t* x16) {
  const int E = hp_.n_embd;
  if (!x16) x16 = sc_x16_;
  if (logits_rows_rb(E) != 0) {
    launch_gemv_f16_rows(logits_w_, x16, E, B, bt_logits_, s);
  } else {  // one table read per row
    for (int i = 0; i < B; i++) {
      LLMI_HIP(hipMemcpyAsync(act_.x16, x16 + (size_t)i * E, (size_t)E * 2, hipMemcpyDeviceToDevice, s));
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
  BatchStops st{};
  st.n = n_stop;
  stop_ids(f, stop, n_stop, st.id);
  RowSamplers sp;
  if (samplers) {
    sp = row_samplers(f, samplers, B);
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
    h2d(bt_samplers_, sp.dev.data(), (size_t)B * sizeof(SamplerDev));
  }
  std::vector<SeqRow> rows((size_t)B);
  std::vector<OutRow0> row0;
  const std::vector<OutRow0> none;
  int max_pos = 0;
  for (int b = 0; b < B; b++) {
    rows[(size_t)b] = SeqRow{slots[b], pos[b]};
    max_pos = std::max(max_pos, pos[b]);
    if (pos[b] == 0) {
      batch_row0(first[b], slots[b], b);
      row0.push_back(OutRow0{b, b, true});
    }
  }
  h2d(bt_rows_, rows.data(), (size_t)B * sizeof(SeqRow));
  h2d(bt_tok_, first, (size_t)B * 4);
  // every step's launches are enqueued at once: tokens, positions, the ids and the stop flags stay on the device
  // (max_pos + i bounds the longest live row: it only decides whether the attention's merge is launched)
  for (int i = 0; i < n_steps; i++) {
    batch_step(B, max_pos + i, true, i == 0 ? row0 : none, !samplers || sp.any_greedy);
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

// Lookup decoding.  A step is batch_extend's launch sequence over B spans of draft_len + 1 token
// rows -- prefill_layers with the span attention, the final norm and the scorer over every row -- whose tables
// lookup_step_kernel writes on the device; the same launch accepts the step just scored.  Steps are enqueued in groups
// and only the B done flags come back between groups.  f16 overflow: as batch_generate, the loop does not leave the
// device and does not check.
void Session::batch_generate_lookup(const int32_t* hist, const int32_t* hist_len, const int32_t* slots,
                                    const int32_t* pos, int B, const llmi_lookup& lk, int max_steps, const int32_t* stop,
                                    int n_stop, int32_t* out, int32_t* n_out, llmi_lookup_stats* stats) {
  lookup_loop("batch_generate_lookup", hist, hist_len, slots, pos, B, lk, max_steps, stop, n_stop, nullptr, out, n_out,
              stats);
}

// Sampled rows: the sampler is a pure function of a token row's logits, the row's sampler and
// the token row's position, so the id the sampled batch loop would emit at every position of a draft span is computed
// for all of the span's rows at once and lookup_step_kernel accepts against those ids in place of the arg-max.  Only
// the step's live token rows of sampled rows need logits: the device lists them and the gathered GEMV reads the table
// once per logits_rows_rb of them, LLMI_SEQ_MAX compact rows per launch into bt_logits_.
void Session::batch_generate_lookup_sampled(const int32_t* hist, const int32_t* hist_len, const int32_t* slots,
                                            const int32_t* pos, int B, const llmi_lookup& lk, int max_steps,
                                            const int32_t* stop, int n_stop, const llmi_sampler* samplers, int32_t* out,
                                            int32_t* n_out, llmi_lookup_stats* stats) {
  if (!samplers) throw status_error(LLMI_E_ARG, "batch_generate_lookup_sampled: null pointer (samplers)");
  lookup_loop("batch_generate_lookup_sampled", hist, hist_len, slots, pos, B, lk, max_steps, stop, n_stop, samplers, out,
              n_out, stats);
}

void Session::lookup_select(const SeqRow* trows, int T, int W, bool gather, bool any_greedy, int32_t* live, int32_t* ids,
                            SeqRow* snap, hipStream_t s) {
  const int E = hp_.n_embd;
  LiveRowsArgs la;
  la.trows = trows;
  la.sp = lk_samplers_;
  la.T = T;
  la.W = W;
  la.all = gather ? 0 : 1;
  la.idx = live;
  la.n_live = live + LLMI_BATCH_TOKENS_MAX;
  la.argmax = any_greedy ? sc_amax_ : nullptr;
  la.ids = ids;
  la.snap = snap;
  launch_lookup_live_rows(la, s);
  TokenRowsArgs ta;
  ta.n_live = la.n_live;
  ta.W = W;
  ta.sp = lk_samplers_;
  ta.trows = trows;
  // every chunk is enqueued: the host does not know the count, and a chunk past it costs its work-groups' return
  for (int c0 = 0; c0 < T; c0 += LLMI_SEQ_MAX) {
    const int n = std::min(LLMI_SEQ_MAX, T - c0);
    if (gather) {
      launch_gemv_f16_rows_gather(logits_w_, sc_x16_, E, live + c0, la.n_live, c0, n, bt_logits_, s);
      if (hp_.final_softcap > 0.0f) launch_softcap_live_rows(bt_logits_, vocab_, n, la.n_live, c0, hp_.final_softcap, s);
    } else {  // every token row, listed or not (the list is the identity)
      batch_logits(n, s, sc_x16_ + (size_t)c0 * E);
    }
    ta.idx = live + c0;
    ta.base = c0;
    ta.cap = n;
    launch_sample_select_token_rows(bt_logits_, vocab_, ta, bt_surv_, s);
    launch_sample_finalize_token_rows(bt_surv_, vocab_, ta, ids, s);
  }
}

void Session::lookup_loop(const char* fn, const int32_t* hist, const int32_t* hist_len, const int32_t* slots,
                          const int32_t* pos, int B, const llmi_lookup& lk, int max_steps, const int32_t* stop,
                          int n_stop, const llmi_sampler* samplers, int32_t* out, int32_t* n_out,
                          llmi_lookup_stats* stats) {
  const std::string f = std::string(fn) + ": ";
  if (!seq_reserved_) throw status_error(LLMI_E_ARG, f + "no KV slots reserved (call seq_reserve first)");
  if (score_path() != 1) throw status_error(LLMI_E_ARG, f + "the batched prefill is off (LLMI_NO_PREFILL)");
  if (B < 1 || B > n_seq_) throw status_error(LLMI_E_RANGE, f + "B must be in 1..n_seq (B)");
  stop_ids(f, stop, n_stop, nullptr);  // (the ids' range is checked where it always was, below)
  if (lk.draft_len < 1 || lk.draft_len > LOOKUP_DRAFT_MAX)
    throw status_error(LLMI_E_RANGE, f + "draft_len must be in 1..31 (draft_len)");
  if (lk.ngram_max < 1 || lk.ngram_max > LOOKUP_NGRAM_MAX)
    throw status_error(LLMI_E_RANGE, f + "ngram_max must be in 1..8 (ngram_max)");
  if (lk.ngram_min < 1 || lk.ngram_min > lk.ngram_max)
    throw status_error(LLMI_E_RANGE, f + "ngram_min must be in 1..ngram_max (ngram_min)");
  if (lk.max_new < 1) throw status_error(LLMI_E_RANGE, f + "max_new must be at least 1 (max_new)");
  if (B * (lk.draft_len + 1) > LLMI_BATCH_TOKENS_MAX)
    throw status_error(LLMI_E_RANGE, f + "more than " + std::to_string(LLMI_BATCH_TOKENS_MAX) +
                                         " token rows in one step (B * (draft_len + 1))");
  if (max_steps < 0) throw status_error(LLMI_E_ARG, f + "negative step count (max_steps)");
  LookupArgs a;
  a.n_stop = n_stop;
  stop_ids(f, stop, n_stop, a.stop);
  const int D = lk.draft_len, W = D + 1, T = B * W, max_new = lk.max_new;
  bool seen[LLMI_SEQ_MAX] = {};
  size_t n_hist = 0, hist_cap = 0;
  int p0 = 0;
  for (int b = 0; b < B; b++) {
    check_slot(f, slots[b], seen);
    if (hist_len[b] < 1) throw status_error(LLMI_E_RANGE, f + "a history needs at least one token (hist_len)");
    // a position-0 row is a one-token prompt, which forward / score run as a decode step (batch_row0): batch_generate
    // runs it before its loop, a lookup step would need it inside
    if (pos[b] < 1)
      throw status_error(LLMI_E_RANGE, f + "a row must start at position 1 or later: position 0 is a one-token prompt, "
                                           "which runs as a decode step the lookup loop does not have (pos)");
    if (pos[b] > max_ctx_ - max_new) throw status_error(LLMI_E_RANGE, f + "context overflow (pos + max_new)");
    n_hist += (size_t)hist_len[b];
    hist_cap += (size_t)hist_len[b] + (size_t)max_new;
    p0 = std::max(p0, pos[b] + max_new - 1);
  }
  for (size_t i = 0; i < n_hist; i++)
    if (hist[i] < 0 || hist[i] >= vocab_) throw status_error(LLMI_E_RANGE, f + "token id out of range (hist)");
  RowSamplers sp;
  if (samplers) {
    sp = row_samplers(f, samplers, B);
    int ept = 0;  // (only a row that draws needs the sampler: all-greedy samplers are the greedy call)
    if (sp.sampled && sample_groups(vocab_, &ept) == 0)
      throw status_error(LLMI_E_ARG, f + "vocabulary over 1,048,576 rows");
  }
  const bool any_greedy = sp.any_greedy, sampled = sp.sampled;
  // (samplers that are all greedy: the greedy loop's launches, nothing else)
  // A/B, read at the call: the logits of every token row, without the list (also the table widths the multi-row
  // GEMV does not take, through batch_logits' row-by-row path)
  const char* ng_env = getenv("LLMI_LOOKUP_NO_GATHER");
  const bool gather = !(ng_env && atoi(ng_env) == 1) && logits_rows_rb(hp_.n_embd) != 0;
  ensure_usable();
  int group = 4;
  if (const char* c = getenv("LLMI_LOOKUP_SYNC")) group = std::max(1, atoi(c));
  const int cap_steps = max_steps == 0 ? max_new : max_steps;
  hipStream_t s = stream_;
  ensure_extend_buffers();
  if (!lk_rowst_) {
    lk_rowst_ = dalloc<LookupRow>(LLMI_SEQ_MAX);
    lk_done_ = dalloc<int32_t>(LLMI_SEQ_MAX);
    lk_tok_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX);
    lk_trows_ = dalloc<SeqRow>(LLMI_BATCH_TOKENS_MAX);
    lk_blocks_ = dalloc<AttnBlock>(LLMI_SEQ_MAX);
    lk_ttok_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX);
    lk_ttrows_ = dalloc<SeqRow>(LLMI_BATCH_TOKENS_MAX);
    lk_tblocks_ = dalloc<AttnBlock>(LLMI_SEQ_MAX);
  }
  if (hist_cap > lk_hist_cap_) {  // grow-only, as the prefill's chunk buffers
    lk_hist_cap_ = std::max(hist_cap, 2 * lk_hist_cap_);
    lk_hist_ = dalloc<int32_t>(lk_hist_cap_);
  }
  if ((size_t)B * max_new > lk_out_cap_) {
    lk_out_cap_ = std::max((size_t)B * max_new, 2 * lk_out_cap_);
    lk_out_ = dalloc<int32_t>(lk_out_cap_);
  }
  lk_last_.B = 0;  // (until this call has run a step: time_kernel(13) reads the buffers above)
  if (sampled) {
    if (!lk_ids_) {
      lk_ids_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX);
      lk_live_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX + 1);
      lk_snap_ = dalloc<SeqRow>(LLMI_BATCH_TOKENS_MAX);
      lk_tids_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX);
      lk_tlive_ = dalloc<int32_t>(LLMI_BATCH_TOKENS_MAX + 1);
      lk_samplers_ = dalloc<SamplerDev>(LLMI_SEQ_MAX);
    }
    lk_samp_.T = 0;
    ensure_batch_logits(std::min(LLMI_SEQ_MAX, B * (lk.draft_len + 1)), true);
    h2d(lk_samplers_, sp.dev.data(), (size_t)B * sizeof(SamplerDev));
  }
  // the histories once, each into its own buffer of hist_len + max_new tokens, and the rows' state
  std::vector<int32_t> hbuf(hist_cap, 0);
  std::vector<LookupRow> st((size_t)B);
  size_t src = 0, dst = 0;
  for (int b = 0; b < B; b++) {
    std::memcpy(hbuf.data() + dst, hist + src, (size_t)hist_len[b] * 4);
    LookupRow r{};
    r.hist = lk_hist_ + dst;
    r.len = hist_len[b];
    r.cap = hist_len[b] + max_new;
    r.slot = slots[b];
    r.pos = pos[b];
    r.remaining = max_new;
    r.match_end = -1;
    st[(size_t)b] = r;
    src += (size_t)hist_len[b];
    dst += (size_t)r.cap;
  }
  h2d(lk_hist_, hbuf.data(), hist_cap * 4);
  h2d(lk_rowst_, st.data(), (size_t)B * sizeof(LookupRow));
  LLMI_HIP(hipMemsetAsync(lk_out_, 0xFF, (size_t)B * max_new * 4, s));  // -1 past n_out
  ensure_prefill_buffers(T);
  ensure_score_buffers(std::max(T, pf_cap_));
  a.rows = lk_rowst_;
  a.B = B;
  a.D = D;
  a.ngram_max = lk.ngram_max;
  a.ngram_min = lk.ngram_min;
  a.argmax = sampled ? lk_ids_ : sc_amax_;  // the ids the accept compares the drafts with
  a.tok = lk_tok_;
  a.trows = lk_trows_;
  a.blocks = lk_blocks_;
  a.out = lk_out_;
  a.max_new = max_new;
  a.done = lk_done_;
  a.mode = LOOKUP_DRAFT;  // the first step's draft and tables
  launch_lookup_step(a, s);
  a.mode = LOOKUP_STEP;
  const OutRun all{0, T, 0, 0, 0};
  const std::vector<OutRow0> none;  // (no row starts at position 0)
  const bool f16_all = prefill_f16_ok();
  std::vector<int32_t> flags((size_t)B, 0);
  {
    // the span attention's launches are recorded for time_kernel(12), which times batch_extend's steps: kept as they were
    std::vector<PrefillAttn> keep_attn = bx_last_attn_;
    bx_step_ = true;
    ScopeExit off{[&] {
      bx_step_ = false;
      bx_last_attn_ = std::move(keep_attn);
    }};
    bool all_done = false;
    for (int n_run = 0; n_run < cap_steps && !all_done;) {
      const int g = std::min(group, cap_steps - n_run);
      for (int i = 0; i < g; i++) {
        // p0: the last position any row may reach, a bound for the attention's merge launch (as batch_loop's)
        prefill_layers(lk_tok_, T, p0, /*trim=*/false, /*last_chunk=*/false, f16_all, lk_trows_, lk_blocks_, B);
        step_tail(sc_x16_, &all, 1, none, /*score=*/!sampled || any_greedy);
        if (sampled) lookup_select(lk_trows_, T, W, gather, any_greedy, lk_live_, lk_ids_, lk_snap_, s);
        launch_lookup_step(a, s);
      }
      n_run += g;
      LLMI_HIP(hipMemcpyAsync(flags.data(), lk_done_, (size_t)B * 4, hipMemcpyDeviceToHost, s));
      LLMI_HIP(hipStreamSynchronize(s));
      all_done = true;
      for (int b = 0; b < B; b++) all_done = all_done && flags[(size_t)b] != 0;
    }
  }
  sc_last_T_ = T;
  LLMI_HIP(hipMemcpyAsync(st.data(), lk_rowst_, (size_t)B * sizeof(LookupRow), hipMemcpyDeviceToHost, s));
  LLMI_HIP(hipMemcpyAsync(out, lk_out_, (size_t)B * max_new * 4, hipMemcpyDeviceToHost, s));
  LLMI_HIP(hipStreamSynchronize(s));
  check_device_error();
  if (stats) std::memset(stats, 0, sizeof(*stats));
  double by = 0.0;
  for (int b = 0; b < B; b++) {
    const LookupRow& r = st[(size_t)b];
    n_out[b] = r.n_out;
    by += 4.0 * r.len;
    if (stats) {
      stats->steps = std::max(stats->steps, r.steps);
      stats->drafted[b] = r.drafted;
      stats->accepted[b] = r.accepted;
    }
  }
  lk_last_ = a;
  lk_last_.mode = LOOKUP_TIME;
  lk_last_.tok = lk_ttok_;
  lk_last_.trows = lk_ttrows_;
  lk_last_.blocks = lk_tblocks_;
  lk_last_bytes_ = by;
  if (sampled) {
    lk_samp_.T = T;
    lk_samp_.W = W;
    lk_samp_.gather = gather;
    lk_samp_.any_greedy = any_greedy;
  }
}

// time_kernel(14): the selection of the most recent sampled lookup step -- the live-row list, the logits of the listed
// rows, soft-cap, select, finalize -- over that step's token rows (lk_snap_), into a list and ids of its own; the
// final-norm rows are whatever sc_x16_ holds now
void Session::time_lookup_select(int reps, double* us, double* bytes) {
  *us = *bytes = 0.0;
  const int T = lk_samp_.T;
  if (T == 0 || reps <= 0) return;
  hipStream_t s = stream_;
  *us = time_reps(s, reps, [&] {
    lookup_select(lk_snap_, T, lk_samp_.W, lk_samp_.gather, lk_samp_.any_greedy, lk_tlive_, lk_tids_, nullptr, s);
  }) * 1000.0 / reps;
  int32_t n_live = 0;  // (as the timed launches left it)
  LLMI_HIP(hipMemcpyAsync(&n_live, lk_tlive_ + LLMI_BATCH_TOKENS_MAX, 4, hipMemcpyDeviceToHost, s));
  LLMI_HIP(hipStreamSynchronize(s));
  // table reads: one per block of RB listed rows; without the list one per block of every chunk's token rows
  const int rb = logits_rows_rb(hp_.n_embd);
  int reads = 0;
  if (lk_samp_.gather) {
    reads = (n_live + rb - 1) / rb;
  } else {
    for (int c0 = 0; c0 < T; c0 += LLMI_SEQ_MAX) {
      const int n = std::min(LLMI_SEQ_MAX, T - c0);
      reads += rb ? (n + rb - 1) / rb : n;
    }
  }
  *bytes = (double)reads * (double)logits_w_.bytes + (double)n_live * vocab_ * 4.0;
}

// time_kernel(13): lookup_step_kernel's draft search over the most recent lookup call's rows, into tables of its own
void Session::time_lookup_step(int reps, double* us, double* bytes) {
  *us = *bytes = 0.0;
  if (lk_last_.B == 0 || reps <= 0) return;
  hipStream_t s = stream_;
  *us = time_reps(s, reps, [&] { launch_lookup_step(lk_last_, s); }) * 1000.0 / reps;
  *bytes = lk_last_bytes_;
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
  *us = time_reps(s, reps, [&] {
    batch_logits(B, s);
    launch_sample_select_rows(bt_logits_, vocab_, B, bt_samplers_, bt_trows_, bt_surv_, s);
    launch_sample_finalize_rows(bt_surv_, vocab_, B, bt_samplers_, sc_amax_, bt_trows_, bt_tok_, st, bt_ring_, false, s);
  }) * 1000.0 / reps;
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
  *us = time_reps(s, reps, [&] {
    for (int l = 0; l < NL; l++) {  // the launches write only the step's scratch rows (the o projection's x)
      PrefillAttn at = bt_last_attn_[(size_t)l];
      at.rows = bt_trows_;
      at.pos0 = max_pos;
      launch_prefill_attn(at, B, s);
    }
  }) * 1000.0 / reps / NL;
  *bytes = by / NL;
}

// time_kernel(12): the attention launches of the most recent batch_extend step as it ran them -- the span form and
// its merge, or (LLMI_BATCH_SPAN_ROWS=1 at that call) the per-token form over the same token rows
void Session::time_extend_attn(int reps, double* us, double* bytes) {
  *us = *bytes = 0.0;
  const int NL = hp_.n_layer, T = (int)bx_last_rows_.size();
  if (T == 0 || (int)bx_last_attn_.size() != NL || reps <= 0) return;
  hipStream_t s = stream_;
  // (the step's own tables: nothing else writes them)
  h2d(bx_rows_, bx_last_rows_.data(), (size_t)T * sizeof(SeqRow));
  h2d(bx_blocks_, bx_last_blocks_.data(), bx_last_blocks_.size() * sizeof(AttnBlock));
  double by = 0.0;  // K and V rows 0 .. last position of every query block, once per block
  for (int l = 0; l < NL; l++)
    for (const auto& b : bx_last_blocks_) by += (double)(b.pos + b.n) * 2.0 * nkv_ * L_[(size_t)l].hd * 2.0;
  *us = time_reps(s, reps, [&] {
    for (int l = 0; l < NL; l++) launch_batch_attn(bx_last_attn_[(size_t)l], T, s);  // (writes the o projection's x only)
  }) * 1000.0 / reps / NL;
  *bytes = by / NL;
}

}  // namespace llmi
