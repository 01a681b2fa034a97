// kernels.h -- host-side launchers for the gfx950 decode kernels.
// All launchers are asynchronous on `s` and capture-safe (no allocation, no
// synchronization), so the session can record them into one hipGraph.
#pragma once

#include "common.h"

namespace llmi {

// ---- device weight layouts (repacked once at upload) -------
// Q4_0 : qs [rows][nb][16] B (16-B aligned), d [rows][nb] f16
// Q8_0 : qs [rows][nb][32] B (16-B aligned), d [rows][nb] f16
// F16  : [rows][cols] f16 (cols % 8 == 0 for the vector kernels)
// Q4_K / Q6_K / Q5_0 / BF16 : the GGUF block bytes, unchanged
// Q4_K / Q6_K, kq (fused fast path, to_kq_layout): 32-element sub-blocks u
//   qs  [rows][nsub][16] B  nibbles in the Q4_0 order (byte i: elements i, 16 + i)
//   d   [rows][nsub] u16    Q4_K: 6-bit scale | 6-bit min << 8; Q6_K: int8 scales of elements 0-15 | 16-31 << 8
//   kdd [rows][nsb] u32     Q4_K: f16 d | f16 dmin << 16; Q6_K: f16 d
//   kqh [rows][nsub] 8 B    Q6_K: the high 2 bits, word w of elements 4w + b (b = byte) at bits 8b + 2w
//                           (first dword: elements 0-15, second: 16-31)
struct DevWeight {
  uint32_t type = 0;
  int rows = 0, cols = 0;
  void* qs = nullptr;      // quants (or raw blocks / f16 / bf16 data)
  uint16_t* d = nullptr;   // per-block scales (Q4_0/Q8_0 only; kq: per sub-block scale words)
  size_t bytes = 0;        // algorithmic bytes (GGUF size of the tensor)
  int slab = 0;            // Q4_0 only: 1 = slab-major blocks (to_slab_layout; layer kernels only)
  int kq = 0;              // Q4_K / Q6_K: 1 = the kq layout above (layer kernels only)
  uint32_t* kdd = nullptr;
  uint2* kqh = nullptr;
};

// Activation prepared for a weight type (device scratch):
//   Q8_0 : Q8Act {qs[nb][32], d[nb], nsum8[nb]}
//   Q8_K : raw 292-B blocks (ops.h:98-102)
//   F16  : x rounded to f16 (ops.cpp:542-551)
struct ActBuf {
  Q8Act q8{};
  uint8_t* q8k = nullptr;
  uint16_t* x16 = nullptr;
  const float* xf = nullptr;  // raw f32 x (Q5_0 / BF16 consume it directly)
};

enum GemvMode { GEMV_EXACT = 0, GEMV_FAST = 1 };

// Kernel timing hook (bench): when set, the next instrumented launch on this
// thread records start/stop through hipExtLaunchKernel -- the events are
// signalled by the kernel's own dispatch, so the elapsed time is the kernel's
// duration as rocprofv3 reports it (no launch gap) -- and clears the hook.
struct KernelTiming {
  hipEvent_t start = nullptr, stop = nullptr;
};
KernelTiming& kernel_timing();

// quantizers (bit-exact with ops.cpp:116-178)
void launch_quantize_q8_0(const float* x, int n, Q8Act out, hipStream_t s);
void launch_quantize_q8_k(const float* x, int n, uint8_t* out, hipStream_t s);
void launch_round_f16(const float* x, int n, uint16_t* out, hipStream_t s);

// o[rows] = W x.  For F16 with amax_key != nullptr the kernel also folds a
// first-index argmax over the outputs into *amax_key (must be pre-zeroed).
void launch_gemv(const DevWeight& w, const ActBuf& x, float* o, GemvMode mode, hipStream_t s,
                 unsigned long long* amax_key = nullptr);

// The fast F16 GEMV for R activation rows at once: x16 [R][xstride] f16 rows (xstride % 8
// == 0), out [R][w.rows] f32; out[r] carries the bits launch_gemv(GEMV_FAST) writes for row r alone.  The widths of
// launch_gemv's pipelined row kernel only (cols % 128 == 0, cols <= 6144).  The table is read once per block of
// logits_rows_rb(cols) activation rows, which wait in LDS: 8 rows up to 3840 columns (60 KB), 4 above (at most
// 48 KB); 0: the width is not supported.
constexpr int logits_rows_rb(int cols) {
  return (cols <= 0 || cols % 128 != 0 || cols > 6144) ? 0 : cols <= 3840 ? 8 : 4;
}
void launch_gemv_f16_rows(const DevWeight& w, const uint16_t* x16, int xstride, int R, float* out, hipStream_t s);
// The gathered form: a device list of *n_live activation-row indices, of which this launch takes
// the compact rows base .. base + cap - 1 (idx points at entry `base`): out[i] (i < min(cap, *n_live - base)) carries
// the bits launch_gemv(GEMV_FAST) writes for activation row idx[i] alone; the other rows of out are not written.  The
// grid covers cap rows; a work-group whose block of logits_rows_rb(cols) rows lies at or past the count returns before
// it loads anything from the table, so the table reads follow the count the host never sees.
void launch_gemv_f16_rows_gather(const DevWeight& w, const uint16_t* x16, int xstride, const int32_t* idx,
                                 const int32_t* n_live, int base, int cap, float* out, hipStream_t s);

// elementwise / norms
// o = rms_norm(x) [* w if w]  per row of n, n_rows rows; exact = serial FMA sum
void launch_rms_norm(const float* x, const float* w, float* o, int n, int n_rows, double eps, bool exact,
                     hipStream_t s);
void launch_softmax(float* x, int n, hipStream_t s);
// NEOX rope on t[n_rows][head_dim] (row r uses table row r / rows_per_pos):
// cs = [n_pos][n_rot/2][2] (cos, sin) precomputed on the host with glibc
void launch_rope(float* t, int n_rows, int head_dim, int n_rot, const float* cs, int rows_per_pos, hipStream_t s);
void launch_scale(float* t, int n, float sc, hipStream_t s);
void launch_vec_scale_f16(uint16_t* y, int n, float v, hipStream_t s);
void launch_vec_mad_f16(uint16_t* y, const uint16_t* x, int n, float v, hipStream_t s);
void launch_gelu_mul(const float* g, const float* u, float* o, int n, hipStream_t s);
void launch_dequantize_rows(uint32_t type, const uint8_t* blocks, size_t row_bytes, const int32_t* row_ids,
                            int n_ids, int n_cols, float scale, float* o, hipStream_t s);

// ---- scoring (k_score.hip) ----
// Fused scorer: per token t of x16 [T][xstride] (f16 rows of E) against the table w16 [V][E] (f16, row-major), from
// the logits l_t[v] = x_t . w_v (f32 MFMA accumulator over all of E in k order; cap tanhf(l / cap) when
// softcap > 0): lse[t] = log sum_v exp(l_t[v]), logprob[t] = l_t[targets[t]] - lse[t] (0.0f for target -1 or
// targets == null), argmax[t] = the first maximal index.  The T x V logits are never written: one launch leaves
// per (token, 128-row vocabulary tile) {max, sum exp(l - max)}, the argmax key and the target's logit, a second
// merges each token's partials in f64 in a fixed order.  E % 16 == 0; every pointer is device memory.
struct ScoreArgs {
  const uint16_t* x16 = nullptr;
  int xstride = 0;
  const uint16_t* w16 = nullptr;
  int T = 0, V = 0, E = 0;
  float softcap = 0.0f;
  const int32_t* targets = nullptr;  // [T] or null
  // scratch (score_plan.h: ms_bytes, key_bytes, tl_bytes)
  float2* ms = nullptr;
  unsigned long long* key = nullptr;
  float* tl = nullptr;
  // outputs [T]
  float* logprob = nullptr;
  float* lse = nullptr;
  int32_t* argmax = nullptr;
};
void launch_score_rows(const ScoreArgs& a, hipStream_t s);
// Row path: the same three results from one f32 logits row (f64 accumulation, the same tie rule) into
// logprob[0] / lse[0] / argmax[0]; target -1: none.
void launch_score_reduce_row(const float* logits, int V, int target, float* logprob, float* lse, int32_t* argmax,
                             hipStream_t s);

// ---- lookup decoding (k_lookup.hip) ----
struct SeqRow;     // (session_kernels.h)
struct AttnBlock;
constexpr int LOOKUP_NGRAM_MAX = 8, LOOKUP_DRAFT_MAX = 31;
// A row's state, device-resident across the steps of one call.  hist[len - 1] is the token the next step runs at
// `pos` of KV slot `slot`; cap >= the initial len + max_new.
struct LookupRow {
  int32_t* hist;
  int32_t len, cap, slot, pos;
  int32_t remaining, n_out, done;  // of max_new; ids emitted so far; 1: a stop id was emitted or remaining == 0
  int32_t nd;                      // draft tokens of the step being run (token rows 1..nd of the row's span)
  int32_t steps, drafted, accepted;  // steps the row was live in; sum of nd; ids emitted past each step's first
  int32_t match_end, match_len;      // the last draft's match (e, ml(e)); -1 / 0: none
  int32_t pad;
};
enum { LOOKUP_STEP = 0, LOOKUP_DRAFT = 1, LOOKUP_TIME = 2 };
// One work-group per row b, its token rows b (D + 1) .. of the step's tables.
// LOOKUP_STEP: accept the step just scored (argmax: the scorer's ids of all B (D + 1) rows; emit a[0], then a[j] while
// d[j-1] == a[j-1]; cut after a stop id; never past `remaining`), append to hist and out[b][n_out..], then draft and
// write the next step's tables.  LOOKUP_DRAFT: the draft and the tables only (the first step; the op-level call).
// LOOKUP_TIME: the draft search of every row whatever its budget, tables written, no state changed (time_kernel(13)).
// Tables: tok [B (D + 1)] (row 0 the current token, 1..nd the draft, the rest a valid id), trows {slot, pos + j} for
// j <= nd else pos -1, blocks[b] = {b (D + 1), 1 + nd, slot, pos}; a finished row: every pos -1.  done: [B] flags.
struct LookupArgs {
  LookupRow* rows = nullptr;
  int B = 0, D = 0, ngram_max = 0, ngram_min = 0, mode = LOOKUP_STEP;
  const int32_t* argmax = nullptr;
  int32_t* tok = nullptr;
  SeqRow* trows = nullptr;
  AttnBlock* blocks = nullptr;
  int32_t* out = nullptr;  // [B][max_new]
  int max_new = 0;
  int32_t* done = nullptr;
  int32_t stop[4] = {0, 0, 0, 0};
  int n_stop = 0;
};
void launch_lookup_step(const LookupArgs& a, hipStream_t s);

// ---- lookup decoding for sampled rows (k_lookup.hip, k_sample.hip) ----
// The step's live-row list, one work-group over the T <= 512 token rows the lookup launch has written: idx[0..n) = the
// token rows t, ascending, with trows[t].pos >= 0 whose row t / W (W = draft_len + 1) samples (sp[t / W].temperature
// > 0), *n_live = n.  all: every token row is listed (LLMI_LOOKUP_NO_GATHER: the sampler's launches skip the ended
// and the greedy ones themselves).  A greedy row's live token rows take ids[t] = argmax[t] (argmax null: the call has
// no greedy row).  snap non-null: trows[0..T) is copied there when some token row is live and sampled -- the last step
// that sampled, for time_kernel(14).
struct SamplerDev;  // (sample.h)
struct LiveRowsArgs {
  const SeqRow* trows = nullptr;
  const SamplerDev* sp = nullptr;
  int T = 0, W = 1, all = 0;
  int32_t* idx = nullptr;     // [T]
  int32_t* n_live = nullptr;  // [1]
  const int32_t* argmax = nullptr;
  int32_t* ids = nullptr;     // [T]
  SeqRow* snap = nullptr;     // [T]
};
void launch_lookup_live_rows(const LiveRowsArgs& a, hipStream_t s);
// x[i][0..V) = cap tanhf(x[i] / cap) (launch_softcap's expression) for the compact rows i < min(rows, *n_live - base)
void launch_softcap_live_rows(float* x, int V, int rows, const int32_t* n_live, int base, float cap, hipStream_t s);

}  // namespace llmi
