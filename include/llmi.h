/*
 * llmi.h -- C ABI of the MI355X-native decode path for corywalker/llm_inference.
 *
 * Library: llm_inference_amd/libllmi.so (HIP, gfx950).  Plain C types only:
 * pointers, sizes, status codes.  No exceptions cross this boundary; every
 * entry point returns llmi_status (0 = OK) and llmi_last_error() holds the
 * reference's own message text for the failure (thread-local).
 *
 * Two layers:
 *  (1) ops.h drop-in (host buffers, synchronous: results are complete on
 *      return, like the reference's fork/join GEMVs, ops.cpp:450).  One entry
 *      point per reference function; the reference line each one replaces is
 *      cited.  The C++ functions with the reference's exact ops.h signatures
 *      are integration/ops_mi355x.cpp, built in place of ops.cpp
 *      (INTEGRATION.md shows the Bazel wiring).
 *  (2) device session: the whole Gemma-3 forward of Model::forward
 *      (model.cpp:706-1049) resident on one MI355X, weights uploaded once from
 *      the caller's GGUF bytes (the GGUF loader/format is unchanged), each
 *      decode token replayed as one hipGraph.
 *
 * Numerics: LLMI_EXACT selects kernels that reproduce the reference's AVX2
 * operation order bit-for-bit (GEMVs, quantizers, norms, rope, f16 vector ops);
 * the default (fast) kernels reassociate reductions across a wavefront and
 * are checked to the tolerances stated in DESIGN.md.
 */
#ifndef LLMI_H
#define LLMI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  LLMI_OK = 0,
  LLMI_E_SIZE = 1,   /* input size mismatch: ops.cpp:196-198 ("input vector size mismatch") */
  LLMI_E_TYPE = 2,   /* unsupported tensor type: ops.cpp:953-954 */
  LLMI_E_ARG = 3,    /* invalid argument (e.g. eps <= 0: ops.cpp:29-32, which exit(1)s) */
  LLMI_E_HIP = 4,    /* HIP runtime failure */
  LLMI_E_GGUF = 5,   /* malformed GGUF / missing metadata: gguf.cpp:276-277, model.cpp:64-66 */
  LLMI_E_NODEV = 6,  /* no usable gfx950 device */
  LLMI_E_RANGE = 7   /* context overflow / token id out of range */
} llmi_status;

/* flags */
#define LLMI_EXACT 1u      /* bit-exact AVX2-order kernels */
#define LLMI_NO_GRAPH 2u   /* session: launch kernels eagerly instead of one hipGraph per token */
#define LLMI_TP_PEER 4u    /* session: tensor-parallel rank of tp_size processes (one per GPU) exchanging by
                              one-shot peer push (llmi_session_peer_connect) instead of RCCL */
#define LLMI_EXACT_KQ 8u   /* session, with LLMI_EXACT only: the exact-order engine also takes K-quant (Q4_K / Q6_K)
                              layers; opt-in, also set by LLMI_EXACT_KQ=1 in the environment at session creation */

const char* llmi_last_error(void);
int llmi_version(void);

/* ---------------------------------------------------------------------------
 * (1) ops.h drop-in -- host pointers, synchronous
 * ------------------------------------------------------------------------- */
/* init_ops(int n_threads), ops.cpp:21-24: selects the HIP device instead of a
 * thread count; must precede the other calls (implicitly device 0 otherwise). */
int llmi_init_ops(int device);

/* mat_vec_mul, ops.cpp:933-956 (+ mat_vec_mul_fp16, ops.cpp:455-612, for
 * type 1 = F16): o[n_rows] = W[n_rows x n_cols] * x.  W is in GGUF block
 * layout (row-major blocks, ops.h:11-31/89-102), types Q4_0 2, Q5_0 6, Q8_0 8,
 * Q4_K 12, Q6_K 14, BF16 30, F16 1.  x_len must equal n_cols. */
int llmi_mat_vec_mul(uint32_t type, const void* w, size_t n_rows, size_t n_cols, const float* x, size_t x_len,
                     float* o, uint32_t flags);

/* Weight handles: upload (and repack) a GGUF weight once, then multiply many
 * times -- what the compat layer does per TensorInfo (keyed by its mmap
 * pointer) so a model.cpp-driven decode moves only x and o per call. */
typedef struct llmi_weight llmi_weight;
int llmi_weight_create(uint32_t type, const void* w, size_t n_rows, size_t n_cols, llmi_weight** out);
int llmi_weight_mat_vec_mul(const llmi_weight* w, const float* x, size_t x_len, float* o, uint32_t flags);
/* device-pointer form on a caller stream (hipStream_t passed as void*) */
int llmi_weight_mat_vec_mul_dev(const llmi_weight* w, const float* x_dev, float* o_dev, uint32_t flags,
                                void* stream);
void llmi_weight_destroy(llmi_weight* w);

int llmi_quantize_row_q8_0(const float* x, size_t n, void* y);  /* ops.cpp:116-139, 34-B BlockQ8_0 out */
int llmi_quantize_row_q8_k(const float* x, size_t n, void* y);  /* ops.cpp:142-178, 292-B block_q8_K out */
/* dequantize_{q4_k,q6_k,q8_0,q5_0}_row, ops.cpp:958-1082 (+F16/F32) */
int llmi_dequantize_row(uint32_t type, const void* blocks, size_t n_cols, float* o);
int llmi_rms_norm(float* o, const float* x, size_t n, double eps, uint32_t flags); /* ops.cpp:28-43 */
int llmi_softmax(float* x, size_t n);                                              /* ops.cpp:45-62 */
/* rope, ops.cpp:67-95; t is [n_tokens][n_heads][head_dim] contiguous, in place */
int llmi_rope(float* t, size_t n_tokens, size_t n_heads, size_t head_dim, int n_rot, float freq_base,
              float freq_scale, int pos);
int llmi_scale(float* t, size_t n, float s);                                      /* ops.cpp:97-105 */
int llmi_vec_scale_f16(uint16_t* y, size_t n, float v);                           /* ops.cpp:1084-1089 */
int llmi_vec_mad_f16(uint16_t* y, const uint16_t* x, size_t n, float v);          /* ops.cpp:1091-1099 */

/* Decode attention of Model::run_attn (model.cpp:478-550) for one query
 * token against an f16 KV history: q [n_head][head_dim] f32 (already
 * normed/roped/scaled), k/v [n_head_kv][n_keys][head_dim] f16 bits, out
 * [n_head][head_dim] f32.  LLMI_EXACT = the reference's sequential algorithm
 * (double scores, f16 V accumulator); default = split-K fp32. */
int llmi_attention(const float* q, const uint16_t* k, const uint16_t* v, int n_head, int n_head_kv, int n_keys,
                   int head_dim, float* out, uint32_t flags);
/* GELU(tanh)(gate) * up, model.cpp:892-899 */
int llmi_gelu_mul(const float* gate, const float* up, size_t n, float* out);

/* ---------------------------------------------------------------------------
 * (2) device session (Gemma-3 GGUF)
 * ------------------------------------------------------------------------- */
typedef struct llmi_session llmi_session;
typedef struct llmi_tp_group llmi_tp_group;

typedef struct {
  int device;          /* HIP device ordinal */
  uint32_t flags;      /* LLMI_EXACT | LLMI_NO_GRAPH | LLMI_TP_PEER | LLMI_EXACT_KQ */
  int max_ctx;         /* KV-cache capacity in positions (default 4096) */
  int attn_split;      /* fast attention key-range splits: 0 = default (32, the only value) */
  /* Row-sharded tensor parallelism (north star: "weights shard row-wise across
   * the 8 GPUs of one node with an RCCL all-gather"; the reference itself is
   * single-device).  Active when tp_id or tp_group is non-NULL: this session
   * is rank tp_rank of tp_size and holds 1/tp_size of every projection's
   * output rows (q/k/v heads, o/down rows, gate/up hidden units, vocabulary
   * rows); after each projection the slices are all-gathered.  Fast kernels
   * only (not with LLMI_EXACT).  Every rank must make the same session calls. */
  int tp_rank, tp_size;
  const void* tp_id;        /* LLMI_TP_ID_BYTES from llmi_tp_unique_id on one rank: RCCL over xGMI */
  llmi_tp_group* tp_group;  /* or: ranks on one device in one process (tests; one host thread per rank) */
  /* or (both NULL, flags LLMI_TP_PEER): the one-shot push exchange between processes, below */
} llmi_session_opts;

#define LLMI_TP_ID_BYTES 128
/* new RCCL communicator id (ncclGetUniqueId); distribute it to every rank */
int llmi_tp_unique_id(void* out);
/* single-device group of `size` ranks: the push exchange split around a host barrier (LLMI_TP_EXCHANGE=copy:
 * device-to-device slice copies) */
int llmi_tp_group_create(int size, llmi_tp_group** out);
void llmi_tp_group_destroy(llmi_tp_group* g);

/* One-shot push exchange (replaces ncclAllGather, the exchange of ops.cpp:439-450's row split
 * across devices): every rank writes its slice of each all-gather as data-tagged 8-byte granules {word, tag}
 * straight into every peer's mailbox through xGMI peer mappings, then polls its own mailbox -- one kernel per
 * exchange, captured in the token's hipGraph.  A LLMI_TP_PEER session: after creation, every rank publishes
 * its mailbox handle, and before its first forward connects to all of them (rank order, tp_size x
 * LLMI_PEER_HANDLE_BYTES); the handles travel by any host channel (bench.py: torch.distributed). */
#define LLMI_PEER_HANDLE_BYTES 64
int llmi_session_peer_handle(const llmi_session* s, void* out);
int llmi_session_peer_connect(llmi_session* s, const void* handles);

/* Parses the GGUF (format of gguf.cpp:274-304, hparams of model.cpp:58-167)
 * and uploads every weight.  The bytes are only read during the call. */
int llmi_session_create(const void* gguf, size_t size, const llmi_session_opts* opts, llmi_session** out);
void llmi_session_destroy(llmi_session* s);

/* Model::forward(tokens, pos) (model.cpp:706): runs n_tokens tokens at
 * positions pos..pos+n_tokens-1 and returns the LAST token's logits
 * (vocab floats, may be NULL) and its greedy argmax (may be NULL).
 * Fast sessions on one device run n_tokens > 1 as a batched prefill (int8
 * MFMA GEMMs over the tokens, causal attention over the cache) instead of
 * the reference's token loop (model.cpp:752-756); LLMI_NO_PREFILL=1 in the
 * environment forces the token loop. */
int llmi_session_forward(llmi_session* s, const int32_t* tokens, int n_tokens, int pos, float* logits,
                         int32_t* argmax);

/* Teacher-forced scoring: runs tokens[0..n) at positions pos..pos+n-1 exactly as llmi_session_forward does
 * (same KV rows, same session state afterwards, the last token's logits / argmax left where forward leaves
 * them), and for EVERY position i reports, from that position's logits l_i[0..V) (after the final soft-cap):
 *   lse[i]     = log sum_v exp(l_i[v])                      (natural log)
 *   logprob[i] = l_i[targets[i]] - lse[i]                    (0.0f exactly where the position has no target)
 *   argmax[i]  = first maximal index (argmax_key's rule: larger value, then smaller id)
 * targets == NULL: targets[i] = tokens[i+1], the last position has none.  Otherwise n ids, -1 = no target.
 * Any of logprob / lse / argmax may be NULL.  One device only (tensor-parallel session: LLMI_E_ARG).
 * Fast sessions with a batched prefill and an F16 output table run the last layer for every token of each
 * prefill chunk and hand the chunk's f16 final-norm rows to the fused MFMA scorer (k_score.hip: the T x V logits
 * are never written); every other session runs the token loop with full logits and reduces each row in f64
 * (llmi_session_info.score_path). */
int llmi_session_score(llmi_session* s, const int32_t* tokens, int n_tokens, int pos, const int32_t* targets,
                       float* logprob, float* lse, int32_t* argmax);

/* Several sequences per step.  Fast sessions on one device with a batched prefill, the fused
 * scorer (F16 output table), Gemma-3 layers of Q4_0 / Q8_0 weights (no K-quant layers) and head_dim 128 or 256 only;
 * every other session gets LLMI_E_ARG from seq_reserve, the message naming the reason.
 * Row contract: if K/V rows 0..p-1 of a slot were written by the batched prefill or by
 * batch steps for tokens x[0..p), a batch step running x[p] at position p of that slot gives, bit for bit, the last
 * position of llmi_session_score / llmi_session_forward of x[0..p] on a fresh session -- whatever B, the other rows,
 * the slot and the row order.  (Rows written by the one-token decode graph -- forward with one token, generate --
 * carry that path's roundings: continuing from them works, nothing bit-exact is promised.) */
#define LLMI_SEQ_MAX 64
/* KV slots 0..n_seq-1.  Slot 0 IS the session's own cache (forward / generate / score keep using it, their graphs
 * untouched); slots 1.. are allocated here, same [n_head_kv][max_ctx][head_dim] f16 layout per layer.  May be
 * called again with a larger n_seq (existing slots keep their rows).  1 <= n_seq <= LLMI_SEQ_MAX. */
int llmi_session_seq_reserve(llmi_session* s, int n_seq);
/* K/V rows [0, n_pos) of every layer, slot src -> slot dst (a prompt run by forward() lands in slot 0; this moves
 * or forks it).  Ordered on the session's stream. */
int llmi_session_seq_copy(llmi_session* s, int dst, int src, int n_pos);
/* One step for B rows: row b runs token tokens[b] at position pos[b] of slot slots[b] (appends its K/V there,
 * attends keys 0..pos[b] of that slot).  argmax[b] / lse[b] (may be NULL) come from the fused scorer; logits
 * ([B][vocab], may be NULL) from the multi-row F16 logits GEMV (one table read per block of rows, section 13; for
 * host-side sampling).  Slots must be distinct within a call.  1 <= B <= n_seq. */
int llmi_session_batch_forward(llmi_session* s, const int32_t* tokens, const int32_t* slots, const int32_t* pos,
                               int B, float* logits, int32_t* argmax, float* lse);
/* Greedy loop on the device, no host round trip between steps: step i feeds row b's arg-max back as its next token
 * at pos[b] + i + 1.  out[i * B + b] = row b's id after step i.  stop (n_stop <= 4 ids, may be NULL): once row b
 * emits one, that entry is the stop id, every later entry of row b is -1, and row b appends nothing at or past
 * the position the stop id would have taken (main.cpp:196's break, per row).  pos[b] + n_steps <= max_ctx.
 * (Prompts and several tokens of one sequence per step: llmi_session_batch_extend below.) */
int llmi_session_batch_generate(llmi_session* s, const int32_t* first, const int32_t* slots, const int32_t* pos,
                                int B, int n_steps, const int32_t* stop, int n_stop, int32_t* out);

/* Ragged batch steps: one step over a list of spans.  Span i runs n_tokens consecutive tokens
 * of slot `slot` at positions pos .. pos + n_tokens - 1 (appends their K/V there, each token attending keys 0 .. its own
 * position of that slot); `tokens` is the spans' tokens concatenated.  A prompt chunk, one decode row (n_tokens = 1:
 * exactly llmi_session_batch_forward's row) and n draft tokens to verify are all spans, and share the step's one pass
 * over the weights.  Outputs are compacted in span order: one entry for a LLMI_SPAN_LAST span (its last token), n_tokens
 * for a LLMI_SPAN_ALL span, none for a LLMI_SPAN_NONE span; argmax / lse (may be NULL) from the fused scorer run over
 * the output rows only, logits ([n_out][vocab], may be NULL) from the multi-row F16 logits GEMV.  A call whose spans
 * are all LLMI_SPAN_NONE runs no final norm, no scorer and no GEMV.
 * Row contract (extends the one above, no tolerance): if K/V rows 0..pos-1 of the slot were written by the batched
 * prefill, by batch steps or by earlier spans for x[0..pos), then for every token row at position p of a span running
 * x[pos..pos+n), an output row's argmax / lse are the last entries of llmi_session_score(x[0..p]) and its logits those
 * of llmi_session_forward(x[0..p], 0) on a fresh single-sequence session, bit for bit -- whatever the other spans, the
 * split of the sequence into spans and calls, the slots and the span order.  The K/V rows pos..pos+n-1 left in the
 * slot are the bits llmi_session_forward(x[0..pos+n), 0) leaves in slot 0; rows at and past pos + n are not touched, and
 * a later span that starts below a slot's previous end simply overwrites (how rejected draft tokens are dropped).
 * (The single-sequence session's own bits are meant as it computes them for the same token list: an output row at
 * position 0 is its one-token decode step -- scored like llmi_session_score scores position 0 of a one-token or of a
 * longer prompt -- and where the batched prefill picks its GEMM by the launch's token rows, the step's row count and
 * the reference prompt's chunk must fall on the same side of that switch: DESIGN.md section 14.1.)
 * Checks: sessions as llmi_session_seq_reserve; 1 <= n_spans <= n_seq, a slot at most once per call, n_tokens >= 1,
 * the sum of n_tokens <= LLMI_BATCH_TOKENS_MAX, pos >= 0, pos + n_tokens <= max_ctx. */
#define LLMI_BATCH_TOKENS_MAX 512          /* token rows per call: the prefill's default chunk */
enum { LLMI_SPAN_LAST = 0, LLMI_SPAN_ALL = 1, LLMI_SPAN_NONE = 2 };
typedef struct { int32_t slot, pos, n_tokens, out; } llmi_span;   /* 16 bytes */
int llmi_session_batch_extend(llmi_session* s, const int32_t* tokens, const llmi_span* spans, int n_spans,
                              float* logits, int32_t* argmax, float* lse);

/* op level, host pointers, synchronous: the fused scorer alone.  x16: [T][E] f16 bits, w16: [V][E] f16 bits
 * (row-major), softcap <= 0: none.  E % 16 == 0, else LLMI_E_SIZE. */
int llmi_score_rows(const uint16_t* x16, const uint16_t* w16, int T, int V, int E, float softcap,
                    const int32_t* targets, float* logprob, float* lse, int32_t* argmax);

/* Layer-by-layer triage: llmi_session_forward's token
 * loop, one token at a time with eager launches, appending the
 * intermediates the reference prints under --verbose (model.cpp VERBOSE
 * print_tensor calls: inp_scaled, attn_norm-L, Qcur-L, Kcur-L, Vcur-L,
 * kqv_out-L, "attention results (node_30 for MUL_MAT)-L", sa_out-L,
 * ffn_norm-L, ffn_geglu-L, ffn_out-L, l_out-L, result_norm, result_output)
 * to the text file `path` in tensor.h's print_tensor format, so the two
 * dumps pair by name and occurrence (scripts/compare_dumps.py, the
 * compare_tensors.py counterpart).  Slow; the results equal forward's. */
int llmi_session_dump(llmi_session* s, const int32_t* tokens, int n_tokens, int pos, const char* path);

/* Op-level parity taps (test hook; the per-op counterpart of
 * llmi_session_dump).  Runs the SAME kernels the decode graph (or, for
 * n_tokens > 1 on a batched-prefill session, the prefill) launches, eagerly,
 * and after each launch copies the buffers it produced to the host and calls
 * fn(user, name, layer, data, bytes) -- e.g. "qkv_g" (the attention block's
 * q|k|v rows as {value, tag} granules), "attn", "xo_g", "o", "kc"/"vc" (the
 * layer's KV cache), "ffn_resid", "ffn_norm", "hid", "down", "result_norm",
 * "logits"/"token"; the prefill taps its GEMM inputs ("pf_x_<proj>", Q8_0
 * blocks) and outputs ("pf_<proj>").  flags bit 0: the decode-loop step
 * (screened token selection) instead of forward's full logits.  flags bit 1
 * (value 2): scoring mode -- llmi_session_score's launches (targets = the next
 * tokens), tapping per chunk "sc_x16" (the [T][E] f16 rows handed to the
 * scorer; they carry no per-token scales, so there is no "sc_xs"), then
 * "sc_lse", "sc_logprob" (f32) and "sc_argmax" (i32).  Slow; the
 * session's state advances exactly as llmi_session_forward's. */
typedef void (*llmi_trace_fn)(void* user, const char* name, int layer, const void* data, size_t bytes);
int llmi_session_trace(llmi_session* s, const int32_t* tokens, int n_tokens, int pos, uint32_t flags,
                       llmi_trace_fn fn, void* user);

/* Greedy decode loop of main.cpp:172-224 kept on the device: token `first`
 * at position `pos`, then n_steps forwards, each feeding its argmax to the
 * next without a host round trip.  out_tokens[i] = argmax after step i (the sampled token when a sampler is
 * set, below). */
int llmi_session_generate(llmi_session* s, int32_t first, int pos, int n_steps, int32_t* out_tokens);

/* Seeded temperature / top-k / top-p sampling in the device decode loop.  With a sampler set,
 * llmi_session_generate / llmi_session_enqueue draw each token from the step's full logits (forward's, after the
 * final soft-cap) instead of taking the argmax: the top_k candidates by (logit descending, id ascending; NaN never),
 * integer weights floor(expf((l_i - l_0) / temperature) 2^32) with glibc's expf, the smallest prefix whose weight
 * reaches top_p of the total, and one 24-bit draw from splitmix64(seed, position).  The result is a pure function
 * of the logits' bits, the parameters, the seed and the position -- the same ids however the steps are chunked.
 * forward / dump / trace ignore the sampler.  One device only: a tensor-parallel session refuses one (LLMI_E_ARG). */
#define LLMI_SAMPLE_MAX_K 256
typedef struct {
  float temperature;  /* > 0; 0: greedy */
  int top_k;          /* 1..LLMI_SAMPLE_MAX_K; 0: LLMI_SAMPLE_MAX_K */
  float top_p;        /* (0, 1]; 1: off */
  uint64_t seed;
} llmi_sampler;
/* NULL or temperature == 0: greedy (the default).  Invalid fields (temperature < 0 or NaN, top_k outside
 * 0..LLMI_SAMPLE_MAX_K, top_p outside (0, 1] or NaN): LLMI_E_ARG, the message names the field.  Takes effect for
 * the steps enqueued after it; no graph is captured again. */
int llmi_session_set_sampler(llmi_session* s, const llmi_sampler* sp);
/* op level, host logits, synchronous: the same kernels (temperature must be > 0).  pos: the position of the token
 * whose logits these are.  cand / cand_q (LLMI_SAMPLE_MAX_K entries, may be NULL) receive the ordered candidates
 * (-1 past the last) and their integer weights, *n_cand = K', *n_nucleus = n (each may be NULL). */
int llmi_sample_logits(const float* logits, size_t n, const llmi_sampler* sp, int pos, int32_t* token,
                       int32_t* cand, uint64_t* cand_q, int* n_cand, int* n_nucleus);

/* Sampling inside the batch loop: llmi_session_batch_generate with a sampler per row
 * (samplers: B entries; NULL: LLMI_E_ARG).  The loop stays on the device: per step the batch step, the rows' full
 * logits (the F16 logits GEMV for several rows at once: one table read per block of rows, each row's logits bit for
 * bit forward's), the final soft-cap and the sampler's two launches for all rows, the second carrying the feedback.
 * Contract: a row that runs x[p] at position p of its slot (under the row contract above on the slot's K/V) emits
 * exactly the rule of llmi_session_set_sampler applied to the logits of llmi_session_forward(x[0..p], 0) on a fresh
 * single-sequence session, with pos = p and its sampler's seed -- whatever B, the other rows and their samplers,
 * the slot, the row order and the chunking of n_steps.  A row whose sampler has temperature == 0 is greedy: its ids
 * are llmi_session_batch_generate's.  Checks, refusals, stop ids and `out` as llmi_session_batch_generate; each
 * sampler is validated as llmi_session_set_sampler validates one (LLMI_E_ARG, the message names the field and the
 * row).  The session's own sampler is neither read nor changed. */
int llmi_session_batch_generate_sampled(llmi_session* s, const int32_t* first, const int32_t* slots, const int32_t* pos,
                                        int B, int n_steps, const int32_t* stop, int n_stop,
                                        const llmi_sampler* samplers, int32_t* out);

/* Lookup decoding: llmi_session_batch_generate's greedy loop with n-gram drafts verified inside
 * the device loop.  Every step runs, per row, the span [current token, up to draft_len draft tokens] -- one ragged
 * step of llmi_session_batch_extend's kind over B (draft_len + 1) token rows -- and one launch accepts the drafts that
 * were the greedy ids, appends the emitted ids to the row's history and drafts the next step; tokens, positions,
 * histories and ids stay on the device.
 * The rule (pure integer).  A row's history h[0..L), ngram_max = N, ngram_min, draft_len = D:
 *   - for every candidate end e in [0, L-2], ml(e) = the largest k <= min(N, e+1, L-1) with h[e-k+1..e] == h[L-k..L-1];
 *   - among the candidates with ml(e) >= ngram_min the largest (ml(e), e) wins: the longer n-gram first, then the most
 *     recent occurrence; none: the draft is empty;
 *   - else c = e+1, P = L-c and d[j] = h[c + (j mod P)] for j = 0..nd-1 (a continuation that reaches the end of the
 *     history wraps periodically, so a repeating tail drafts its full length);
 *   - nd = min(D, remaining-1), `remaining` what is left of the row's max_new: no draft is ever written at or past
 *     pos + max_new.
 * Accept.  The span [cur, d[0..nd)] ran at positions p..p+nd, a[j] = the arg-max of span row j: emit a[0]; for
 * j = 1..nd emit a[j] if d[j-1] == a[j-1], else stop; truncate after the first stop id, inclusive (that ends the row);
 * truncate to `remaining`.  With m ids emitted: they are appended to the history, cur = the last one, pos += m; the row
 * is done when `remaining` reaches 0 or a stop id was emitted.
 * hist: the rows' histories concatenated (hist_len[b] tokens each).  Row b's last history token is the token to run at
 * pos[b] (llmi_session_batch_generate's first[b]); the history need not be the slot's real token list -- it only
 * steers the drafts.  Steps are enqueued in groups of LLMI_LOOKUP_SYNC (environment, default 4, read at the call); after
 * each group the B done flags are read back in one copy, and the call returns when every row is done or max_steps
 * steps have run (0: max_new).  out[b][0..n_out[b]) = row b's ids, -1 past them.
 * Contract (no tolerance): under the row contract above on the slots' K/V, out[b] equals row b's ids of
 * llmi_session_batch_generate(first = the row's last history token, slots, pos, n_steps = max_new, stop) on the same
 * state, up to and including the row's stop id -- whatever the histories, draft_len, the n-gram bounds, B, the other
 * rows, the row order and LLMI_LOOKUP_SYNC -- because every span row carries llmi_session_score's bits.  K/V rows
 * pos[b] .. pos[b]+n_out[b]-1 left in the slot are the bits llmi_session_batch_generate leaves there; rows from
 * pos[b]+n_out[b] up to pos[b]+max_new-1 may hold rejected drafts; rows at and past pos[b]+max_new are never touched.
 * The one condition is the GEMM switch of llmi_session_batch_extend's contract: the step's B (draft_len + 1) token
 * rows must stay on the side of the switch that llmi_session_batch_generate's B rows are on (at most 384 rows on the
 * 4B shapes, 128 on the 27B shapes, any on the 1B: DESIGN.md section 14.1).  f16 overflow: as
 * llmi_session_batch_generate, the loop does not leave the device and does not check.
 * stats (may be NULL) is a pure function of the emitted ids, the histories and the parameters: steps = the steps in
 * which some row was live, drafted[b] = the draft tokens row b ran, accepted[b] = the ids it emitted past the first of
 * each step.
 * Checks (each message names the argument): sessions as llmi_session_seq_reserve; B, the slots and n_stop as
 * llmi_session_batch_generate; 1 <= draft_len <= 31; 1 <= ngram_min <= ngram_max <= 8; max_new >= 1;
 * B (draft_len + 1) <= LLMI_BATCH_TOKENS_MAX; hist_len >= 1; token ids in range; pos >= 1 (LLMI_E_RANGE: a position-0
 * row is a one-token prompt, which runs as a decode step of its own -- llmi_session_batch_generate runs it before its
 * loop, a lookup step would need it inside); pos + max_new <= max_ctx; max_steps >= 0. */
typedef struct { int32_t draft_len, ngram_max, ngram_min, max_new; } llmi_lookup;           /* 16 bytes */
typedef struct { int32_t steps; int32_t drafted[LLMI_SEQ_MAX]; int32_t accepted[LLMI_SEQ_MAX]; } llmi_lookup_stats;
int llmi_session_batch_generate_lookup(llmi_session* s, const int32_t* hist, const int32_t* hist_len,
                                       const int32_t* slots, const int32_t* pos, int B, const llmi_lookup* lk,
                                       int max_steps, const int32_t* stop, int n_stop, int32_t* out, int32_t* n_out,
                                       llmi_lookup_stats* stats);
/* Lookup decoding for sampled rows: everything above holds -- the draft rule, the wrap-around,
 * nd = min(D, remaining-1), the cut after a stop id, the cut at `remaining` -- with one substitution.  For span row j
 * of row b, running at position p + j, a[j] is
 *   - samplers[b].temperature > 0: the sampling rule of llmi_session_set_sampler applied to that token row's full
 *     logits (after the final soft-cap) with samplers[b] and pos = p + j;
 *   - samplers[b].temperature == 0: the fused scorer's arg-max, as in llmi_session_batch_generate_lookup.
 * Emit a[0]; for j >= 1 emit a[j] while d[j-1] == a[j-1].  The draw depends on the position of the token row, not on a
 * step counter or a generator's state, so a[j] is the id llmi_session_batch_generate_sampled emits at p + j whenever the
 * tokens before it are the ones that loop ran: a draft token is right exactly when it equals that id, and accepting is
 * an equality -- no rejection rule, no tolerance, no change of distribution.
 * Contract (no tolerance): under the row contract on the slots' K/V, out[b] equals row b's ids of
 * llmi_session_batch_generate_sampled(first = the row's last history token, slots, pos, n_steps = max_new, stop,
 * samplers) on the same state, up to and including the row's stop id -- whatever the histories, draft_len, the n-gram
 * bounds, B, the other rows and their samplers, the row order, LLMI_LOOKUP_SYNC and LLMI_LOOKUP_NO_GATHER.  The K/V
 * rows, the stale-row bound, the GEMM-switch condition and stats are those of llmi_session_batch_generate_lookup.
 * Only the live token rows of sampled rows need logits: each step the device lists them and a gathered form of the
 * multi-row logits GEMV reads the F16 table once per llmi_logits_rows_rb(n_embd) listed rows, LLMI_SEQ_MAX rows per
 * launch; the host never reads the count.  LLMI_LOOKUP_NO_GATHER=1 (environment, read at the call): the logits of all
 * B (draft_len + 1) token rows, without the list -- the same ids; table widths llmi_logits_rows does not take run this
 * way too, row by row.  The fused scorer runs only when some row is greedy; when every row is, the launches are
 * llmi_session_batch_generate_lookup's.
 * Checks: those of llmi_session_batch_generate_lookup; samplers NULL: LLMI_E_ARG; each sampler as
 * llmi_session_batch_generate_sampled validates it (the message names the field and the row). */
int llmi_session_batch_generate_lookup_sampled(llmi_session* s, const int32_t* hist, const int32_t* hist_len,
                                               const int32_t* slots, const int32_t* pos, int B, const llmi_lookup* lk,
                                               int max_steps, const int32_t* stop, int n_stop,
                                               const llmi_sampler* samplers, int32_t* out, int32_t* n_out,
                                               llmi_lookup_stats* stats);
/* op level, host pointers, synchronous: the gathered multi-row logits GEMV alone (+ the soft-cap over the listed rows).
 * x16 [T][E], w16 [V][E] as llmi_logits_rows; idx: n_idx activation-row indices in [0, T) (any order, repeats allowed),
 * 0 <= n_idx <= cap <= LLMI_SEQ_MAX; logits: [cap][V], read and written: logits[i] (i < n_idx) carries the bits
 * llmi_logits_rows gives row idx[i]; the rows at and past n_idx come back as they went in. */
int llmi_logits_rows_gather(const uint16_t* x16, const uint16_t* w16, int T, int V, int E, float softcap,
                            const int32_t* idx, int n_idx, int cap, float* logits);
/* op level, host pointers, synchronous: the sampler's two launches over R <= LLMI_BATCH_TOKENS_MAX logits rows [R][V],
 * in the lookup loop's chunks of LLMI_SEQ_MAX rows.  Row r draws with samplers[sampler_of_row[r]] (indices in
 * [0, LLMI_SEQ_MAX); each sampler named needs temperature > 0) at position pos[r]: ids[r] = llmi_sample_logits' token
 * for that row; pos[r] < 0 (an ended row): ids[r] = -1. */
int llmi_sample_logits_rows(const float* logits, int R, int V, const llmi_sampler* samplers,
                            const int32_t* sampler_of_row, const int32_t* pos, int32_t* ids);
/* op level, host pointers, synchronous: the draft rule alone, by the same kernel.  draft: draft_len entries;
 * *n_draft = the tokens drafted (0: no match; else draft_len), *match_end = e (-1: none), *match_len = ml(e)
 * (each may be NULL).  L >= 1, 1 <= draft_len <= 31, 1 <= ngram_min <= ngram_max <= 8. */
int llmi_lookup_draft(const int32_t* hist, int L, int ngram_max, int ngram_min, int draft_len, int32_t* draft,
                      int* n_draft, int* match_end, int* match_len);

/* op level, host pointers, synchronous: the multi-row F16 logits GEMV alone.  x16: [T][E] f16 bits, w16: [V][E] f16
 * bits (row-major), logits: [T][V], softcap <= 0: none.  logits[t] carries the bits of the fast F16
 * llmi_mat_vec_mul of w16 with row t.  E % 128 == 0 and E <= 6144, else LLMI_E_SIZE.  llmi_logits_rows_rb: the rows
 * that share one read of the table at width E (0: E is not supported). */
int llmi_logits_rows(const uint16_t* x16, const uint16_t* w16, int T, int V, int E, float softcap, float* logits);
int llmi_logits_rows_rb(int E);

/* Enqueue n_steps decode steps without waiting (bench); llmi_session_sync
 * waits and copies the produced tokens (may be NULL). */
int llmi_session_enqueue(llmi_session* s, int32_t first, int pos, int n_steps);
int llmi_session_sync(llmi_session* s, int32_t* out_tokens, int n);

typedef struct {
  int n_layer, n_embd, n_ff, n_head, n_head_kv, head_dim, vocab, max_ctx;
  size_t weight_bytes;        /* device bytes of all uploaded weights */
  size_t bytes_per_token;     /* algorithmic HBM bytes of one decode token, KV excluded */
  size_t kv_bytes_per_pos;    /* + this many bytes per attended position */
  int kernels_per_token;      /* launches captured in the decode graph */
  int tp_rank, tp_size;       /* weight_bytes / bytes_per_token / kv_bytes_per_pos are this rank's */
  int batched_prefill;        /* 1: llmi_session_forward runs n_tokens > 1 as a batched (MFMA) prefill */
  int screened_logits;        /* 1: llmi_session_enqueue/generate pick each greedy token by int8 screening +
                                 exact f16 rescoring (same ids as the full F16 logits GEMV; forward keeps it) */
  size_t screen_bytes;        /* bytes of the int8 screening table streamed per decode-loop token */
  int prefill_f16_redo;       /* f16 prefills whose final norm row came out non-finite and were recomputed on the
                                 int8 path (never a non-finite result; the per-token scales make it unreachable short
                                 of an attention output past 65504) */
  int layer_engine;           /* always 0: the round-3 layer engine (one launch per decode layer) measured slower
                                 than three launches and was removed in round 6 */
  int ffn_engine;             /* always 0: the FFN engine (gate_up + GELU + down as one launch), likewise */
  int tp_exchange;            /* tensor-parallel exchange: 0 none, 1 RCCL, 2 device copies, 3 one-shot push, 4 one-shot
                                 push fused into the decode launches (the default push mode) */
  long long block_slow_waits; /* attention-block hand-off waits (per wave) that took over 20 us, since creation */
  int exact_engine;           /* 1: LLMI_EXACT runs on the exact-order engine (k_exact.hip: the reference's
                                 arithmetic with streamed GEMVs and fused norms; Gemma-3 layers whose projections are
                                 each Q4_0 or Q8_0, q/k/v of one type and gate/up of one type; tensor-parallel
                                 sessions: Q4_0 only; with LLMI_EXACT_KQ, one device: each of q|k|v, o, gate|up, down
                                 may instead be Q4_K / Q6_K with columns % 256 == 0 -- q, k, v with at most one change
                                 of type along them (Q4_K_M's q|k Q4_K, v Q6_K), gate and up both Q4_K (both Q6_K is
                                 turned away), o and down either; the two families may alternate between launches,
                                 not inside q|k|v or gate|up), 0: the per-op exact kernels (always with
                                 LLMI_EXACT_XL=0) */
  int exact_batched_prefill;  /* 1: an exact session runs a prompt's tokens before the last layer by layer, T at a
                                 time (the reference's chains per (row, token)), then the last as a decode step
                                 (every type combination the engine accepts) */
  int prefill_gemm;           /* the batched prefill's GEMM: 7 f16 MFMA on f16 rows of the dequantized Q8_0 activation
                                 blocks (Q4_0 layers, one device: the default), 5 int8 MFMA on Q8_0 / Q8_K blocks
                                 (LLMI_PREFILL_F16=0, Q8_0 weights, tensor-parallel ranks), 6 f16 for K-quant layers
                                 (LLMI_PREFILL_F16=1); 0 no batched prefill */
  int sampling;               /* 1 while a sampler is set (llmi_session_set_sampler) */
  /* (bytes 132..135, the tail padding after score_path, carry the KV slot count: LLMI_SESSION_INFO_N_SEQ below.
   *  The next field appended goes there as `int n_seq`, not after them.) */
  int score_path;             /* llmi_session_score: 1 the fused MFMA scorer on the batched prefill's rows, 2 the row
                                 path (token loop with full logits + an f64 reduce per row), 0 none (tensor parallel);
                                 LLMI_NO_PREFILL is read at the call, as forward reads it */
} llmi_session_info;
/* The KV slot count (llmi_session_seq_reserve; 1 until reserved) travels in the four bytes after score_path -- the
 * struct's tail padding, so sizeof stays 136 and score_path stays the last declared field.  llmi_session_get_info_sized
 * writes it when info_size covers those bytes; read it with this macro (info: a llmi_session_info*). */
#define LLMI_SESSION_INFO_N_SEQ_OFFSET 132
#define LLMI_SESSION_INFO_N_SEQ(info) (*(const int*)((const char*)(info) + LLMI_SESSION_INFO_N_SEQ_OFFSET))
/* The caller owns the struct, so the library must know how large the caller's is: fills the first
 * min(info_size, sizeof(llmi_session_info)) bytes and never writes past info_size.  Fields are only ever appended. */
int llmi_session_get_info_sized(const llmi_session* s, llmi_session_info* info, size_t info_size);
/* The exported symbol of this name serves binaries built before score_path was appended: it fills the fields up to
 * and including `sampling` (the struct as it was then, 128 bytes) and nothing after them.  Code compiled against
 * this header reaches the sized form through the macro below and gets every field. */
int llmi_session_get_info(const llmi_session* s, llmi_session_info* info);
#define llmi_session_get_info(s, info) llmi_session_get_info_sized((s), (info), sizeof(llmi_session_info))

/* Benchmark hook: time `reps` passes over one decode kernel family, every
 * launch with the real arguments of the decode step and bracketed by HIP
 * events its own dispatch signals, on the session stream:
 *   0 = attention block (qkv + attention + o, one launch per layer; KV
 *       history read at the session's current position),
 *   1 = F16 logits GEMV, 2 = the decode loop's screened token selection,
 *   3 = gate_up (+ norm prologue + GELU), 4 = down (+ Q8_0 prologue),
 *   5 = qkv / o / gate_up / down as standalone layer GEMVs (round-1 family),
 *   6, 7 = the removed layer / FFN engines (always 0 / 0),
 *   8 = the sampler's two launches (candidate selection + finalize) on the session's current logits, with the
 *       session's sampler (temperature 1, top_k 64, top_p 0.95 when none is set); bytes = the logits row;
 *   9 = the fused scorer's launches (partials + merge) over the most recently scored chunk; bytes = the F16 table
 *       plus the chunk's [T][E] f16 rows (0 / 0 when nothing was scored yet or the row path is in use);
 *  10 = the multi-sequence attention launch (+ its merge) of the most recent batch step, one pass over the layers;
 *       bytes = the K and V rows 0..pos[b] of every row that was live in that step, per layer (0 / 0 before any
 *       batch step);
 *  11 = the sampled batch loop's token selection over the most recent sampled batch step's rows: the multi-row
 *       logits GEMV, the sampler's select and finalize launches (no feedback); bytes = table reads
 *       (ceil(B / llmi_logits_rows_rb(n_embd))) x the F16 table plus the B x vocab f32 logits (0 / 0 before any
 *       sampled batch step);
 *  12 = the span attention launch (+ its merge) of the most recent llmi_session_batch_extend step, one pass over
 *       the layers (with LLMI_BATCH_SPAN_ROWS=1 in the environment at that call: the per-token form the step ran);
 *       bytes = the K and V rows 0..last position of every query block of that step, counted once per block, of one
 *       layer (0 / 0 before any such step);
 *  13 = lookup_step_kernel's draft search (+ the step's tables) over the rows of the most recent
 *       llmi_session_batch_generate_lookup call, with that call's parameters, every row searched whatever is left of
 *       its budget, no state changed; bytes = the history tokens read, 4 bytes x the sum of the rows' history lengths
 *       as the call left them (0 / 0 before any lookup step);
 *  14 = the sampled lookup loop's selection over the token rows of the most recent step of
 *       llmi_session_batch_generate_lookup_sampled that had a live sampled row: the live-row list, the gathered logits
 *       GEMV's chunks, the soft-cap, the sampler's select and finalize launches, into a list and ids of its own (no
 *       state changed); bytes = ceil(n_live / llmi_logits_rows_rb(n_embd)) x the F16 table plus the n_live x vocab f32
 *       logits (after a call under LLMI_LOOKUP_NO_GATHER=1: one read per block of every chunk's token rows, and all
 *       B (draft_len + 1) rows' logits); 0 / 0 before any such step.
 * Returns the mean microseconds and the mean algorithmic bytes per launch
 * (0 / 0 when the family does not exist on this session). */
int llmi_session_time_kernel(llmi_session* s, int which, int reps, double* us_per_launch, double* bytes_per_launch);

/* Device self-tests of arithmetic the exact kernels rely on (synchronous, current device):
 *   0 = every f32 bit pattern through the hardware f32 -> f16 conversion vs the reference's f32_to_f16
 *       (gguf.cpp:68-95): out[0] non-NaN mismatches, out[1] NaN mismatches, out[2] first non-NaN mismatch;
 *   1 = the exact engine's speculative rms_norm sum-of-squares chain vs the serial chain (ops.cpp:33-36) on 8192
 *       vectors of 2560: out[0] differing results (must be 0), out[1] segments recomputed serially;
 *   2 = (no GPU work) the sessions' device memory: out[0] bytes allocated, out[1] bytes released and kept for
 *       reuse, out[2] bytes held back while sessions were constructed concurrently. */
int llmi_selftest(int which, unsigned long long* out);

#ifdef __cplusplus
}
#endif
#endif
