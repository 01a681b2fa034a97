// sample.h -- seeded temperature / top-k / top-p sampling of one logits row.
//
// Two launches (k_sample.hip; the second also as the decode loop's folded token feedback in k_session.hip):
//   select    G work-groups, each over a contiguous chunk of the row: the chunk's top K keys (any member of the
//             row's top K is in its chunk's top K), 256 slots per work-group, unused slots 0;
//   finalize  one work-group: the top K of the G x 256 survivors, sorted, then the integer weights, the nucleus
//             cut, the draw and the token feedback.
// A key is 64 bits: the logit as an order-preserving u32 (-0 read as +0) above the inverted id, so keys are
// distinct, "greater" is "higher logit, then lower id", and 0 is free for "no key" (NaN logits, padding).  The top K
// are found by a radix threshold select over the key bits that differ inside the set (the id bits included:
// all-equal logits refine through the ids), 8 bits a pass with an LDS histogram, and taken as key >= threshold.
// The only atomics are integer adds in LDS (counts and slots); the selected SET is fixed by the threshold and its
// order by a sort of distinct keys, so nothing depends on arrival order.
#pragma once

#include "common.h"
#include "glibc_math.h"

namespace llmi {

constexpr int SAMPLE_MAX_K = 256;       // LLMI_SAMPLE_MAX_K
constexpr int SAMPLE_THREADS = 1024;
constexpr int SAMPLE_MAX_GROUPS = 64;   // finalize holds 16 survivor keys per thread: 64 x 256
constexpr int SAMPLE_FIN_EPT = SAMPLE_MAX_GROUPS * SAMPLE_MAX_K / SAMPLE_THREADS;

struct SamplerDev {  // the session's sampler, device-resident (launch_set_sampler writes it in stream order)
  float temperature;
  int top_k;  // 1..256
  float top_p;
  int pad;
  unsigned long long seed;
};

struct SampleDbg {  // what llmi_sample_logits returns besides the token
  int token, n_cand, n_nucleus, pad;
  int cand[SAMPLE_MAX_K];
  unsigned long long q[SAMPLE_MAX_K];
};

// work-groups of the select launch and logits per thread (4 up to 262,144 logits, then 8, then 16); 0: the row is
// too long
inline int sample_groups(int V, int* ept) {
  for (int e : {4, 8, 16}) {
    const long long chunk = (long long)SAMPLE_THREADS * e;
    const long long g = ((long long)V + chunk - 1) / chunk;
    if (g <= SAMPLE_MAX_GROUPS) {
      *ept = e;
      return (int)(g < 1 ? 1 : g);
    }
  }
  return 0;
}

#if defined(__HIPCC__)

struct SampleShared {
  unsigned hist[256];
  unsigned wsum[4];
  unsigned long long red[2 * SAMPLE_THREADS / 64];
  unsigned bin, above, cnt, slot;
  unsigned long long key[SAMPLE_MAX_K];
  unsigned long long Q[SAMPLE_MAX_K];
  unsigned long long qsum[4];
  unsigned n_lt, j_le;
  int tok;
};

__device__ __forceinline__ unsigned long long sample_key(float l, uint32_t id) {
  uint32_t u = __float_as_uint(l);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0ull;  // NaN: never a candidate
  if ((u & 0x7fffffffu) == 0u) u = 0u;               // -0 ties with +0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((unsigned long long)u << 32) | (0xFFFFFFFFu - id);
}
__device__ __forceinline__ float sample_key_logit(unsigned long long k) {
  const uint32_t u = (uint32_t)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// The K-th greatest of the work-group's non-zero keys (EPT per thread; all of them when there are fewer than K),
// the same value in every thread.  {key != 0 and key >= result} are exactly min(K, keys) keys; the result itself may
// be 0 with keys present (a bin of all-zero prefix bits taken whole: -inf or a logit <= -2^127 as the K-th), so
// callers test the keys, never the threshold, against 0.
// Every thread of the SAMPLE_THREADS-wide work-group must call it (barriers inside).
template <int EPT>
__device__ unsigned long long sample_block_threshold(const unsigned long long (&key)[EPT], int K, SampleShared& sh) {
  constexpr int NW = SAMPLE_THREADS / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  unsigned long long mx = 0ull, mn = ~0ull;
#pragma unroll
  for (int k = 0; k < EPT; k++) {
    mx = key[k] > mx ? key[k] : mx;
    mn = (key[k] != 0ull && key[k] < mn) ? key[k] : mn;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long a = __shfl_xor(mx, o), b = __shfl_xor(mn, o);
    mx = a > mx ? a : mx;
    mn = b < mn ? b : mn;
  }
  __syncthreads();  // (sh may still be read from an earlier use)
  if (lane == 0) {
    sh.red[wave] = mx;
    sh.red[NW + wave] = mn;
  }
  __syncthreads();
  for (int w = 0; w < NW; w++) {
    const unsigned long long a = sh.red[w], b = sh.red[NW + w];
    mx = a > mx ? a : mx;
    mn = b < mn ? b : mn;
  }
  if (mx == 0ull) return 0ull;
  // the bits above `hi` are the same in every key: the passes start at the first bit that differs
  const unsigned long long diff = mx ^ mn;
  int hi = diff ? 64 - __clzll((long long)diff) : 0;
  unsigned long long prefix = mx;
  unsigned need = (unsigned)K;
  bool first = true;
  while (hi > 0) {
    const int w = hi < 8 ? hi : 8, shift = hi - w;
    const unsigned long long pre_hi = hi >= 64 ? 0ull : (prefix >> hi);
    if (t < 256) sh.hist[t] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < EPT; k++) {
      const unsigned long long kk = key[k];
      if (kk != 0ull && (hi >= 64 ? 0ull : (kk >> hi)) == pre_hi)
        atomicAdd(&sh.hist[(unsigned)(kk >> shift) & ((1u << w) - 1u)], 1u);
    }
    __syncthreads();
    unsigned v = 0u, s = 0u;
    if (t < 256) {  // s: keys in this wave's bins >= t
      v = sh.hist[t];
      s = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned x = __shfl_down(s, o);
        if (lane + o < 64) s += x;
      }
      if (lane == 0) sh.wsum[wave] = s;
    }
    __syncthreads();
    if (first) {
      const unsigned total = sh.wsum[0] + sh.wsum[1] + sh.wsum[2] + sh.wsum[3];
      need = need < total ? need : total;
      first = false;
    }
    if (t < 256) {
      for (int ww = wave + 1; ww < 4; ww++) s += sh.wsum[ww];
      if (s >= need && s - v < need) {  // the bin that holds the need-th greatest key
        sh.bin = (unsigned)t;
        sh.above = s - v;
        sh.cnt = v;
      }
    }
    __syncthreads();
    const unsigned b = sh.bin, cnt = sh.cnt;
    need -= sh.above;
    prefix = (hi >= 64 ? 0ull : (pre_hi << hi)) | ((unsigned long long)b << shift);
    hi = shift;
    if (cnt == need) break;  // the whole bin is taken: the bits below stay 0
  }
  return hi >= 64 ? 0ull : (prefix >> hi) << hi;
}

// finalize: the top K of `n_surv` survivor keys, sorted; weights, nucleus, draw.
// Returns the token in every thread.  dbg may be null.
__device__ int sample_finalize_block(const unsigned long long* __restrict__ surv, int n_surv,
                                     const SamplerDev* __restrict__ sp, int pos, SampleDbg* __restrict__ dbg,
                                     SampleShared& sh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float T = sp->temperature, top_p = sp->top_p;
  int K = sp->top_k;
  if (K <= 0 || K > SAMPLE_MAX_K) K = SAMPLE_MAX_K;
  const unsigned long long seed = sp->seed;
  unsigned long long key[SAMPLE_FIN_EPT];
#pragma unroll
  for (int k = 0; k < SAMPLE_FIN_EPT; k++) {
    const int i = t + k * SAMPLE_THREADS;
    key[k] = i < n_surv ? surv[i] : 0ull;
  }
  const unsigned long long thr = sample_block_threshold<SAMPLE_FIN_EPT>(key, K, sh);
  if (t < SAMPLE_MAX_K) sh.key[t] = 0ull;
  if (t == 0) {
    sh.slot = 0u;
    sh.n_lt = 0u;
    sh.j_le = 0u;
    sh.tok = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SAMPLE_FIN_EPT; k++)
    if (key[k] != 0ull && key[k] >= thr) {
      const unsigned slot = atomicAdd(&sh.slot, 1u);
      if (slot < (unsigned)SAMPLE_MAX_K) sh.key[slot] = key[k];
    }
  __syncthreads();
  const int n_cand = (int)(sh.slot < (unsigned)SAMPLE_MAX_K ? sh.slot : (unsigned)SAMPLE_MAX_K);
  // bitonic sort, descending (distinct keys: the order is unique), over the power of two that holds the candidates
  int P = 2;
  while (P < n_cand) P <<= 1;
  for (int k = 2; k <= P; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (t < P) {
        const int x = t ^ j;
        if (x > t) {
          const unsigned long long a = sh.key[t], b = sh.key[x];
          if ((t & k) == 0 ? a < b : a > b) {
            sh.key[t] = b;
            sh.key[x] = a;
          }
        }
      }
      __syncthreads();
    }
  if (n_cand == 0) {  // every logit NaN: token 0 (finalize_token_kernel's rule)
    if (dbg) {
      if (t < SAMPLE_MAX_K) {
        dbg->cand[t] = -1;
        dbg->q[t] = 0ull;
      }
      if (t == 0) {
        dbg->token = 0;
        dbg->n_cand = 0;
        dbg->n_nucleus = 0;
      }
    }
    return 0;
  }
  // integer weights: t_i = (l_i - l_0) / T (f32, correctly rounded), w_i = glibc expf, q_i = floor(w_i 2^32)
  const bool valid = t < n_cand;
  const unsigned long long k0 = sh.key[0];
  const unsigned long long kt = valid ? sh.key[t] : 0ull;
  const int cand = valid ? (int)(0xFFFFFFFFu - (uint32_t)(kt & 0xFFFFFFFFull)) : -1;
  const float l0 = sample_key_logit(k0);
  const bool top_finite = (__float_as_uint(l0) & 0x7f800000u) != 0x7f800000u;
  unsigned long long q = 0ull;
  if (valid) {
    if (top_finite) {
      const float ti = __fdiv_rn(__fsub_rn(sample_key_logit(kt), l0), T);
      const float wi = llmi_glibc::expf(ti);
      q = (unsigned long long)((double)wi * 4294967296.0);
    } else {
      q = t == 0 ? (1ull << 32) : 0ull;  // a non-finite top logit: the token is c_0
    }
  }
  // Q_j = q_0 + ... + q_j (u64)
  unsigned long long Q = q;
  if (t < SAMPLE_MAX_K) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned long long x = __shfl_up(Q, o);
      if (lane >= o) Q += x;
    }
    if (lane == 63) sh.qsum[wave] = Q;
  }
  __syncthreads();
  if (t < SAMPLE_MAX_K) {
    for (int ww = 0; ww < wave; ww++) Q += sh.qsum[ww];
    sh.Q[t] = Q;
  }
  __syncthreads();
  const unsigned long long Qtot = sh.Q[n_cand - 1];
  int n = n_cand;
  if (top_p < 1.0f) {  // nucleus: the smallest n >= 1 with Q_{n-1} >= thr
    const unsigned long long pthr = (unsigned long long)((double)top_p * (double)Qtot);
    if (valid && Q < pthr) atomicAdd(&sh.n_lt, 1u);
    __syncthreads();
    n = (int)sh.n_lt + 1;
    n = n < n_cand ? n : n_cand;
  }
  // draw: splitmix64 of seed + (pos + 1) golden, 24 bits
  unsigned long long z = seed + (unsigned long long)(long long)(pos + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z ^= z >> 31;
  const unsigned long long u = z >> 40;
  const unsigned long long r = (u * sh.Q[n - 1]) >> 24;
  if (t < n && Q <= r) atomicAdd(&sh.j_le, 1u);  // Q is non-decreasing: j = the number of Q_i <= r
  __syncthreads();
  const int j = (int)sh.j_le;
  if (t == j) sh.tok = cand;  // j < n: r < Q_{n-1}
  __syncthreads();
  const int tok = sh.tok;
  if (dbg) {
    if (t < SAMPLE_MAX_K) {
      dbg->cand[t] = cand;
      dbg->q[t] = q;
    }
    if (t == 0) {
      dbg->token = tok;
      dbg->n_cand = n_cand;
      dbg->n_nucleus = n;
    }
  }
  return tok;
}

#endif  // __HIPCC__

// k_sample.hip
void launch_set_sampler(SamplerDev* d, float temperature, int top_k, float top_p, unsigned long long seed,
                        hipStream_t s);
// surv: sample_groups(V) x 256 keys
void launch_sample_select(const float* logits, int V, const SamplerDev* sp, unsigned long long* surv, hipStream_t s);
// one work-group: the token from the survivors.  d_pos: the position of the token whose logits were sampled.
// feedback (d_token non-null): d_token = token, d_pos += 1, ring[ring_idx++] = token, the n_keys argmax keys back to
// 0 -- what finalize_token_kernel does.  dbg may be null.
void launch_sample_finalize(const unsigned long long* surv, int V, const SamplerDev* sp, int32_t* d_pos,
                            int32_t* d_token, int32_t* ring, int32_t* ring_idx, int ring_cap,
                            unsigned long long* keys, int n_keys, SampleDbg* dbg, hipStream_t s);

// The batch loop's rows (Session::batch_generate_sampled): the two launches over B logits rows
// [B][V], sampler sp[b] per row, survivors surv [B][SAMPLE_MAX_GROUPS x 256].  Row b is the one-row launches' work
// on logits row b with sp[b] at pos = rows[b].pos; a row with sp[b].temperature == 0 is greedy (its id is
// argmax[b], the fused scorer's) and a row with rows[b].pos < 0 has ended: both leave the select launch at once.
// The finalize launch is also the row's launch_batch_feedback (session_kernels.h): out[b] = id (-1: ended), a stop
// id ends the row, any other id becomes tokens[b] at rows[b].pos + 1.  feedback false (time_kernel): writes nothing.
struct SeqRow;
struct BatchStops;
void launch_sample_select_rows(const float* logits, int V, int B, const SamplerDev* sp, const SeqRow* rows,
                               unsigned long long* surv, hipStream_t s);
void launch_sample_finalize_rows(const unsigned long long* surv, int V, int B, const SamplerDev* sp,
                                 const int32_t* argmax, SeqRow* rows, int32_t* tokens, const BatchStops& stops,
                                 int32_t* out, bool feedback, hipStream_t s);

// The lookup loop's token rows (Session::batch_generate_lookup_sampled): the two launches over
// `cap` compact rows -- logits [cap][V], survivors [cap][SAMPLE_MAX_GROUPS x 256] -- of a device list.  Compact row i
// (i < min(cap, *n_live - base); idx points at entry `base`) is token row t = idx[i]: the one-row launches' work on
// logits row i with sampler sp[sp_of ? sp_of[t] : t / W] at pos = trows[t].pos, its id into ids[t].  A token row with
// trows[t].pos < 0 has ended and one whose sampler has temperature 0 is greedy (the caller fills its id): both are
// skipped, as are the rows at and past the count.  No token feedback: lookup_step_kernel reads ids.
struct TokenRowsArgs {
  const int32_t* idx = nullptr;
  const int32_t* n_live = nullptr;
  int base = 0, cap = 0, W = 1;
  const SamplerDev* sp = nullptr;
  const int32_t* sp_of = nullptr;
  const SeqRow* trows = nullptr;
};
void launch_sample_select_token_rows(const float* logits, int V, const TokenRowsArgs& a, unsigned long long* surv,
                                     hipStream_t s);
void launch_sample_finalize_token_rows(const unsigned long long* surv, int V, const TokenRowsArgs& a, int32_t* ids,
                                       hipStream_t s);

// k_session.hip: launch_sample_finalize with the feedback, then the next step's embed_norm (as
// launch_finalize_embed_norm)
struct NormOut;
void launch_sample_finalize_embed_norm(const unsigned long long* surv, int V, const SamplerDev* sp,
                                       unsigned long long* keys, int n_keys, int32_t* d_token, int32_t* d_pos,
                                       int32_t* ring, int32_t* ring_idx, int ring_cap, uint32_t type,
                                       const uint8_t* table, size_t row_bytes, float emb_scale, float* resid,
                                       const float* w, const NormOut& out, int n, double eps, bool exact,
                                       hipStream_t s);

}  // namespace llmi
