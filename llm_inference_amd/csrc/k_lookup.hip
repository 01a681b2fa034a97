// k_lookup.hip -- lookup decoding (llmi_session_batch_generate_lookup): one launch per step
// that accepts the drafts of the step just scored, appends the emitted ids to the row's history and output ring,
// drafts the next step's tokens by n-gram lookup in the history and writes the next step's device tables (token ids,
// one SeqRow per token row, one AttnBlock per row).  One work-group per row; plain vector stores only, no global
// atomics and no cross-work-group waits -- a row's state is touched by its own work-group alone.
// For sampled rows (llmi_session_batch_generate_lookup_sampled; section 16) the same launch accepts against the rows'
// seeded draws, and two small launches serve the logits those draws need: the list of the step's live token rows and
// the final soft-cap over that list.
#include "sample.h"
#include "session_kernels.h"

namespace llmi {

// The rule (include/llmi.h): history h[0..L), candidate end e in [0, L - 2], ml(e) = the largest
// k <= min(N, e + 1, L - 1) with h[e-k+1..e] == h[L-k..L-1]; the largest (ml, e) with ml >= ngram_min wins; the draft
// continues at c = e + 1 with period P = L - c.
__global__ __launch_bounds__(256) void lookup_step_kernel(LookupArgs a) {
  const int b = blockIdx.x, t = threadIdx.x, W = a.D + 1, base = b * W;
  __shared__ int sh_state[4];                 // len, pos, remaining, done
  __shared__ unsigned long long sh_best[4];   // one packed (ml, e) per wave
  LookupRow* r = a.rows + b;
  int32_t* h = r->hist;
  if (t == 0) {
    int len = r->len, pos = r->pos, rem = r->remaining, done = r->done;
    if (a.mode == LOOKUP_STEP && !done) {
      // accept: span row j ran [cur, d[0..nd)][j] at pos + j, argmax[base + j] is its greedy id.  a[0] always;
      // a[j] while every draft before it was the greedy id; cut after a stop id; never past the row's budget
      const int nd = r->nd, n_out = r->n_out, cap = r->cap;
      int m = 0;
      bool stopped = false;
      for (int j = 0; j <= nd && !stopped; j++) {
        if (j > 0 && a.tok[base + j] != a.argmax[base + j - 1]) break;
        if (m >= rem || len + m >= cap) break;  // (nd <= remaining - 1: not reached)
        const int32_t id = a.argmax[base + j];
        h[len + m] = id;
        a.out[(size_t)b * a.max_new + n_out + m] = id;
        m++;
        for (int i = 0; i < 4; i++) stopped = stopped || (i < a.n_stop && a.stop[i] == id);
      }
      len += m;
      pos += m;
      rem -= m;
      done = (stopped || rem <= 0) ? 1 : 0;
      r->len = len;
      r->pos = pos;
      r->remaining = rem;
      r->n_out = n_out + m;
      r->done = done;
      r->steps += 1;
      r->drafted += nd;
      r->accepted += m - 1;
    }
    if (a.mode != LOOKUP_TIME) a.done[b] = done;
    sh_state[0] = len;
    sh_state[1] = pos;
    sh_state[2] = rem;
    sh_state[3] = done;
  }
  __syncthreads();  // (also orders thread 0's history stores before the reads below)
  const int len = sh_state[0], pos = sh_state[1], rem = sh_state[2];
  const bool done = sh_state[3] != 0 && a.mode != LOOKUP_TIME;
  // the draft: at most `want` tokens (LOOKUP_TIME: the full search whatever the row's budget)
  const int want = a.mode == LOOKUP_TIME ? a.D : done ? 0 : min(a.D, rem - 1);
  int nd = 0, c = 0, P = 1, ml = 0, me = -1;
  if (want > 0 && len >= 2) {  // (block-uniform)
    const int N = a.ngram_max;
    int32_t suf[LOOKUP_NGRAM_MAX];
#pragma unroll
    for (int k = 0; k < LOOKUP_NGRAM_MAX; k++) suf[k] = (k < N && k < len) ? h[len - 1 - k] : -1;
    unsigned long long best = 0;  // (ml << 32 | e) + 1 > 0 for a candidate; 0: none
    for (int e = t; e <= len - 2; e += 256) {
      const int kmax = min(min(N, e + 1), len - 1);
      int k = 0;
      bool run = true;
#pragma unroll
      for (int i = 0; i < LOOKUP_NGRAM_MAX; i++) {
        run = run && i < kmax && h[e - min(i, e)] == suf[i];
        k += run ? 1 : 0;
      }
      if (k >= a.ngram_min) {
        const unsigned long long key = ((unsigned long long)k << 32 | (unsigned)e) + 1ull;
        best = key > best ? key : best;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if ((t & 63) == 0) sh_best[t >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; w++) best = sh_best[w] > best ? sh_best[w] : best;
    if (best) {
      best -= 1ull;
      ml = (int)(best >> 32);
      me = (int)(best & 0xFFFFFFFFull);
      c = me + 1;
      P = len - c;
      nd = want;
    }
  }
  const int32_t cur = h[len - 1];
  // the next step's tables: row j of the span runs [cur, d[0..nd)][j] at pos + j; rows past nd (and every row of a
  // finished row) are "ended" rows (pos -1) that carry a valid token id and append nothing
  if (t < W) {
    a.tok[base + t] = (t >= 1 && t <= nd) ? h[c + (t - 1) % P] : cur;
    SeqRow sr;
    sr.slot = r->slot;
    sr.pos = (!done && t <= nd) ? pos + t : -1;
    a.trows[base + t] = sr;
  }
  if (t == 0) {
    AttnBlock blk;
    blk.tok0 = base;
    blk.n = 1 + nd;
    blk.slot = r->slot;
    blk.pos = done ? -1 : pos;
    a.blocks[b] = blk;
    if (a.mode != LOOKUP_TIME) {
      r->nd = nd;
      r->match_end = me;
      r->match_len = ml;
    }
  }
}

void launch_lookup_step(const LookupArgs& a, hipStream_t s) {
  if (a.B < 1 || a.D < 1 || a.D > LOOKUP_DRAFT_MAX || a.ngram_min < 1 || a.ngram_min > a.ngram_max ||
      a.ngram_max > LOOKUP_NGRAM_MAX || a.n_stop < 0 || a.n_stop > 4 || a.max_new < 1)
    throw std::runtime_error("lookup_step: 1 <= draft_len <= 31, 1 <= ngram_min <= ngram_max <= 8, n_stop <= 4");
  hipLaunchKernelGGL(lookup_step_kernel, dim3(a.B), dim3(256), 0, s, a);
  LLMI_HIP(hipGetLastError());
}

// ---- sampled rows ----
// The live-row list of the step whose tables lookup_step_kernel has written: thread t owns token row t; an inclusive
// scan of the live flags (waves by shuffle, the 8 wave totals through LDS) gives each live row its place, so the list
// is in token-row order and nothing depends on arrival order.  One work-group: T <= 512.
__global__ __launch_bounds__(512) void lookup_live_rows_kernel(LiveRowsArgs a) {
  __shared__ int sh_wave[8];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  SeqRow sr;
  sr.slot = 0;
  sr.pos = -1;
  bool sampled = false;
  if (t < a.T) {
    sr = a.trows[t];
    sampled = a.sp[t / a.W].temperature > 0.0f;
  }
  const bool run = sr.pos >= 0;
  const int live = (t < a.T && (a.all || (run && sampled))) ? 1 : 0;
  const int n_sampling = __syncthreads_count(run && sampled);  // (the snapshot's condition, whatever a.all)
  int inc = live;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int x = __shfl_up(inc, o);
    if (lane >= o) inc += x;
  }
  if (lane == 63) sh_wave[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    before += w < wave ? sh_wave[w] : 0;
    total += sh_wave[w];
  }
  if (live) a.idx[before + inc - 1] = t;
  if (t == 0) *a.n_live = total;
  if (t < a.T) {
    if (run && !sampled && a.argmax) a.ids[t] = a.argmax[t];
    if (a.snap && n_sampling > 0) a.snap[t] = sr;
  }
}

void launch_lookup_live_rows(const LiveRowsArgs& a, hipStream_t s) {
  if (a.T < 1 || a.T > 512 || a.W < 1 || a.T % a.W != 0)
    throw std::runtime_error("lookup_live_rows: 1 <= T <= 512 token rows, W rows per sampler");
  hipLaunchKernelGGL(lookup_live_rows_kernel, dim3(1), dim3(512), 0, s, a);
  LLMI_HIP(hipGetLastError());
}

// softcap_kernel (k_session.hip) over the compact rows below the device count; a work-group past it returns at once
__global__ __launch_bounds__(256) void softcap_live_rows_kernel(float* __restrict__ x, int V, int rows,
                                                                const int32_t* __restrict__ n_live, int base,
                                                                float cap) {
  if ((int)blockIdx.y >= min(rows, *n_live - base)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  float* xr = x + (size_t)blockIdx.y * V;
  if (i < V) xr[i] = cap * llmi_glibc::tanhf(xr[i] / cap);
}

void launch_softcap_live_rows(float* x, int V, int rows, const int32_t* n_live, int base, float cap, hipStream_t s) {
  if (V < 1 || rows < 1 || rows > 65535) throw std::runtime_error("softcap_live_rows: 1 <= rows <= 65535");
  hipLaunchKernelGGL(softcap_live_rows_kernel, dim3((V + 255) / 256, rows), dim3(256), 0, s, x, V, rows, n_live, base,
                     cap);
  LLMI_HIP(hipGetLastError());
}

}  // namespace llmi
