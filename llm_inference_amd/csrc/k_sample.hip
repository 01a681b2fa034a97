// k_sample.hip -- the sampler's two launches (sample.h): the multi-work-group candidate
// selection over a logits row and the one-work-group finalize with the token feedback.  The decode loop's folded
// form of the finalize (with the next step's embed_norm) is in k_session.hip.  The batch loop's rows (section 13) and
// the lookup loop's token rows (section 16) are the same two blocks over many logits rows.
#include "sample.h"
#include "session_kernels.h"

namespace llmi {

__global__ void set_sampler_kernel(SamplerDev* d, float temperature, int top_k, float top_p, unsigned long long seed) {
  d->temperature = temperature;
  d->top_k = top_k;
  d->top_p = top_p;
  d->pad = 0;
  d->seed = seed;
}

void launch_set_sampler(SamplerDev* d, float temperature, int top_k, float top_p, unsigned long long seed,
                        hipStream_t s) {
  hipLaunchKernelGGL(set_sampler_kernel, dim3(1), dim3(1), 0, s, d, temperature, top_k, top_p, seed);
  LLMI_HIP(hipGetLastError());
}

// work-group g: logits [g EPT 1024, (g + 1) EPT 1024) -> its top K keys in surv[g 256 ..], the other slots 0
template <int EPT>
__device__ __forceinline__ void sample_select_block(const float* __restrict__ logits, int V,
                                                    const SamplerDev* __restrict__ sp,
                                                    unsigned long long* __restrict__ surv, SampleShared& sh) {
  const int t = threadIdx.x;
  int K = sp->top_k;
  if (K <= 0 || K > SAMPLE_MAX_K) K = SAMPLE_MAX_K;
  const long long base = (long long)blockIdx.x * (EPT * SAMPLE_THREADS);
  unsigned long long key[EPT];
#pragma unroll
  for (int k = 0; k < EPT; k++) {
    const long long i = base + (long long)k * SAMPLE_THREADS + t;
    key[k] = i < (long long)V ? sample_key(logits[i], (uint32_t)i) : 0ull;
  }
  const unsigned long long thr = sample_block_threshold<EPT>(key, K, sh);
  if (t < SAMPLE_MAX_K) sh.key[t] = 0ull;
  if (t == 0) sh.slot = 0u;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < EPT; k++)
    if (key[k] != 0ull && key[k] >= thr) {
      const unsigned slot = atomicAdd(&sh.slot, 1u);
      if (slot < (unsigned)SAMPLE_MAX_K) sh.key[slot] = key[k];
    }
  __syncthreads();
  if (t < SAMPLE_MAX_K) surv[(size_t)blockIdx.x * SAMPLE_MAX_K + t] = sh.key[t];
}

template <int EPT>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_select_kernel(const float* __restrict__ logits, int V,
                                                                       const SamplerDev* __restrict__ sp,
                                                                       unsigned long long* __restrict__ surv) {
  __shared__ SampleShared sh;
  sample_select_block<EPT>(logits, V, sp, surv, sh);
}

void launch_sample_select(const float* logits, int V, const SamplerDev* sp, unsigned long long* surv, hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  if (ept == 4)
    hipLaunchKernelGGL(sample_select_kernel<4>, dim3(g), dim3(SAMPLE_THREADS), 0, s, logits, V, sp, surv);
  else if (ept == 8)
    hipLaunchKernelGGL(sample_select_kernel<8>, dim3(g), dim3(SAMPLE_THREADS), 0, s, logits, V, sp, surv);
  else
    hipLaunchKernelGGL(sample_select_kernel<16>, dim3(g), dim3(SAMPLE_THREADS), 0, s, logits, V, sp, surv);
  LLMI_HIP(hipGetLastError());
}

__global__ __launch_bounds__(SAMPLE_THREADS) void sample_finalize_kernel(
    const unsigned long long* __restrict__ surv, int n_surv, const SamplerDev* __restrict__ sp,
    int32_t* __restrict__ d_pos, int32_t* __restrict__ d_token, int32_t* __restrict__ ring,
    int32_t* __restrict__ ring_idx, int ring_cap, unsigned long long* __restrict__ keys, int n_keys,
    SampleDbg* __restrict__ dbg) {
  __shared__ SampleShared sh;
  const int pos = *d_pos;
  const int tok = sample_finalize_block(surv, n_surv, sp, pos, dbg, sh);
  if (threadIdx.x == 0 && d_token) {
    const int i = *ring_idx;
    for (int q = 0; q < n_keys; q++) keys[q] = 0ull;
    *d_token = tok;
    *d_pos = pos + 1;
    if (i < ring_cap) ring[i] = tok;
    *ring_idx = i + 1;
  }
}

void launch_sample_finalize(const unsigned long long* surv, int V, const SamplerDev* sp, int32_t* d_pos,
                            int32_t* d_token, int32_t* ring, int32_t* ring_idx, int ring_cap,
                            unsigned long long* keys, int n_keys, SampleDbg* dbg, hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  hipLaunchKernelGGL(sample_finalize_kernel, dim3(1), dim3(SAMPLE_THREADS), 0, s, surv, g * SAMPLE_MAX_K, sp, d_pos,
                     d_token, ring, ring_idx, ring_cap, keys, n_keys, dbg);
  LLMI_HIP(hipGetLastError());
}

// ---- the batch loop's rows ----
// Work-group (g, b): sample_select_kernel's work-group g on logits row b with sp[b], into surv[b][g].  A row that
// has ended (pos < 0) or decodes greedily (temperature 0: its id is the scorer's arg-max) selects nothing.
template <int EPT>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_select_rows_kernel(const float* __restrict__ logits, int V,
                                                                            const SamplerDev* __restrict__ sp,
                                                                            const SeqRow* __restrict__ rows,
                                                                            unsigned long long* __restrict__ surv) {
  __shared__ SampleShared sh;
  const int b = blockIdx.y;
  if (rows[b].pos < 0 || sp[b].temperature == 0.0f) return;
  sample_select_block<EPT>(logits + (size_t)b * V, V, sp + b, surv + (size_t)b * SAMPLE_MAX_GROUPS * SAMPLE_MAX_K, sh);
}

void launch_sample_select_rows(const float* logits, int V, int B, const SamplerDev* sp, const SeqRow* rows,
                               unsigned long long* surv, hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  if (B < 1 || B > 64) throw std::runtime_error("sample_select_rows: 1 <= B <= 64");
  const dim3 grid(g, B);
  if (ept == 4)
    hipLaunchKernelGGL(sample_select_rows_kernel<4>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, sp, rows, surv);
  else if (ept == 8)
    hipLaunchKernelGGL(sample_select_rows_kernel<8>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, sp, rows, surv);
  else
    hipLaunchKernelGGL(sample_select_rows_kernel<16>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, sp, rows, surv);
  LLMI_HIP(hipGetLastError());
}

// Work-group b: row b's id -- sample_finalize_block on its survivors with sp[b] at pos = rows[b].pos, or argmax[b]
// for a greedy row -- then batch_feedback_kernel's feedback for the row (feedback 0: time_kernel, nothing written).
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_finalize_rows_kernel(
    const unsigned long long* __restrict__ surv, int n_surv, const SamplerDev* __restrict__ sp,
    const int32_t* __restrict__ argmax, SeqRow* __restrict__ rows, int32_t* __restrict__ tokens, BatchStops stops,
    int32_t* __restrict__ out, int feedback) {
  __shared__ SampleShared sh;
  const int b = blockIdx.x;
  const SeqRow sr = rows[b];
  __syncthreads();  // (thread 0 rewrites rows[b] below)
  if (sr.pos < 0) {
    if (threadIdx.x == 0 && feedback) out[b] = -1;
    return;
  }
  int id;
  if (sp[b].temperature == 0.0f)
    id = argmax[b];
  else
    id = sample_finalize_block(surv + (size_t)b * SAMPLE_MAX_GROUPS * SAMPLE_MAX_K, n_surv, sp + b, sr.pos, nullptr, sh);
  if (threadIdx.x != 0 || !feedback) return;
  out[b] = id;
  bool stop = false;
  for (int i = 0; i < 4; i++) stop = stop || (i < stops.n && stops.id[i] == id);
  if (stop) {
    rows[b].pos = -1;
  } else {
    tokens[b] = id;
    rows[b].pos = sr.pos + 1;
  }
}

void launch_sample_finalize_rows(const unsigned long long* surv, int V, int B, const SamplerDev* sp,
                                 const int32_t* argmax, SeqRow* rows, int32_t* tokens, const BatchStops& stops,
                                 int32_t* out, bool feedback, hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  if (B < 1 || B > 64) throw std::runtime_error("sample_finalize_rows: 1 <= B <= 64");
  hipLaunchKernelGGL(sample_finalize_rows_kernel, dim3(B), dim3(SAMPLE_THREADS), 0, s, surv, g * SAMPLE_MAX_K, sp,
                     argmax, rows, tokens, stops, out, feedback ? 1 : 0);
  LLMI_HIP(hipGetLastError());
}

// ---- the lookup loop's token rows ----
// Compact row i of the launch (logits row i, survivors surv[i]) is token row t = idx[i] of the step, with the sampler
// *q and the position trows[t].pos.  The rows at and past the device count, ended token rows and greedy rows' token
// rows leave at once.  -1: none
__device__ __forceinline__ int sample_token_row(int i, const TokenRowsArgs& a, const SamplerDev** q) {
  if (i >= min(a.cap, *a.n_live - a.base)) return -1;
  const int t = a.idx[i];
  *q = a.sp + (a.sp_of ? a.sp_of[t] : t / a.W);
  if (a.trows[t].pos < 0 || (*q)->temperature == 0.0f) return -1;
  return t;
}

template <int EPT>
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_select_token_rows_kernel(const float* __restrict__ logits,
                                                                                  int V, TokenRowsArgs a,
                                                                                  unsigned long long* __restrict__ surv) {
  __shared__ SampleShared sh;
  const SamplerDev* q = nullptr;
  const int i = blockIdx.y, t = sample_token_row(i, a, &q);
  if (t < 0) return;
  sample_select_block<EPT>(logits + (size_t)i * V, V, q, surv + (size_t)i * SAMPLE_MAX_GROUPS * SAMPLE_MAX_K, sh);
}

void launch_sample_select_token_rows(const float* logits, int V, const TokenRowsArgs& a, unsigned long long* surv,
                                     hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  if (a.cap < 1 || a.cap > 512 || a.W < 1) throw std::runtime_error("sample_select_token_rows: 1 <= cap <= 512");
  const dim3 grid(g, a.cap);
  if (ept == 4)
    hipLaunchKernelGGL(sample_select_token_rows_kernel<4>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, a, surv);
  else if (ept == 8)
    hipLaunchKernelGGL(sample_select_token_rows_kernel<8>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, a, surv);
  else
    hipLaunchKernelGGL(sample_select_token_rows_kernel<16>, grid, dim3(SAMPLE_THREADS), 0, s, logits, V, a, surv);
  LLMI_HIP(hipGetLastError());
}

// Work-group i: ids[t] = sample_finalize_block on compact row i's survivors at pos = trows[t].pos.  No token feedback:
// lookup_step_kernel reads ids where the greedy loop reads the scorer's arg-max.
__global__ __launch_bounds__(SAMPLE_THREADS) void sample_finalize_token_rows_kernel(
    const unsigned long long* __restrict__ surv, int n_surv, TokenRowsArgs a, int32_t* __restrict__ ids) {
  __shared__ SampleShared sh;
  const SamplerDev* q = nullptr;
  const int i = blockIdx.x, t = sample_token_row(i, a, &q);
  if (t < 0) return;
  const int id = sample_finalize_block(surv + (size_t)i * SAMPLE_MAX_GROUPS * SAMPLE_MAX_K, n_surv, q, a.trows[t].pos,
                                       nullptr, sh);
  if (threadIdx.x == 0) ids[t] = id;
}

void launch_sample_finalize_token_rows(const unsigned long long* surv, int V, const TokenRowsArgs& a, int32_t* ids,
                                       hipStream_t s) {
  int ept = 0;
  const int g = V > 0 ? sample_groups(V, &ept) : 0;
  if (g == 0) throw std::runtime_error("sample: between 1 and 1,048,576 logits");
  if (a.cap < 1 || a.cap > 512 || a.W < 1) throw std::runtime_error("sample_finalize_token_rows: 1 <= cap <= 512");
  hipLaunchKernelGGL(sample_finalize_token_rows_kernel, dim3(a.cap), dim3(SAMPLE_THREADS), 0, s, surv, g * SAMPLE_MAX_K,
                     a, ids);
  LLMI_HIP(hipGetLastError());
}

}  // namespace llmi
