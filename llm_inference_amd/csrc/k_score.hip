// k_score.hip -- teacher-forced scoring (llmi_session_score / llmi_score_rows).
//
// Fused scorer: S = X16 . W16^T on v_mfma_f32_32x32x16_f16, reduced in registers / LDS to per-token
// log-sum-exp, target log-prob and first-index argmax; the T x V logits never reach memory.
//  * A work-group (4 waves) owns SCORE_VT = 128 vocabulary rows (wave w: rows 32 w .. + 31) and loops over the
//    chunk's token tiles of SCORE_TT = 128 (4 MFMA tiles per wave).  Per 64-k stage the threads stage the
//    [128][64] table tile and the [128][64] token tile through registers into two f16 LDS tiles (128-B rows, 16-B
//    units XOR-swizzled as GEMM v7's), the next stage's global loads in flight during the MFMAs.
//  * The f32 accumulator is carried over all of E in k order: every logit is one fixed chain whatever T, the
//    chunking or the tile a token lands in.
//  * Ragged edges: rows past V / tokens past T re-read the last valid row (score_plan.h) and are masked in the
//    epilogue (they contribute nothing); 16-B units past E load as zeros.
//  * Epilogue per (token, wave): the soft-cap, max, sum exp(l - max) and argmax_key over the wave's 32 rows (16 per
//    lane, then the other half-wave), the 4 waves merged in wave order through LDS: one partial per (token,
//    vocabulary tile).  The target's logit is written by the one lane that holds it.
//  * score_merge_kernel: per token, max and key over the tiles, then sum_i s_i exp(m_i - M) in f64 (strided per
//    thread in tile order, a fixed LDS tree across threads): deterministic, no float atomics.
#include "kernels.h"
#include "score_plan.h"

namespace llmi {

namespace {

typedef _Float16 sc_f16x8 __attribute__((ext_vector_type(8)));
typedef float sc_v16f __attribute__((ext_vector_type(16)));

// 16-B unit u of LDS row `row` (128-B rows), k_prefill.hip's pg7_slot
__device__ __forceinline__ int sc_slot(int row, int u) { return row * 8 + (u ^ ((row ^ (row >> 1)) & 7)); }

__device__ __forceinline__ unsigned long long sc_shfl_xor_u64(unsigned long long v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((unsigned long long)hi << 32) | lo;
}

__global__ __launch_bounds__(256, 2) void score_partials_kernel(ScoreArgs a, int n_vt) {
  constexpr int NU = SCORE_VT * 8 / 256;  // 16-B units of a tile's stage per thread (both tiles: 128 rows)
  static_assert(SCORE_VT == 128 && SCORE_TT == 128 && SCORE_KS == 64 && NU == 4, "tile geometry");
  __shared__ __attribute__((aligned(16))) unsigned char s_w[SCORE_VT * 128];
  __shared__ __attribute__((aligned(16))) unsigned char s_x[SCORE_TT * 128];
  __shared__ float s_m[4][SCORE_TT], s_s[4][SCORE_TT];
  __shared__ unsigned long long s_k[4][SCORE_TT];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
  const int vt = blockIdx.x, v0 = vt * SCORE_VT;
  const int E = a.E, nst = (E + SCORE_KS - 1) / SCORE_KS, n_tt = (a.T + SCORE_TT - 1) / SCORE_TT;
  const int ku = t & 7;  // this thread's 16-B unit of every row it loads (unit g = u 256 + t: row g / 8)
  size_t woff[NU];
#pragma unroll
  for (int u = 0; u < NU; u++) woff[u] = (size_t)min(v0 + ((u * 256 + t) >> 3), a.V - 1) * E + ku * 8;
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  for (int tt = 0; tt < n_tt; tt++) {
    const int tk0 = tt * SCORE_TT;
    size_t xoff[NU];
#pragma unroll
    for (int u = 0; u < NU; u++) xoff[u] = (size_t)min(tk0 + ((u * 256 + t) >> 3), a.T - 1) * a.xstride + ku * 8;
    u32x4_t wr[NU], xr[NU];
    auto load = [&](int c) {
      const bool in = c * SCORE_KS + ku * 8 < E;  // E % 8 == 0: a unit is inside or outside as a whole
#pragma unroll
      for (int u = 0; u < NU; u++) {
        wr[u] = in ? *reinterpret_cast<const u32x4_t*>(a.w16 + woff[u] + (size_t)c * SCORE_KS) : zero4;
        xr[u] = in ? *reinterpret_cast<const u32x4_t*>(a.x16 + xoff[u] + (size_t)c * SCORE_KS) : zero4;
      }
    };
    sc_v16f acc[4];
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] = sc_v16f{};
    load(0);
    for (int c = 0; c < nst; c++) {
      __syncthreads();  // every read of the previous stage (and of the previous tile's s_m / s_s / s_k)
#pragma unroll
      for (int u = 0; u < NU; u++) {
        const int row = (u * 256 + t) >> 3;
        *reinterpret_cast<u32x4_t*>(s_w + sc_slot(row, ku) * 16) = wr[u];
        *reinterpret_cast<u32x4_t*>(s_x + sc_slot(row, ku) * 16) = xr[u];
      }
      __syncthreads();
      if (c + 1 < nst) load(c + 1);
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {  // 16 k per MFMA: lane half h holds k 16 ks + 8 h .. + 7 (unit 2 ks + h)
        const sc_f16x8 A = *reinterpret_cast<const sc_f16x8*>(s_w + sc_slot(32 * w + r, 2 * ks + h) * 16);
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const sc_f16x8 B = *reinterpret_cast<const sc_f16x8*>(s_x + sc_slot(32 * j + r, 2 * ks + h) * 16);
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A, B, acc[j], 0, 0, 0);
        }
      }
    }
    // acc[j][i] = logit of row v0 + 32 w + 8 (i >> 2) + 4 h + (i & 3), token tk0 + 32 j + r
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int tok = tk0 + 32 * j + r;
      const int tgt = (a.targets && tok < a.T) ? a.targets[tok] : -1;
      float lv[16];
      float m = -INFINITY;
      unsigned long long key = 0;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int row = v0 + 32 * w + 8 * (i >> 2) + 4 * h + (i & 3);
        float l = acc[j][i];
        if (a.softcap > 0.0f) l = a.softcap * llmi_glibc::tanhf(l / a.softcap);  // softcap_kernel's expression
        lv[i] = l;
        if (row < a.V) {
          m = fmaxf(m, l);
          const unsigned long long k = argmax_key(l, (uint32_t)row);
          key = k > key ? k : key;
          if (row == tgt) a.tl[tok] = l;  // tok < T here (tgt >= 0); one lane of the whole grid
        }
      }
      m = fmaxf(m, __shfl_xor(m, 32));
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int row = v0 + 32 * w + 8 * (i >> 2) + 4 * h + (i & 3);
        if (row < a.V) s += expf(lv[i] - m);
      }
      s += __shfl_xor(s, 32);
      const unsigned long long ko = sc_shfl_xor_u64(key, 32);
      key = ko > key ? ko : key;
      if (h == 0) {
        s_m[w][32 * j + r] = m;
        s_s[w][32 * j + r] = s;
        s_k[w][32 * j + r] = key;
      }
    }
    __syncthreads();
    if (t < SCORE_TT && tk0 + t < a.T) {  // the 4 waves' 32-row partials in wave order
      float M = s_m[0][t];
      unsigned long long key = s_k[0][t];
#pragma unroll
      for (int q = 1; q < 4; q++) {
        M = fmaxf(M, s_m[q][t]);
        key = s_k[q][t] > key ? s_k[q][t] : key;
      }
      float S = 0.0f;
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (s_s[q][t] > 0.0f) S += s_s[q][t] * expf(s_m[q][t] - M);  // (a wave past V: s = 0, m = -inf)
      const size_t o = (size_t)(tk0 + t) * n_vt + vt;
      a.ms[o] = make_float2(M, S);
      a.key[o] = key;
    }
  }
}

// f64 block sum in a fixed order (LDS tree), 256 threads
__device__ __forceinline__ double sc_block_sum256(double v, double* sh) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o) sh[t] = sh[t] + sh[t + o];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void score_merge_kernel(ScoreArgs a, int n_vt) {
  __shared__ double sh[256];
  __shared__ float s_mx[256];
  __shared__ unsigned long long s_key[256];
  const int t = threadIdx.x, tok = blockIdx.x;
  const float2* ms = a.ms + (size_t)tok * n_vt;
  const unsigned long long* keys = a.key + (size_t)tok * n_vt;
  float m = -INFINITY;
  unsigned long long key = 0;
  for (int i = t; i < n_vt; i += 256) {
    m = fmaxf(m, ms[i].x);
    key = keys[i] > key ? keys[i] : key;
  }
  s_mx[t] = m;
  s_key[t] = key;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o) {
      s_mx[t] = fmaxf(s_mx[t], s_mx[t + o]);
      s_key[t] = s_key[t + o] > s_key[t] ? s_key[t + o] : s_key[t];
    }
    __syncthreads();
  }
  const double M = (double)s_mx[0];
  double sum = 0.0;
  for (int i = t; i < n_vt; i += 256) {
    const float2 p = ms[i];
    if (p.y > 0.0f) sum += (double)p.y * exp((double)p.x - M);
  }
  sum = sc_block_sum256(sum, sh);
  if (t == 0) {
    const double lse = M + log(sum);
    const int tgt = a.targets ? a.targets[tok] : -1;
    if (a.lse) a.lse[tok] = (float)lse;
    if (a.logprob) a.logprob[tok] = tgt >= 0 ? (float)((double)a.tl[tok] - lse) : 0.0f;
    if (a.argmax) a.argmax[tok] = s_key[0] ? (int32_t)argmax_key_index(s_key[0]) : 0;  // (every logit NaN: id 0)
  }
}

// Row path: one f32 logits row (forward's, after the soft-cap)
__global__ __launch_bounds__(1024) void score_reduce_row_kernel(const float* __restrict__ x, int n, int target,
                                                                float* logprob, float* lse, int32_t* argmax) {
  __shared__ double sh[1024];
  __shared__ float s_mx[1024];
  __shared__ unsigned long long s_key[1024];
  const int t = threadIdx.x;
  float m = -INFINITY;
  unsigned long long key = 0;
  for (int i = t; i < n; i += 1024) {
    const float v = x[i];
    m = fmaxf(m, v);
    const unsigned long long k = argmax_key(v, (uint32_t)i);
    key = k > key ? k : key;
  }
  s_mx[t] = m;
  s_key[t] = key;
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if (t < o) {
      s_mx[t] = fmaxf(s_mx[t], s_mx[t + o]);
      s_key[t] = s_key[t + o] > s_key[t] ? s_key[t + o] : s_key[t];
    }
    __syncthreads();
  }
  const double M = (double)s_mx[0];
  double sum = 0.0;
  for (int i = t; i < n; i += 1024) sum += exp((double)x[i] - M);
  sh[t] = sum;
  __syncthreads();
  for (int o = 512; o >= 1; o >>= 1) {
    if (t < o) sh[t] = sh[t] + sh[t + o];
    __syncthreads();
  }
  if (t == 0) {
    const double l = M + log(sh[0]);
    if (lse) *lse = (float)l;
    if (logprob) *logprob = target >= 0 ? (float)((double)x[target] - l) : 0.0f;
    if (argmax) *argmax = s_key[0] ? (int32_t)argmax_key_index(s_key[0]) : 0;
  }
}

}  // namespace

void launch_score_rows(const ScoreArgs& a, hipStream_t s) {
  const ScorePlan p = score_plan(a.T, a.V, a.E);
  if (!p.ok || a.xstride < a.E || a.xstride % 8 != 0) throw std::runtime_error("score_rows: T, V >= 1 and E % 16 == 0");
  if (!a.x16 || !a.w16 || !a.ms || !a.key || !a.tl) throw std::runtime_error("score_rows: null buffer");
  hipLaunchKernelGGL(score_partials_kernel, dim3(p.n_vtiles), dim3(256), 0, s, a, p.n_vtiles);
  LLMI_HIP(hipGetLastError());
  hipLaunchKernelGGL(score_merge_kernel, dim3(a.T), dim3(256), 0, s, a, p.n_vtiles);
  LLMI_HIP(hipGetLastError());
}

void launch_score_reduce_row(const float* logits, int V, int target, float* logprob, float* lse, int32_t* argmax,
                             hipStream_t s) {
  if (V < 1 || target >= V) throw std::runtime_error("score_reduce_row: target outside the row");
  hipLaunchKernelGGL(score_reduce_row_kernel, dim3(1), dim3(1024), 0, s, logits, V, target, logprob, lse, argmax);
  LLMI_HIP(hipGetLastError());
}

}  // namespace llmi
