// k_score_top.hip -- the N most likely ids of every scored position with their log-probs (llmi_session_score_top /
// llmi_score_rows_top).  Runs after k_score.hip's merge; the T x V logits still never exist.
//
// score_top_kernel, one work-group (4 waves) per token:
//  * Tile pick.  The scorer left one argmax_key per (token, 128-row vocabulary tile).  Keys are distinct (value,
//    then lower id), so every one of the token's N largest logits lies in one of the N tiles with the largest
//    tile keys (an element outside them has N tile maxima above it).  The token's n_vt keys go to LDS and the
//    min(N, n_vt) largest are taken in rounds: round j is the block maximum below round j - 1's.
//  * Rescore.  The token's f16 row is staged once in LDS.  Per picked tile, wave w recomputes rows 32 w .. + 31 on
//    v_mfma_f32_32x32x16_f16 with the scorer's chain: A = the table row (lane (r, h): 16-B unit 2 ks + h), B = the
//    token row's same unit in every column, accumulator from 0, k ascending 16 at a time, units past E zero, and
//    on through the zero-padded steps of the last 64-k stage.  An MFMA output depends only on its A row, its B
//    column and the k order, so each logit carries the scorer's bits.  A-fragments go from global memory straight
//    to registers (every table byte has one consumer, so no LDS ring), the next ST_KD k steps' loads in flight
//    behind the current MFMAs.  All 32 columns are equal; lane r < 16 keeps accumulator element r.
//  * Select.  The n_pick x 128 candidate keys (soft-capped as the scorer caps, rows past V absent) overwrite the
//    tile keys in LDS and the N largest come out in the same rounds, in key order: slot j gets the id and
//    (float)((double)logit - lse64[tok]), the merge's own expression for the target's log-prob.
// score_top_row_kernel (row path): the same rule over one f32 logits row, segments in place of tiles.
// Plain vector stores only, no atomics.
#include "kernels.h"
#include "score_plan.h"

namespace llmi {

namespace {

typedef _Float16 st_f16x8 __attribute__((ext_vector_type(8)));
typedef float st_v16f __attribute__((ext_vector_type(16)));
typedef unsigned long long st_u64;

constexpr int ST_KD = 8;  // k steps (16-B loads per lane) in flight per wave: 8 KB

__device__ __forceinline__ st_u64 st_shfl_xor_u64(st_u64 v, int m) {
  const unsigned lo = __shfl_xor((unsigned)v, m), hi = __shfl_xor((unsigned)(v >> 32), m);
  return ((st_u64)hi << 32) | lo;
}

// the float an argmax_key was made from (common.h: negative values were complemented, the others got the top bit)
__device__ __forceinline__ float st_key_value(st_u64 k) {
  const uint32_t u = (uint32_t)(k >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// The N largest of the distinct keys key_at(0 .. n) (0: absent) into out[0 .. N), descending; slots past the number
// of keys present get 0.  Round j is the block maximum below round j - 1's result: nothing is removed, so key_at may
// read LDS or global memory that stays as it is.  NT threads; red alternates by round, which leaves one barrier per
// round (a thread writes red[j & 1] again only after the barrier of round j + 1, which every thread reaches after
// its reads of round j).  Ends with a barrier: out is readable, and whatever key_at read may be overwritten.
template <int NT, typename F>
__device__ __forceinline__ void st_top_rounds(F key_at, int n, int N, st_u64* out, st_u64 (*red)[NT / 64]) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  st_u64 bound = ~0ull;
  for (int j = 0; j < N; j++) {
    st_u64 best = 0;
    for (int i = t; i < n; i += NT) {
      const st_u64 k = key_at(i);
      if (k < bound && k > best) best = k;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const st_u64 o = st_shfl_xor_u64(best, m);
      best = o > best ? o : best;
    }
    if (lane == 0) red[j & 1][w] = best;
    __syncthreads();
    best = red[j & 1][0];
#pragma unroll
    for (int q = 1; q < NT / 64; q++) best = red[j & 1][q] > best ? red[j & 1][q] : best;
    if (t == 0) out[j] = best;
    bound = best;
  }
  __syncthreads();
}

__device__ __forceinline__ void st_store(st_u64 k, double lse, int32_t* id, float* lp) {
  *id = k ? (int32_t)argmax_key_index(k) : 0;
  *lp = (float)((double)st_key_value(k) - lse);
}

__global__ __launch_bounds__(256) void score_top_kernel(ScoreArgs a, int n_vt, int n_pick, int n_ksteps, int key_off) {
  extern __shared__ __attribute__((aligned(16))) unsigned char st_lds[];
  __shared__ st_u64 s_red[2][4], s_sel[SCORE_TOP_MAX];
  __shared__ int s_pick[SCORE_TOP_MAX];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
  const int tok = blockIdx.x, E = a.E, N = a.top_n;
  u32x4_t* s_x = reinterpret_cast<u32x4_t*>(st_lds);           // the token's row: E / 8 units of 16 B
  st_u64* s_key = reinterpret_cast<st_u64*>(st_lds + key_off);  // tile keys, then the candidates

  const uint16_t* xrow = a.x16 + (size_t)tok * a.xstride;
  for (int u = t; u < E / 8; u += 256) s_x[u] = *reinterpret_cast<const u32x4_t*>(xrow + u * 8);
  const st_u64* keys = a.key + (size_t)tok * n_vt;
  for (int i = t; i < n_vt; i += 256) s_key[i] = keys[i];
  __syncthreads();

  // ---- tile pick
  st_top_rounds<256>([&](int i) { return s_key[i]; }, n_vt, n_pick, s_sel, s_red);
  if (t < n_pick) s_pick[t] = (int)min(argmax_key_index(s_sel[t]) / SCORE_VT, (uint32_t)n_vt - 1);
  __syncthreads();

  // ---- rescore: the candidates replace the tile keys
  const u32x4_t zero4 = {0u, 0u, 0u, 0u};
  for (int p = 0; p < n_pick; p++) {
    const int v0 = s_pick[p] * SCORE_VT;
    const uint16_t* wrow = a.w16 + (size_t)min(v0 + 32 * w + r, a.V - 1) * E;  // (rows past V: masked below)
    u32x4_t cur[ST_KD], nxt[ST_KD];
    auto load = [&](u32x4_t* d, int c) {
#pragma unroll
      for (int q = 0; q < ST_KD; q++) {
        const int u = 2 * (c * ST_KD + q) + h;  // E % 8 == 0: a unit is inside or outside as a whole
        d[q] = u * 8 < E ? *reinterpret_cast<const u32x4_t*>(wrow + u * 8) : zero4;
      }
    };
    st_v16f acc = st_v16f{};
    load(cur, 0);
    for (int c = 0; c * ST_KD < n_ksteps; c++) {
      load(nxt, c + 1);  // (units past the chain's end are past E: zeros, no access)
#pragma unroll
      for (int q = 0; q < ST_KD; q++) {
        const int ks = c * ST_KD + q, u = 2 * ks + h;
        if (ks < n_ksteps) {  // (uniform) the chain ends with the scorer's last stage, zero-padded steps included
          const u32x4_t b = u * 8 < E ? s_x[u] : zero4;
          acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(st_f16x8, cur[q]),
                                                       __builtin_bit_cast(st_f16x8, b), acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int q = 0; q < ST_KD; q++) cur[q] = nxt[q];
    }
    // acc[i] = logit of tile row 32 w + 8 (i >> 2) + 4 h + (i & 3), the same in every column r
    float l = acc[0];
#pragma unroll
    for (int i = 1; i < 16; i++) l = r == i ? acc[i] : l;
    if (r < 16) {
      const int lr = 32 * w + 8 * (r >> 2) + 4 * h + (r & 3), row = v0 + lr;
      if (a.softcap > 0.0f) l = a.softcap * llmi_glibc::tanhf(l / a.softcap);  // k_score.hip's expression
      s_key[p * SCORE_VT + lr] = row < a.V ? argmax_key(l, (uint32_t)row) : 0ull;
    }
  }
  __syncthreads();

  // ---- select
  st_top_rounds<256>([&](int i) { return s_key[i]; }, n_pick * SCORE_VT, N, s_sel, s_red);
  if (t < N) st_store(s_sel[t], a.lse64[tok], a.top_id + (size_t)tok * N + t, a.top_lp + (size_t)tok * N + t);
}

// Row path: one f32 logits row of n (forward's, after the soft-cap).  Thread t owns the contiguous segment
// [t seg, (t + 1) seg); the N segments with the largest maxima hold the N largest logits (the tile argument).
__global__ __launch_bounds__(1024) void score_top_row_kernel(const float* __restrict__ x, int n, int N,
                                                             const double* __restrict__ lse64, int32_t* top_id,
                                                             float* top_lp) {
  __shared__ st_u64 s_seg[1024], s_red[2][16], s_sel[SCORE_TOP_MAX];
  __shared__ int s_pick[SCORE_TOP_MAX];
  const int t = threadIdx.x;
  const int seg = (n + 1023) / 1024, n_seg = (n + seg - 1) / seg, n_pick = min(N, n_seg);
  auto key_of = [&](long long i) { return i < n ? argmax_key(x[i], (uint32_t)i) : 0ull; };
  st_u64 best = 0;
  for (int e = 0; e < seg; e++) {
    const st_u64 k = key_of((long long)t * seg + e);
    best = k > best ? k : best;
  }
  s_seg[t] = best;  // (0 for a segment past the row)
  __syncthreads();
  st_top_rounds<1024>([&](int i) { return s_seg[i]; }, 1024, n_pick, s_sel, s_red);
  if (t < n_pick) s_pick[t] = (int)min(argmax_key_index(s_sel[t]) / (uint32_t)seg, (uint32_t)n_seg - 1);
  __syncthreads();
  st_top_rounds<1024>([&](int c) { return key_of((long long)s_pick[c / seg] * seg + c % seg); }, n_pick * seg, N, s_sel,
                      s_red);
  if (t < N) st_store(s_sel[t], *lse64, top_id + t, top_lp + t);
}

}  // namespace

void launch_score_top(const ScoreArgs& a, hipStream_t s) {
  const ScoreTopPlan q = score_top_plan(score_plan(a.T, a.V, a.E), a.top_n);
  if (!q.ok) throw std::runtime_error("score_top: top_n outside 1 .. min(32, V), or the vocabulary too large");
  if (a.xstride < a.E || a.xstride % 8 != 0) throw std::runtime_error("score_top: row stride");
  if (!a.x16 || !a.w16 || !a.key || !a.lse64 || !a.top_id || !a.top_lp) throw std::runtime_error("score_top: null buffer");
  const ScorePlan p = score_plan(a.T, a.V, a.E);
  hipLaunchKernelGGL(score_top_kernel, dim3(a.T), dim3(256), q.lds_bytes, s, a, p.n_vtiles, q.n_pick, q.n_ksteps,
                     (int)q.key_off);
  LLMI_HIP(hipGetLastError());
}

void launch_score_top_row(const float* logits, int V, int top_n, const double* lse64, int32_t* top_id, float* top_lp,
                          hipStream_t s) {
  if (V < 1 || top_n < 1 || top_n > SCORE_TOP_MAX || top_n > V) throw std::runtime_error("score_top_row: top_n outside 1 .. min(32, V)");
  if (!logits || !lse64 || !top_id || !top_lp) throw std::runtime_error("score_top_row: null buffer");
  hipLaunchKernelGGL(score_top_row_kernel, dim3(1), dim3(1024), 0, s, logits, V, top_n, lse64, top_id, top_lp);
  LLMI_HIP(hipGetLastError());
}

}  // namespace llmi
