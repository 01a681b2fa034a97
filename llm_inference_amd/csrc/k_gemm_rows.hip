// k_gemm_rows.hip -- the skinny f16 x Q4_0 GEMM: 1 <= T <= 64 token rows, and below it the
// skinny int8 GEMM for Q8_0 / Q4_0 weights: 1 <= T <= 32 (section 18).
//
//   out[t][n] = tscale[t] * (p_0 + p_1 (+ p_2 + p_3)),   p_g = sum over blocks b = g, g + WK, ... (ascending)
//
// with the bits of prefill_gemm6_kernel (k_prefill.hip, WQ == 0): the weight f16((1024 + q) - 1032) * d in f16
// arithmetic (one rounding), two v_mfma_f32_32x32x16_f16 steps per Q4_0 block (the low nibbles = elements 0..15,
// then the high = 16..31; lane half h supplies elements 8h .. 8h + 7 of the sixteen to both operands, weight rows
// in A, tokens in B), WK = 4 for nb >= 160 else 2, every partial carried through one MFMA accumulator from 0, the
// partials added left to right in f32.  Which wave computes an output is free, and that is all this kernel changes.
//
// A batch step is a stream of weights with a few token rows beside it, so the kernel is built as the row-bound GEMV
// is, not as a tiled GEMM:
//  * Weights go from global memory straight to registers.  A wave owns (RW rows, one K group): every weight byte is
//    consumed by exactly one wave, so there is no LDS ring and no barrier on the weight stream.  The lane (r, h)
//    needs bytes 8h .. 8h + 7 of its row's block; the two lane halves instead load the whole 16 B of two
//    consecutive blocks of the group (a "pair": blocks b0 and b0 + WK) and exchange halves with two
//    v_permlane32_swap, a third hands both halves both f16 scales: one 16-B and one 2-B load per lane and pair.
//  * NS register stages of PPC pairs each; stage c + NS - 1 is issued before stage c is consumed.
//  * The T live activation rows wait in LDS in chunks of CB blocks (one stage of every K group), double-buffered,
//    one barrier per chunk; rows are CB x 64 + 16 B apart, which spreads the 16-B fragment reads of 16 token rows
//    over all 64 banks.  A chunk is loaded one step ahead into registers, *before* that step's weight stage, so
//    the wait for it leaves the younger weight stages in flight.
//  * 33..64 rows: a second token tile (accumulator) reuses the dequantized A fragments; its chunks are half as long.
//  * RW = 16: the wave fills half of its MFMA tile's rows (the rest are zero) -- twice the waves, and so twice the
//    loads in flight, for the narrow projections (4B o / down: 80 row tiles).
//  * Epilogue as v6's: the waves' tiles to LDS, the K groups summed in group order, row-contiguous stores.
#include <type_traits>

#include "session_kernels.h"

namespace llmi {

namespace {

typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<N, I + 1>(f);
  }
}

__device__ __forceinline__ size_t q4_block_index(int slab, int rows, int nb, int n, int b) {
  return slab ? ((size_t)(b >> 3) * rows + n) * 8 + (b & 7) : (size_t)n * nb + b;
}

// lanes 32..63 of a <-> lanes 0..31 of b
__device__ __forceinline__ void swap32(uint32_t& a, uint32_t& b) {
  const auto v = __builtin_amdgcn_permlane32_swap(a, b, false, false);
  a = v[0];
  b = v[1];
}

template <int NTT, int RW, int WR, int WK, int NS>
struct GR {
  static constexpr int NW = WR * WK, NTH = 64 * NW, MR = WR * RW;
  static constexpr int CB = NTT == 1 ? 16 : 8;  // blocks per activation chunk
  static constexpr int PPC = CB / (2 * WK);     // block pairs per wave and chunk
  static constexpr int XROW = CB * 64 + 16;     // bytes between token rows in LDS
  static constexpr int XU = (32 * NTT * CB * 4 + NTH - 1) / NTH;  // 16-B activation units per thread and chunk
  static constexpr int EPI = NW * 32 * 33 * 4;
  static_assert(PPC >= 1 && (RW == 32 || RW == 16) && NS >= 2, "geometry");
  static size_t lds(int T) {
    const size_t x = 2 * (size_t)T * XROW;
    return x > (size_t)EPI ? x : (size_t)EPI;
  }
};

template <int NTT, int RW, int WR, int WK, int NS>
__global__ __launch_bounds__(64 * WR * WK) void gemm_rows_kernel(PrefillGemm16 a) {
  using C = GR<NTT, RW, WR, WK, NS>;
  constexpr int CB = C::CB, PPC = C::PPC;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
  const int kg = w % WK, wr = w / WK;
  const int nb = a.nb, T = a.T, nc = (nb + CB - 1) / CB;
  const int nbase = blockIdx.x * C::MR;
  const bool live = r < RW;
  const int n = nbase + wr * RW + (r & (RW - 1));  // (the idle lanes of a half tile reload a live row: in bounds)
  const size_t xbuf = (size_t)T * C::XROW;
  const uint4* __restrict__ qs = a.qs;
  const uint16_t* __restrict__ wds = a.wd;
  const uint16_t* __restrict__ x = a.x;
  const int slab = a.slab, rows = a.rows, xstride = a.xstride;

  uint4 wq[NS][PPC];
  uint32_t wd[NS][PPC];
  auto issue_w = [&](int c, auto slot) __attribute__((always_inline)) {  // chunk c's pairs of this wave: lane half h loads block b0 + WK h
    constexpr int sl = decltype(slot)::value;
    static_for<PPC>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      const int b0 = c * CB + kg + 2 * WK * p;
      int b = b0 + WK * h;
      if (b >= nb) b = b0 < nb ? b0 : kg;  // past the end (not consumed): any block of the row
      const size_t idx = q4_block_index(slab, rows, nb, n, b);
      wq[sl][p] = qs[idx];
      wd[sl][p] = wds[idx];
    });
  };
  u32x4 xr[C::XU];
  auto load_x = [&](int c) __attribute__((always_inline)) {  // unit u: 16 B number u % (4 CB) of token row u / (4 CB)
    static_for<C::XU>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int u = t + i * C::NTH, row = u / (CB * 4), un = c * CB * 4 + u % (CB * 4);
      if (row < T && un < nb * 4) xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)row * xstride + (size_t)un * 8);
    });
  };
  auto store_x = [&](int c) __attribute__((always_inline)) {
    unsigned char* xb = s_mem + (c & 1) * xbuf;
    static_for<C::XU>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int u = t + i * C::NTH, row = u / (CB * 4), un = u % (CB * 4);
      if (row < T && c * CB * 4 + un < nb * 4) *reinterpret_cast<u32x4*>(xb + (size_t)row * C::XROW + un * 16) = xr[i];
    });
  };

  v16f acc[NTT];
  int trow[NTT];
#pragma unroll
  for (int j = 0; j < NTT; j++) {
    acc[j] = v16f{};
    trow[j] = min(32 * j + r, T - 1) * C::XROW + 16 * h;  // columns past T repeat the last row (never stored)
  }
  const f16x2v m1032 = {(_Float16)-1032.0f, (_Float16)-1032.0f};
  // one Q4_0 block: q0 / q1 = bytes 8h .. 8h + 7 of the row's block, d its scale, lb its place in the chunk
  auto block = [&](uint32_t q0, uint32_t q1, uint32_t d, const unsigned char* xb, int lb) __attribute__((always_inline)) {
    const f16x2v sc = __builtin_bit_cast(f16x2v, (d & 0xFFFFu) | (d << 16));
    f16x8 A0, A1;
    const uint32_t dw[2] = {q0, q1};
#pragma unroll
    for (int e = 0; e < 2; e++) {
      const uint32_t v = dw[e], vh = v >> 4;
#pragma unroll
      for (int pr = 0; pr < 2; pr++) {  // bytes 2 pr, 2 pr + 1 of the dword = elements 8h + 4e + 2pr, +1
        const uint32_t sel = pr ? 0x0C030C02u : 0x0C010C00u;
        const uint32_t lo = __builtin_amdgcn_perm(0u, v, sel) & 0x000F000Fu;
        const uint32_t hi = __builtin_amdgcn_perm(0u, vh, sel) & 0x000F000Fu;
        const f16x2v fl = (__builtin_bit_cast(f16x2v, lo | 0x64006400u) + m1032) * sc;  // (1024 + q) - 1032, x d
        const f16x2v fh = (__builtin_bit_cast(f16x2v, hi | 0x64006400u) + m1032) * sc;
        A0[4 * e + 2 * pr] = fl[0];
        A0[4 * e + 2 * pr + 1] = fl[1];
        A1[4 * e + 2 * pr] = fh[0];
        A1[4 * e + 2 * pr + 1] = fh[1];
      }
    }
    if (!live) A0 = A1 = f16x8{};
#pragma unroll
    for (int j = 0; j < NTT; j++) {
      const f16x8 B0 = *reinterpret_cast<const f16x8*>(xb + trow[j] + lb * 64);
      const f16x8 B1 = *reinterpret_cast<const f16x8*>(xb + trow[j] + lb * 64 + 32);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A0, B0, acc[j], 0, 0, 0);
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A1, B1, acc[j], 0, 0, 0);
    }
  };
  auto compute = [&](int c, auto slot) __attribute__((always_inline)) {
    constexpr int sl = decltype(slot)::value;
    const unsigned char* xb = s_mem + (c & 1) * xbuf;
    static_for<PPC>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      const int lb = kg + 2 * WK * p, b0 = c * CB + lb;
      if (b0 < nb) {  // (wave-uniform)
        uint32_t q0 = wq[sl][p].x, q1 = wq[sl][p].y, q2 = wq[sl][p].z, q3 = wq[sl][p].w;
        uint32_t d0 = wd[sl][p], d1 = d0;
        swap32(q0, q2);  // q0 q1: this lane's half of block b0; q2 q3: of block b0 + WK
        swap32(q1, q3);
        swap32(d0, d1);  // d0: block b0's scale in both halves; d1: block b0 + WK's
        block(q0, q1, d0, xb, lb);
        if (b0 + WK < nb) block(q2, q3, d1, xb, lb + WK);
      }
    });
  };
  auto lds_barrier = []() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  load_x(0);
  issue_w(0, std::integral_constant<int, 0>{});
  store_x(0);
  if (nc > 1) load_x(1);
  static_for<NS - 2>([&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value + 1;
    if (k < nc) issue_w(k, std::integral_constant<int, k>{});
  });
  lds_barrier();
  for (int c0 = 0; c0 < nc; c0 += NS) {
    static_for<NS>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      const int c = c0 + k;
      if (c < nc) {
        if (c + 1 < nc) store_x(c + 1);  // loaded a step ago, ahead of that step's weight stage
        if (c + 2 < nc) load_x(c + 2);
        if (c + NS - 1 < nc) issue_w(c + NS - 1, std::integral_constant<int, (k + NS - 1) % NS>{});
        __builtin_amdgcn_sched_barrier(0);
        compute(c, kc);
        lds_barrier();
      }
    });
  }
  // every wave's tile (RW rows x 32 tokens) to LDS, then the K groups summed in group order
  float* ep = reinterpret_cast<float*>(s_mem);
#pragma unroll
  for (int j = 0; j < NTT; j++) {
    if (j) __builtin_amdgcn_s_barrier();  // the previous token tile's sums are read
    float* mine = ep + (size_t)w * 32 * 33;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) mine[r * 33 + (reg & 3) + 8 * (reg >> 2) + 4 * h] = acc[j][reg];
    lds_barrier();
    for (int i = t; i < C::MR * 32; i += C::NTH) {
      const int row = i % C::MR, tk = i / C::MR, tok = 32 * j + tk;
      const float* p = ep + (size_t)(row / RW) * WK * 32 * 33 + tk * 33 + row % RW;
      float v = p[0];
#pragma unroll
      for (int g = 1; g < WK; g++) v += p[g * 32 * 33];
      if (tok < T) a.out[(size_t)tok * a.ostride + nbase + row] = a.tscale ? v * a.tscale[tok] : v;
    }
  }
}

template <int NTT, int RW, int WR, int WK, int NS>
bool try_rows(const PrefillGemm16& a, hipStream_t s) {
  using C = GR<NTT, RW, WR, WK, NS>;
  if (a.rows % C::MR) return false;
  auto* k = gemm_rows_kernel<NTT, RW, WR, WK, NS>;
  static const bool attr = [&] {  // (above the 64 KB default at T = 32 and T = 64)
    LLMI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)C::lds(32 * NTT)));
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL(k, dim3(a.rows / C::MR), dim3(C::NTH), C::lds(a.T), s, a);
  return true;
}

// The launch table.  rw: live rows per wave.  32-row waves where they alone fill the chip's 1024 SIMDs (4B gate_up:
// 1280 waves), 16-row waves below that (4B qkv 256 -> 512 waves, o 160 -> 320, down 320 -> 640).  LLMI_GR_RW=16|32
// forces one for A/B (scripts/bench_gemm_rows.py).
template <int NTT>
bool launch_rows(const PrefillGemm16& a, hipStream_t s) {
  const int wk = a.nb >= 160 ? 4 : 2;
  int rw = (a.rows / 32) * wk >= 1024 ? 32 : 16;
  if (const char* f = getenv("LLMI_GR_RW")) rw = atoi(f) == 32 ? 32 : 16;
  if (wk == 4) return rw == 32 ? try_rows<NTT, 32, 2, 4, 3>(a, s) : try_rows<NTT, 16, 2, 4, 3>(a, s);
  if (rw == 32) return try_rows<NTT, 32, 4, 2, 3>(a, s) || try_rows<NTT, 32, 2, 2, 3>(a, s);
  return try_rows<NTT, 16, 4, 2, 3>(a, s);
}

// ---------------------------------------------------------------------------
// The int8 form: Q8_0 activation blocks times Q8_0 (W8) or Q4_0 (W4) weights, 1 <= T <= 32.
//
//   out[t][n] = (p_0 + p_1 (+ p_2 + p_3)) (x 1/16: W4),   p_g: acc = fmaf(d_w d_x, (float)isum_b, acc) from +0 over
//                                                              the blocks b = g, g + WK, ... (ascending)
//
// with the bits of prefill_gemm5_kernel (k_prefill.hip, KQ == 0): isum_b from one v_mfma_i32_32x32x32_i8 per block
// (weight rows in A, tokens in B, lane half h supplies elements 16h .. 16h + 15), the 32 x 32 scale products from
// v5's own instruction -- v_mfma_f32_32x32x16_f16 with k = 0 alone, so there is no second way of forming d_w d_x
// whose rounding (or handling of subnormal f16 scales) would have to be shown equal -- WK = 4 for nb >= 160 else 2,
// the partials added left to right; W4's A fragment is 16 (n - 8) and the 16 is undone once per output.
//
// The frame is the f16 kernel's: a wave owns (RW rows, one K group), weights go from global memory to registers in
// NS stages of BPS blocks, the T activation rows wait in LDS in double-buffered chunks (one stage of every K group)
// with one barrier per chunk.  What differs:
//  * W8: lane (r, h) loads the 16-B half h of its row's block -- the A fragment as it lies, nothing to unpack.
//  * W4: both lane halves need all 16 B of a block (each takes one nibble of every byte), so the halves load two
//    consecutive blocks of the group and four v_permlane32_swap (and one for the scales) hand each half both
//    blocks: one 16-B and one 2-B load per lane and block pair.
//  * An XBlock is 48 B (q[32], d, nsum8, pad) and travels whole: the B fragment is its part h, d_x the dword at
//    byte 32.  Rows are CB x 48 + 16 B apart -- an odd multiple of 16 B, so the 16-B reads of 16 token rows fall on
//    16 different slots of the 256 B the banks span.
//  * Per block the matrix pipe gives D (i32) and S (f32 scale products); the VALU's 16 conversions and 16 FMAs of
//    block b - 1 run beside block b's MFMAs (ping-pong result registers, as v5).  A stage's tail blocks past the
//    row's end put zeros in their slot: fmaf(+0, +0, acc) leaves acc as it is (acc is never -0).
// ---------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

template <bool W8, int RW, int WR, int WK, int NS>
struct GI {
  static constexpr int NW = WR * WK, NTH = 64 * NW, MR = WR * RW;
  static constexpr int BPS = 4;                        // blocks per wave and stage
  static constexpr int LPS = W8 ? BPS : BPS / 2;       // 16-B weight loads per lane and stage
  static constexpr int CB = BPS * WK;                  // blocks per activation chunk
  static constexpr int XROW = CB * 48 + 16;            // bytes between token rows in LDS
  static constexpr int XU = (32 * CB * 3 + NTH - 1) / NTH;  // 16-B activation units per thread and chunk
  static constexpr int EPI = NW * 32 * 33 * 4;
  static_assert((RW == 32 || RW == 16) && NS >= 2 && BPS % 2 == 0 && (XROW / 16) % 2 == 1, "geometry");
  static_assert(2 * 32 * XROW <= 65536 && EPI <= 65536, "LDS within the default limit");
  static size_t lds(int T) {
    const size_t x = 2 * (size_t)T * XROW;
    return x > (size_t)EPI ? x : (size_t)EPI;
  }
};

template <bool W8, int RW, int WR, int WK, int NS>
__global__ __launch_bounds__(64 * WR * WK) void gemm_rows_i8_kernel(PrefillGemm a) {
  using C = GI<W8, RW, WR, WK, NS>;
  constexpr int BPS = C::BPS, LPS = C::LPS, CB = C::CB;
  extern __shared__ __attribute__((aligned(16))) unsigned char s_mem[];
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), r = lane & 31, h = lane >> 5;
  const int kg = w % WK, wr = w / WK;
  const int nb = a.nb, T = a.T, nbw = nb / WK, nc = (nbw + BPS - 1) / BPS;  // nbw: this wave's blocks (nb % 4 == 0)
  const int nbase = blockIdx.x * C::MR;
  const bool live = r < RW;
  const int n = nbase + wr * RW + (r & (RW - 1));  // (the idle lanes of a half tile reload a live row: in bounds)
  const size_t xbuf = (size_t)T * C::XROW;
  const uint4* __restrict__ qs = a.qs;
  const uint16_t* __restrict__ wds = a.wd;
  const unsigned char* __restrict__ x = reinterpret_cast<const unsigned char*>(a.x);
  const size_t xpitch = (size_t)a.xstride * sizeof(XBlock);
  const int slab = a.slab, rows = a.rows;

  uint4 wq[NS][LPS];
  uint32_t wd[NS][LPS];
  auto issue_w = [&](int c, auto slot) __attribute__((always_inline)) {  // stage c: blocks kg + WK (c BPS + 0 .. BPS - 1)
    constexpr int sl = decltype(slot)::value;
    static_for<LPS>([&](auto pc) __attribute__((always_inline)) {
      constexpr int p = decltype(pc)::value;
      int i = c * BPS + (W8 ? p : 2 * p + h);  // W4: lane half h loads the pair's block h
      if (i >= nbw) i = nbw - 1;               // past the end (not consumed): a block of the row
      const int b = kg + WK * i;
      if constexpr (W8) {
        const size_t idx = (size_t)n * nb + b;
        wq[sl][p] = qs[idx * 2 + h];
        wd[sl][p] = wds[idx];
      } else {
        const size_t idx = q4_block_index(slab, rows, nb, n, b);
        wq[sl][p] = qs[idx];
        wd[sl][p] = wds[idx];
      }
    });
  };
  u32x4 xr[C::XU];
  auto load_x = [&](int c) __attribute__((always_inline)) {  // unit u: 16 B number u % (3 CB) of token row u / (3 CB)
    static_for<C::XU>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int u = t + i * C::NTH, row = u / (CB * 3), un = u % (CB * 3);
      if (row < T && c * CB + un / 3 < nb)
        xr[i] = *reinterpret_cast<const u32x4*>(x + (size_t)row * xpitch + ((size_t)c * CB * 3 + un) * 16);
    });
  };
  auto store_x = [&](int c) __attribute__((always_inline)) {
    unsigned char* xb = s_mem + (c & 1) * xbuf;
    static_for<C::XU>([&](auto ic) __attribute__((always_inline)) {
      constexpr int i = decltype(ic)::value;
      const int u = t + i * C::NTH, row = u / (CB * 3), un = u % (CB * 3);
      if (row < T && c * CB + un / 3 < nb) *reinterpret_cast<u32x4*>(xb + (size_t)row * C::XROW + un * 16) = xr[i];
    });
  };

  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = 0.0f;
  const v16i zero = {};
  const v16f zerof = {};
  v16i Dr[2];  // results of two blocks in flight, ping-pong by the block's parity in its stage (BPS is even)
  v16f Sr[2];
  Dr[1] = zero;
  Sr[1] = zerof;  // fmaf(+0, +0, acc) leaves acc unchanged
  auto epi = [&](auto sl) __attribute__((always_inline)) {
    constexpr int S = decltype(sl)::value;
#pragma unroll
    for (int reg = 0; reg < 16; reg++) acc[reg] = fmaf(Sr[S][reg], (float)Dr[S][reg], acc[reg]);
    // pins the FMAs here, beside the MFMAs issued just before them: left free, they sink past the stage's end and
    // every block of the stage keeps its result registers until then
    asm volatile("" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]),
                      "+v"(acc[7]), "+v"(acc[8]), "+v"(acc[9]), "+v"(acc[10]), "+v"(acc[11]), "+v"(acc[12]),
                      "+v"(acc[13]), "+v"(acc[14]), "+v"(acc[15]));
  };
  const int trow = min(r, T - 1) * C::XROW;  // columns past T repeat the last row (never stored)
  const uint32_t lsh = 4u - 4u * h;           // W4: the lane half's nibble to the byte's top
  auto compute = [&](int c, auto slot) __attribute__((always_inline)) {
    constexpr int sl = decltype(slot)::value;
    const unsigned char* xb = s_mem + (c & 1) * xbuf + trow;
    uint32_t Aq[BPS][4], Ad[BPS];
    if constexpr (W8) {
      static_for<BPS>([&](auto jc) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        Aq[j][0] = wq[sl][j].x, Aq[j][1] = wq[sl][j].y, Aq[j][2] = wq[sl][j].z, Aq[j][3] = wq[sl][j].w;
        Ad[j] = wd[sl][j];
      });
    } else {
      static_for<LPS>([&](auto pc) __attribute__((always_inline)) {
        constexpr int p = decltype(pc)::value;
        const uint32_t q4[4] = {wq[sl][p].x, wq[sl][p].y, wq[sl][p].z, wq[sl][p].w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          uint32_t q0 = q4[e], q1 = q4[e];
          swap32(q0, q1);  // q0: the pair's first block in both halves; q1: its second
          Aq[2 * p][e] = q0;
          Aq[2 * p + 1][e] = q1;
        }
        uint32_t d0 = wd[sl][p], d1 = d0;
        swap32(d0, d1);
        Ad[2 * p] = d0;
        Ad[2 * p + 1] = d1;
      });
    }
    v4i Bq[BPS];
    float Bd[BPS];
    static_for<BPS>([&](auto jc) __attribute__((always_inline)) {  // the stage's B fragments and d_x, ahead of its MFMAs
      constexpr int j = decltype(jc)::value;
      const unsigned char* xp = xb + (kg + WK * j) * 48;
      Bq[j] = *reinterpret_cast<const v4i*>(xp + 16 * h);
      Bd[j] = *reinterpret_cast<const float*>(xp + 32);
    });
    __builtin_amdgcn_sched_barrier(0);
    static_for<BPS>([&](auto jc) __attribute__((always_inline)) {
      constexpr int j = decltype(jc)::value, ps = j & 1;
      // a block past the row's end (the last stage's tail; wave-uniform) multiplies with both scales +0: S = +0 and
      // fmaf(+0, D, acc) = acc for any integer D
      const bool on = !h && c * BPS + j < nbw;
      v4i A;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const uint32_t v = W8 ? Aq[j][e] : ((Aq[j][e] << lsh) & 0xF0F0F0F0u) ^ 0x80808080u;  // W4: 16 (n - 8)
        A[e] = (int)(RW == 32 || live ? v : 0u);
      }
      f16x8 As = {}, Bs = {};
      As[0] = __builtin_bit_cast(_Float16, (uint16_t)(on && live ? Ad[j] & 0xFFFFu : 0u));
      Bs[0] = on ? (_Float16)Bd[j] : (_Float16)0.0f;  // d_x holds an f16 value: exact
      Dr[ps] = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, Bq[j], zero, 0, 0, 0);
      Sr[ps] = __builtin_amdgcn_mfma_f32_32x32x16_f16(As, Bs, zerof, 0, 0, 0);
      epi(std::integral_constant<int, ps ^ 1>{});  // the previous block's results, beside this block's MFMAs
      __builtin_amdgcn_sched_barrier(0);             // (keeps the blocks in order: two result sets live, not BPS)
    });
  };
  auto lds_barrier = []() __attribute__((always_inline)) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
  };

  load_x(0);
  issue_w(0, std::integral_constant<int, 0>{});
  store_x(0);
  if (nc > 1) load_x(1);
  static_for<NS - 2>([&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value + 1;
    if (k < nc) issue_w(k, std::integral_constant<int, k>{});
  });
  lds_barrier();
  for (int c0 = 0; c0 < nc; c0 += NS) {
    static_for<NS>([&](auto kc) __attribute__((always_inline)) {
      constexpr int k = decltype(kc)::value;
      const int c = c0 + k;
      if (c < nc) {
        if (c + 1 < nc) store_x(c + 1);  // loaded a step ago, ahead of that step's weight stage
        if (c + 2 < nc) load_x(c + 2);
        if (c + NS - 1 < nc) issue_w(c + NS - 1, std::integral_constant<int, (k + NS - 1) % NS>{});
        __builtin_amdgcn_sched_barrier(0);
        compute(c, kc);
        lds_barrier();
      }
    });
  }
  epi(std::integral_constant<int, (BPS - 1) & 1>{});  // the last block's results
  // every wave's tile (RW rows x 32 tokens) to LDS, then the K groups summed in group order
  float* ep = reinterpret_cast<float*>(s_mem);
  float* mine = ep + (size_t)w * 32 * 33;
#pragma unroll
  for (int reg = 0; reg < 16; reg++) mine[r * 33 + (reg & 3) + 8 * (reg >> 2) + 4 * h] = acc[reg];
  lds_barrier();
  for (int i = t; i < C::MR * T; i += C::NTH) {
    const int row = i % C::MR, tok = i / C::MR;
    const float* p = ep + (size_t)(row / RW) * WK * 32 * 33 + tok * 33 + row % RW;
    float v = p[0];
#pragma unroll
    for (int g = 1; g < WK; g++) v += p[g * 32 * 33];
    a.out[(size_t)tok * a.ostride + nbase + row] = W8 ? v : v * 0.0625f;  // W4: the 16 of 16 (n - 8)
  }
}

template <bool W8, int RW, int WR, int WK, int NS>
bool try_rows_i8(const PrefillGemm& a, hipStream_t s) {
  using C = GI<W8, RW, WR, WK, NS>;
  if (a.rows % C::MR) return false;
  hipLaunchKernelGGL((gemm_rows_i8_kernel<W8, RW, WR, WK, NS>), dim3(a.rows / C::MR), dim3(C::NTH), C::lds(a.T), s, a);
  return true;
}

// The launch table: the K split from K alone (v5's), eight waves per work-group where the rows allow.  rw as in the
// f16 table: 32-row waves where they alone fill the chip's 1024 SIMDs, 16-row waves below that; a row count that is
// no multiple of the wider work-group's rows takes the next narrower one (every v5 shape has rows % 32 == 0).
template <bool W8>
bool launch_rows_i8(const PrefillGemm& a, hipStream_t s) {
  const int wk = a.nb >= 160 ? 4 : 2;
  int rw = (a.rows / 32) * wk >= 1024 ? 32 : 16;
  if (const char* f = getenv("LLMI_GR_RW")) rw = atoi(f) == 32 ? 32 : 16;
  if (wk == 4) return (rw == 32 && try_rows_i8<W8, 32, 2, 4, 3>(a, s)) || try_rows_i8<W8, 16, 2, 4, 3>(a, s);
  return (rw == 32 && try_rows_i8<W8, 32, 4, 2, 3>(a, s)) || try_rows_i8<W8, 16, 4, 2, 3>(a, s) ||
         try_rows_i8<W8, 16, 2, 2, 3>(a, s);
}

}  // namespace

bool gemm_rows_i8_supported(const DevWeight& w) {
  return (w.type == T_Q8_0 || w.type == T_Q4_0) && prefill_gemm_supported(w);
}

void launch_gemm_rows_i8(const PrefillGemm& a, hipStream_t s) {
  if (a.T < 1 || a.T > GEMM_ROWS_I8_T_MAX) throw std::runtime_error("gemm_rows_i8: T outside 1..32");
  if (a.kq || a.rows % 32 || a.nb % 4 || (a.slab && (a.w8 || a.nb % 8))) throw std::runtime_error("gemm_rows_i8: shape");
  if (!(a.w8 ? launch_rows_i8<true>(a, s) : launch_rows_i8<false>(a, s))) throw std::runtime_error("gemm_rows_i8: shape");
  LLMI_HIP(hipGetLastError());
}

bool gemm_rows_supported(const DevWeight& w) { return w.type == T_Q4_0 && prefill_gemm16_supported(w); }

void launch_gemm_rows(const PrefillGemm16& a, hipStream_t s) {
  if (a.T < 1 || a.T > GEMM_ROWS_T_MAX) throw std::runtime_error("gemm_rows: T outside 1..64");
  if (a.rows % 64 || a.nb % 4 || a.xstride % 8 || (a.slab && a.nb % 8))
    throw std::runtime_error("gemm_rows: shape");
  const bool ok = a.T <= 32 ? launch_rows<1>(a, s) : launch_rows<2>(a, s);
  if (!ok) throw std::runtime_error("gemm_rows: shape");
  LLMI_HIP(hipGetLastError());
}

}  // namespace llmi
