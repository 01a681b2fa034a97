// score_plan_check.cpp -- host-only check of the fused scorer's launch planning (llm_inference_amd/csrc/score_plan.h).
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       scripts/dev/score_plan_check.cpp -o /tmp/score_plan_check && /tmp/score_plan_check
//
// For every shape the GPU tests use (and the real 262,208 x 2560 table at 512 tokens) it walks the launch exactly as
// score_partials_kernel indexes it -- per work-group, token tile, stage, thread and unit -- against real host
// buffers of the planned sizes: every table / row load offset is read, every LDS slot and every partial is
// written, so an index past a buffer is an AddressSanitizer report, and the counts are asserted.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../llm_inference_amd/csrc/score_plan.h"

using namespace llmi;

static int sc_slot(int row, int u) { return row * 8 + (u ^ ((row ^ (row >> 1)) & 7)); }

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

static void walk(long long T, long long V, long long E, bool full) {
  const ScorePlan p = score_plan(T, V, E);
  CHECK(p.ok);
  CHECK((long long)(p.n_vtiles - 1) * SCORE_VT + p.v_tail == V && p.v_tail >= 1 && p.v_tail <= SCORE_VT);
  CHECK((long long)(p.n_ttiles - 1) * SCORE_TT + p.t_tail == T && p.t_tail >= 1 && p.t_tail <= SCORE_TT);
  CHECK((long long)(p.n_stages - 1) * SCORE_KS + 8LL * p.k_tail_units == E && p.k_tail_units >= 1 && p.k_tail_units <= 8);
  CHECK(p.x_bytes == (size_t)T * E * 2 && p.w_bytes == (size_t)V * E * 2);
  if (!full) return;  // (the real table: the arithmetic above only)
  std::vector<unsigned short> x((size_t)T * E, 1), w((size_t)V * E, 1);
  std::vector<unsigned char> ms(p.ms_bytes, 0), key(p.key_bytes, 0), lds_w(SCORE_VT * 128), lds_x(SCORE_TT * 128);
  std::vector<float> tl(p.tl_bytes / 4);
  size_t loaded_w = 0, loaded_x = 0, partials = 0;
  for (int vt = 0; vt < p.n_vtiles; vt++) {
    for (int tt = 0; tt < p.n_ttiles; tt++) {
      for (int c = 0; c < p.n_stages; c++) {
        std::vector<int> slot_used(SCORE_VT * 8, 0);
        for (int t = 0; t < 256; t++) {
          const int ku = t & 7;
          const bool in = (long long)c * SCORE_KS + ku * 8 < E;
          for (int u = 0; u < 4; u++) {
            const int row = (u * 256 + t) >> 3;
            CHECK(row < SCORE_VT && row < SCORE_TT);
            const long long vr = score_clamped_row(vt, SCORE_VT, row, V), tr = score_clamped_row(tt, SCORE_TT, row, T);
            const size_t wo = (size_t)vr * E + ku * 8 + (size_t)c * SCORE_KS;
            const size_t xo = (size_t)tr * E + ku * 8 + (size_t)c * SCORE_KS;
            if (in) {
              for (int e = 0; e < 8; e++) {
                loaded_w += w[wo + e];
                loaded_x += x[xo + e];
              }
            }
            const int s = sc_slot(row, ku);
            CHECK(s >= 0 && s < SCORE_VT * 8);
            slot_used[s]++;
            lds_w[(size_t)s * 16 + 15] = 1;
            lds_x[(size_t)s * 16 + 15] = 1;
          }
        }
        for (int s : slot_used) CHECK(s == 1);  // the swizzle is a permutation: every 16-B slot written once
      }
      const int nt = tt + 1 < p.n_ttiles ? SCORE_TT : p.t_tail;
      for (int t = 0; t < nt; t++) {
        const size_t o = ((size_t)tt * SCORE_TT + t) * p.n_vtiles + vt;
        ms[o * 8 + 7]++;
        key[o * 8 + 7]++;
        tl[(size_t)tt * SCORE_TT + t] = 0.0f;
        partials++;
      }
    }
  }
  CHECK(partials == (size_t)T * p.n_vtiles);
  for (size_t o = 0; o < (size_t)T * p.n_vtiles; o++) CHECK(ms[o * 8 + 7] == 1 && key[o * 8 + 7] == 1);
  // every stage of every (vocabulary tile, token tile) loads 128 rows x (its units inside E)
  const size_t per_tile = (size_t)SCORE_VT * E;
  CHECK(loaded_w == per_tile * p.n_vtiles * p.n_ttiles && loaded_x == per_tile * p.n_vtiles * p.n_ttiles);
}

int main() {
  const long long shapes[][3] = {{1, 64, 256},      {31, 129, 256},  {33, 1000, 1152}, {130, 4096, 2560},
                                 {70, 2113, 5376},  {6, 300, 256},   {9, 777, 512},    {12, 1000, 256},
                                 {40, 2048, 1152},  {128, 4096, 2560}, {44, 4096, 2560}, {33, 4096, 2560},
                                 {2, 5, 16},        {129, 129, 48},  {1, 1, 16}};
  for (const auto& s : shapes) walk(s[0], s[1], s[2], true);
  walk(512, 262208, 2560, false);
  // shapes the planner must turn away
  CHECK(!score_plan(0, 10, 16).ok && !score_plan(3, 0, 16).ok && !score_plan(3, 10, 24).ok && !score_plan(3, 10, 0).ok);
  CHECK(!score_plan(3, 10, 1LL << 31).ok && !score_plan(1LL << 31, 10, 16).ok);
  std::puts("score_plan_check OK");
  return 0;
}
