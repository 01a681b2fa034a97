// score_plan.h -- host-side launch planning of the fused scorer (k_score.hip): tile counts, partial-buffer
// sizes and the ragged edges.  Header-only and free of HIP, so a stand-alone host program can run it under the
// sanitizers (scripts/dev/score_plan_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>

namespace llmi {

constexpr int SCORE_VT = 128;  // vocabulary rows per work-group (4 waves x 32)
constexpr int SCORE_TT = 128;  // tokens per pass of a work-group (4 MFMA tiles of 32 per wave)
constexpr int SCORE_KS = 64;   // k per LDS stage (128-B rows)

struct ScorePlan {
  int T = 0, V = 0, E = 0;
  int n_vtiles = 0;   // work-groups of the partials launch; partials per token
  int n_ttiles = 0;   // token passes of every work-group
  int n_stages = 0;   // LDS stages over E (the last may be partial: units past E load as zeros)
  int v_tail = 0;     // rows of the last vocabulary tile (1..SCORE_VT)
  int t_tail = 0;     // tokens of the last token tile (1..SCORE_TT)
  int k_tail_units = 0;  // 16-B units of the last stage (1..8)
  size_t ms_bytes = 0;   // float2 {max, sum exp(l - max)} [T][n_vtiles]
  size_t key_bytes = 0;  // argmax keys [T][n_vtiles]
  size_t tl_bytes = 0;   // target logits [T]
  size_t x_bytes = 0, w_bytes = 0;
  bool ok = false;
};

// T >= 1, V >= 1, E >= 16 and E % 16 == 0; every index the kernels form stays below 2^31 elements per row offset
// (row * E is computed in size_t on the device).
inline ScorePlan score_plan(long long T, long long V, long long E) {
  ScorePlan p;
  if (T < 1 || V < 1 || E < 16 || E % 16 != 0) return p;
  if (T > INT32_MAX || V > INT32_MAX || E > INT32_MAX) return p;
  p.T = (int)T;
  p.V = (int)V;
  p.E = (int)E;
  p.n_vtiles = (int)((V + SCORE_VT - 1) / SCORE_VT);
  p.n_ttiles = (int)((T + SCORE_TT - 1) / SCORE_TT);
  p.n_stages = (int)((E + SCORE_KS - 1) / SCORE_KS);
  p.v_tail = (int)(V - (long long)(p.n_vtiles - 1) * SCORE_VT);
  p.t_tail = (int)(T - (long long)(p.n_ttiles - 1) * SCORE_TT);
  p.k_tail_units = (int)((E - (long long)(p.n_stages - 1) * SCORE_KS) / 8);
  p.ms_bytes = (size_t)T * (size_t)p.n_vtiles * 8;
  p.key_bytes = (size_t)T * (size_t)p.n_vtiles * 8;
  p.tl_bytes = (size_t)T * 4;
  p.x_bytes = (size_t)T * (size_t)E * 2;
  p.w_bytes = (size_t)V * (size_t)E * 2;
  p.ok = true;
  return p;
}

// The global row a tile's local row reads: rows past the edge re-read the last valid row (their results are masked),
// so no load ever leaves the table or the rows.
inline long long score_clamped_row(long long tile, int tile_rows, int local, long long n_rows) {
  const long long r = tile * tile_rows + local;
  return r < n_rows ? r : n_rows - 1;
}

}  // namespace llmi
