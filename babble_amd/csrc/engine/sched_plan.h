// sched_plan.h -- the pure arithmetic of DivideRounds' host scheduling
// (rounds.cpp, split.cpp): no HIP, no handle, so a plain host program checks
// it (tests/cpp/sched_plan_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

namespace bh {

// Segment boundaries of a K-segment pipeline over events [base, N): Ns[0] =
// base, Ns[K] = N (K clamped to 64), segment k holding a ratio^k share: a
// short first segment (the pipeline's fill is its dataflow: the loop waits
// for its coordinates only) and segments growing about as fast as the loop
// outruns the dataflow (seg_ratio, rounds.cpp, picks the ratio and says why)
inline void segment_bounds(int64_t base, int64_t N, int K, double ratio, int64_t *Ns) {
  Ns[0] = base;
  if (K <= 1) { Ns[1] = N; return; }
  double w[64], tot = 0;
  K = std::min(K, 64);
  for (int k = 0; k < K; ++k) tot += (w[k] = std::pow(ratio, k));
  double acc = 0;
  for (int k = 1; k < K; ++k) {
    acc += w[k - 1];
    // at least one event per segment (segments_for keeps >= 4096 per segment on average)
    Ns[k] = std::max(Ns[k - 1] + 1, base + (int64_t)((double)(N - base) * acc / tot));
  }
  Ns[K] = N;
}

// The 64-row tiles holding the rows [cstart[c] + lo[c], cstart[c] + hi[c])
// of every chain c (the transpose's work list): ascending, in layout order
// (cstart ascends with c), a tile shared by two chains' runs once.  Returns
// their number; out has room for every tile of the layout.
inline int64_t tile_list(int n, const int32_t *cstart, const int32_t *lo, const int32_t *hi, int32_t *out) {
  int64_t nt = 0;
  for (int c = 0; c < n; ++c) {
    if (hi[c] <= lo[c]) continue;
    const int64_t a = ((int64_t)cstart[c] + lo[c]) >> 6, b = ((int64_t)cstart[c] + hi[c] - 1) >> 6;
    for (int64_t t = (nt && out[nt - 1] >= a) ? out[nt - 1] + 1 : a; t <= b; ++t) out[nt++] = (int32_t)t;
  }
  return nt;
}

// The round an incremental call resumes at: the last round whose boundaries
// lie inside the previous prefix on every chain the call extends (rq[c]:
// chain c's first round outside it, k_resume_point), never below r0.
inline int32_t resume_round(int n, const int32_t *rq, const int32_t *old_len, const int32_t *new_len, int32_t r0) {
  int32_t m = INT32_MAX;
  for (int c = 0; c < n; ++c)
    if (new_len[c] > old_len[c]) m = std::min(m, rq[c]);
  return std::max(r0, m == INT32_MAX ? r0 : m - 1);
}

}  // namespace bh
