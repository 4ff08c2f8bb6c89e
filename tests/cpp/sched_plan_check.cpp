// sched_plan_check -- the pure planning helpers of DivideRounds' host
// scheduling (babble_amd/csrc/engine/sched_plan.h) against brute-force
// restatements.  A plain host program: no device, no engine library.
#include <cstdio>
#include <set>
#include <vector>

#include "../../babble_amd/csrc/engine/sched_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      ++failures;                                        \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                      \
      fprintf(stderr, "\n");                             \
    }                                                    \
  } while (0)

using Vec = std::vector<int32_t>;

// strictly ascending, and the sorted-unique set of (cstart[c] + j) >> 6
static void check_tiles(const char *name, const Vec &cstart, const Vec &lo, const Vec &hi) {
  const int n = (int)cstart.size();
  std::set<int32_t> want;
  for (int c = 0; c < n; ++c)
    for (int32_t j = lo[c]; j < hi[c]; ++j) want.insert((cstart[c] + j) >> 6);
  int64_t rows = 0;
  for (int c = 0; c < n; ++c) rows = std::max<int64_t>(rows, (int64_t)cstart[c] + std::max(hi[c], 0));
  Vec out((size_t)(rows / 64 + 2), -7);
  const int64_t nt = bh::tile_list(n, cstart.data(), lo.data(), hi.data(), out.data());
  CHECK(nt == (int64_t)want.size(), "%s: %lld tiles, want %zu", name, (long long)nt, want.size());
  for (int64_t i = 1; i < nt; ++i) CHECK(out[i] > out[i - 1], "%s: not ascending at %lld", name, (long long)i);
  if (nt == (int64_t)want.size()) CHECK(std::equal(want.begin(), want.end(), out.begin()), "%s: wrong tiles", name);
}

static void tiles() {
  check_tiles("runs meet inside one tile", {0, 100}, {90, 0}, {100, 20});
  check_tiles("run starts on a tile boundary", {0, 128}, {10, 0}, {70, 64});
  check_tiles("run ends on a tile's last row", {0, 192}, {0, 5}, {64, 6});
  check_tiles("two runs meet exactly on a boundary", {0, 64}, {0, 0}, {64, 1});
  check_tiles("empty chain between two", {0, 70, 140}, {3, 5, 0}, {70, 5, 200});
  check_tiles("all chains empty", {0, 64, 128}, {4, 0, 9}, {4, 0, 9});
  check_tiles("one chain, many tiles", {37}, {1000}, {5000});
  // a layout with slack rows, every (lo, hi) of a small chain set
  const Vec cs = {0, 75, 203, 330};
  for (int32_t a = 0; a <= 70; a += 7)
    for (int32_t b = a; b <= 75; b += 5) check_tiles("sweep", cs, {a, 0, a / 2, b}, {b, a, 75, b + 63});
}

static void check_bounds(int64_t base, int64_t N, int K, double ratio) {
  std::vector<int64_t> Ns((size_t)std::max(K, 1) + 1, -1);
  bh::segment_bounds(base, N, K, ratio, Ns.data());
  const int Ke = K <= 1 ? 1 : std::min(K, 64);  // K > 64 is clamped
  CHECK(Ns[0] == base, "Ns[0] %lld != base %lld (K %d)", (long long)Ns[0], (long long)base, K);
  CHECK(Ns[(size_t)Ke] == N, "Ns[K] %lld != N %lld (K %d, ratio %g)", (long long)Ns[(size_t)Ke], (long long)N, K, ratio);
  for (int k = Ke + 1; k <= K; ++k) CHECK(Ns[(size_t)k] == -1, "entry %d past the clamp written", k);
  if (N - base >= Ke)
    for (int k = 0; k < Ke; ++k)
      CHECK(Ns[(size_t)k + 1] > Ns[(size_t)k], "not increasing at %d (base %lld N %lld K %d ratio %g)", k,
            (long long)base, (long long)N, K, ratio);
  // brute force: the boundary before segment k is the ratio^j shares below it
  double tot = 0;
  for (int k = 0; k < Ke; ++k) tot += std::pow(ratio, k);
  double acc = 0;
  int64_t prev = base;
  for (int k = 1; k < Ke; ++k) {
    acc += std::pow(ratio, k - 1);
    const int64_t want = std::max(prev + 1, base + (int64_t)((double)(N - base) * acc / tot));
    CHECK(Ns[(size_t)k] == want, "Ns[%d] %lld, want %lld", k, (long long)Ns[(size_t)k], (long long)want);
    prev = want;
  }
}

static void bounds() {
  for (double ratio : {1.0, 1.15, 1.8})
    for (int K : {1, 2, 3, 8, 12, 16, 64, 65, 100})
      for (int64_t base : {(int64_t)0, (int64_t)4097, (int64_t)9000000})
        for (int64_t span : {(int64_t)100, (int64_t)4096, (int64_t)1000003, (int64_t)10000000})
          check_bounds(base, base + span, K, ratio);
  check_bounds(5, 5 + 8, 8, 1.8);  // N - base == K: one event each
  // equal shares at ratio 1
  int64_t Ns[5];
  bh::segment_bounds(0, 4000, 4, 1.0, Ns);
  for (int k = 0; k <= 4; ++k) CHECK(Ns[k] == 1000 * k, "equal segments: Ns[%d] = %lld", k, (long long)Ns[k]);
}

static int32_t brute_resume(const Vec &rq, const Vec &olen, const Vec &nlen, int32_t r0) {
  bool any = false;
  int32_t m = 0;
  for (size_t c = 0; c < rq.size(); ++c)
    if (nlen[c] > olen[c]) {
      m = any ? std::min(m, rq[c]) : rq[c];
      any = true;
    }
  if (!any) return r0;
  return m - 1 > r0 ? m - 1 : r0;
}

static void resume() {
  const int32_t r0 = 3;
  auto run = [&](const char *name, const Vec &rq, const Vec &olen, const Vec &nlen, int32_t want) {
    const int32_t got = bh::resume_round((int)rq.size(), rq.data(), olen.data(), nlen.data(), r0);
    CHECK(got == want, "%s: resume round %d, want %d", name, got, want);
    CHECK(got == brute_resume(rq, olen, nlen, r0), "%s: differs from the restatement", name);
  };
  run("no chain grew", {9, 1, 7}, {5, 5, 5}, {5, 5, 5}, r0);
  run("one grown chain at r0", {9, r0, 7}, {5, 5, 5}, {5, 6, 5}, r0);  // (not r0 - 1)
  run("one grown chain above r0", {9, 8, 7}, {5, 5, 5}, {5, 6, 5}, 7);
  run("minimum over grown chains only", {9, 4, 7}, {5, 5, 5}, {6, 5, 8}, 6);  // (chain 1, rq 4, did not grow)
  run("grown chain below r0", {1, 9, 9}, {0, 5, 5}, {2, 5, 5}, r0);
  run("every chain grew", {12, 10, 11}, {1, 2, 3}, {2, 3, 4}, 9);
  // exhaustive over small inputs
  for (int mask = 0; mask < 8; ++mask)
    for (int32_t a = 0; a < 6; ++a)
      for (int32_t b = 0; b < 6; ++b) {
        const Vec rq = {a, b, 5}, olen = {4, 4, 4}, nlen = {4 + (mask & 1), 4 + (mask >> 1 & 1), 4 + (mask >> 2 & 1)};
        run("sweep", rq, olen, nlen, brute_resume(rq, olen, nlen, r0));
      }
}

int main() {
  tiles();
  bounds();
  resume();
  if (failures) {
    fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  printf("sched_plan ok\n");
  return 0;
}
