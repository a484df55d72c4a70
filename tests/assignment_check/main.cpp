// tests/assignment_check/main.cpp — TEST INFRASTRUCTURE: the cases of tests/test_fms_cpu.py on
// csrc/assignment.h as a stand-alone program, which tests/test_fms_cpu.py builds with
// -fsanitize=address,undefined and runs directly. Exits 0 when every case holds.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <numeric>
#include <vector>

#include "assignment.h"

static int failures = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
      failures++;                                                 \
    }                                                             \
  } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double u01() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  z ^= z >> 31;
  return (double)(z >> 11) / 9007199254740992.0;
}

// the best total over all injective maps of the shorter side into the longer one
static double brute_force(const std::vector<double> &s, int ra, int rb, int ld) {
  const bool swap = ra > rb;
  const int n = swap ? rb : ra, m = swap ? ra : rb;
  std::vector<int> idx(m);
  std::iota(idx.begin(), idx.end(), 0);
  double best = -std::numeric_limits<double>::infinity();
  do {
    double t = 0;
    for (int i = 0; i < n; i++) t += swap ? s[idx[i] + (size_t)ld * i] : s[i + (size_t)ld * idx[i]];
    best = std::max(best, t);
  } while (std::next_permutation(idx.begin(), idx.end()));
  return best;
}

static void check_matching(const std::vector<double> &s, int ra, int rb, int ld, const std::vector<int> &perm,
                           double sum) {
  std::vector<int> seen(rb, 0);
  int hit = 0;
  double t = 0;
  for (int p = 0; p < ra; p++) {
    if (perm[p] < 0) continue;
    CHECK(perm[p] < rb);
    if (perm[p] >= rb) return;
    CHECK(!seen[perm[p]]);
    seen[perm[p]] = 1;
    hit++;
    t += s[p + (size_t)ld * perm[p]];
  }
  CHECK(hit == std::min(ra, rb));
  CHECK(t == sum);
}

int main() {
  using ppals::match_columns;
  {  // a greedy matcher takes 0.9 and is left with 0.1
    const double s[4] = {0.9, 0.8, 0.8, 0.1};
    int perm[2];
    double sum = 0;
    CHECK(match_columns(s, 2, 2, 2, perm, &sum));
    CHECK(perm[0] == 1 && perm[1] == 0 && sum == 0.8 + 0.8);
    CHECK(match_columns(s, 2, 2, 2, nullptr, nullptr));
  }
  const int shapes[3][2] = {{5, 5}, {3, 5}, {5, 3}};
  for (int rep = 0; rep < 20; rep++)
    for (auto &sh : shapes)
      for (int pad = 0; pad < 3; pad += 2) {
        const int ra = sh[0], rb = sh[1], ld = ra + pad;
        std::vector<double> s((size_t)ld * rb, std::numeric_limits<double>::quiet_NaN());  // (the padding is never read)
        for (int q = 0; q < rb; q++)
          for (int p = 0; p < ra; p++) s[p + (size_t)ld * q] = 2.0 * u01() - 1.0;
        std::vector<int> perm(ra, -7);
        double sum = 0;
        CHECK(match_columns(s.data(), ra, rb, ld, perm.data(), &sum));
        check_matching(s, ra, rb, ld, perm, sum);
        const double want = brute_force(s, ra, rb, ld);
        CHECK(std::fabs(sum - want) <= 16 * std::numeric_limits<double>::epsilon());
      }
  for (int n : {64, 128}) {  // a planted permutation: >= 0.85 on it, <= 0.05 in modulus off it
    std::vector<int> pi(n);
    std::iota(pi.begin(), pi.end(), 0);
    for (int i = n - 1; i > 0; i--) std::swap(pi[i], pi[(int)(u01() * (i + 1))]);
    std::vector<double> s((size_t)n * n);
    for (auto &x : s) x = 0.1 * u01() - 0.05;
    for (int p = 0; p < n; p++) s[p + (size_t)n * pi[p]] = 0.85 + 0.15 * u01();
    std::vector<int> perm(n);
    double sum = 0;
    CHECK(match_columns(s.data(), n, n, n, perm.data(), &sum));
    CHECK(perm == pi);
  }
  for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(),
                     -std::numeric_limits<double>::infinity()}) {
    std::vector<double> s(15, 0.5);
    s[7] = bad;
    int perm[3] = {-7, -7, -7};
    double sum = -7;
    CHECK(!match_columns(s.data(), 3, 5, 3, perm, &sum));
    CHECK(perm[0] == -7 && sum == -7);
  }
  {  // the score from a congruence block: weights, and a weight pair without a positive finite maximum
    const double phi[4] = {1.0, 0.25, 0.125, -1.0}, wa[2] = {2.0, 0.0}, wb[2] = {1.0, 0.0};
    double f = 0;
    int perm[2];
    CHECK(ppals::fms_from_congruence(phi, 2, wa, wb, 2, 2, false, perm, &f) && f == 0.1875);
    CHECK(ppals::fms_from_congruence(phi, 2, wa, wb, 2, 2, true, perm, &f));
    CHECK(f == 0.25 && perm[0] == 0 && perm[1] == 1);  // 1.0 * (1 - 1/2) and 0 for the pair of zero weights
  }
  if (failures) return 1;
  std::printf("assignment.h: all cases hold\n");
  return 0;
}
