// assignment.h — the rectangular assignment problem behind the factor match score, host only and free
// of HIP: ppals_match_columns and CpEngine::fms_pairs (include/ppals.h, "factor match score").
//
// match_columns: given score[p + ld*q], p < ra, q < rb, choose m = min(ra, rb) pairs (p, q), no p and no q
// twice, of the largest total. The exact optimum by the Hungarian method with potentials (shortest
// augmenting paths, O(min^2 * max) <= O(n^3)); ties are broken by the scan order alone, so the same input
// gives the same matching. The total is re-added from the chosen entries in the order of p.
#pragma once
#include <cmath>
#include <limits>
#include <vector>

namespace ppals {

// perm (may be nullptr): ra ints, perm[p] = the matched q, or -1 for a p left out (ra > rb).
// Returns false, touching nothing, when an entry is not finite.
inline bool match_columns(const double *score, int ra, int rb, int ld, int *perm, double *sum) {
  for (int q = 0; q < rb; q++)
    for (int p = 0; p < ra; p++)
      if (!std::isfinite(score[p + (size_t)ld * q])) return false;
  // rows of the method: the shorter side (n <= m); cost = -score
  const bool swap = ra > rb;
  const int n = swap ? rb : ra, m = swap ? ra : rb;
  auto cost = [&](int i, int j) {  // i < n, j < m
    return swap ? -score[j + (size_t)ld * i] : -score[i + (size_t)ld * j];
  };
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<double> u(n + 1, 0.0), v(m + 1, 0.0), minv(m + 1);
  std::vector<int> row_of(m + 1, 0), way(m + 1, 0);  // 1-based; row_of[j] = 0: column j is free
  std::vector<char> used(m + 1);
  for (int i = 1; i <= n; i++) {
    row_of[0] = i;
    int j0 = 0;
    minv.assign(m + 1, inf);
    used.assign(m + 1, 0);
    do {
      used[j0] = 1;
      const int i0 = row_of[j0];
      double delta = inf;
      int j1 = 0;
      for (int j = 1; j <= m; j++) {
        if (used[j]) continue;
        const double cur = cost(i0 - 1, j - 1) - u[i0] - v[j];
        if (cur < minv[j]) {
          minv[j] = cur;
          way[j] = j0;
        }
        if (minv[j] < delta) {
          delta = minv[j];
          j1 = j;
        }
      }
      for (int j = 0; j <= m; j++) {
        if (used[j]) {
          u[row_of[j]] += delta;
          v[j] -= delta;
        } else {
          minv[j] -= delta;
        }
      }
      j0 = j1;
    } while (row_of[j0] != 0);
    do {
      const int j1 = way[j0];
      row_of[j0] = row_of[j1];
      j0 = j1;
    } while (j0);
  }
  std::vector<int> pi(ra, -1);
  for (int j = 1; j <= m; j++) {
    if (!row_of[j]) continue;
    if (swap)
      pi[j - 1] = row_of[j] - 1;
    else
      pi[row_of[j] - 1] = j - 1;
  }
  double total = 0;
  for (int p = 0; p < ra; p++)
    if (pi[p] >= 0) total += score[p + (size_t)ld * pi[p]];
  if (perm)
    for (int p = 0; p < ra; p++) perm[p] = pi[p];
  if (sum) *sum = total;
  return true;
}

// The factor match score of a rank-ra model against a rank-rb one from their block of the congruence
// matrix (Phi[p + ld*q]) and their weights w_a[ra], w_b[rb] (read only when `weights`):
//   score = Phi                                              (weights false)
//         = Phi * (1 - |w_a - w_b| / max(w_a, w_b))          (true; 0 where the max is not positive finite)
//   fms   = (largest total of min(ra, rb) matched pairs) / min(ra, rb)
// Returns false when Phi holds an entry that is not finite.
inline bool fms_from_congruence(const double *Phi, int ld, const double *wa, const double *wb, int ra, int rb,
                                bool weights, int *perm, double *fms) {
  std::vector<double> s((size_t)ra * rb);
  for (int q = 0; q < rb; q++)
    for (int p = 0; p < ra; p++) {
      double x = Phi[p + (size_t)ld * q];
      if (!std::isfinite(x)) return false;
      if (weights) {
        const double mx = wa[p] > wb[q] ? wa[p] : wb[q];
        const double f = 1.0 - std::fabs(wa[p] - wb[q]) / mx;
        x = (mx > 0.0 && mx <= std::numeric_limits<double>::max() && std::isfinite(f)) ? x * f : 0.0;
      }
      s[p + (size_t)ra * q] = x;
    }
  double total = 0;
  if (!match_columns(s.data(), ra, rb, ra, perm, &total)) return false;
  *fms = total / (double)(ra < rb ? ra : rb);
  return true;
}

}  // namespace ppals
