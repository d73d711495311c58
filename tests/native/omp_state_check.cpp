// csrc/omp_state.hpp compiled for the host: the Cholesky append and solve of K28 (omp.hip) against a direct long double solve of the
// normal equations, and every branch of the rule that picks a step's candidate, on a table.
//   g++ -O2 -std=c++17 -o omp_state_check omp_state_check.cpp && ./omp_state_check   -> "failures=0"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

#include "../../semanticlens_amd/csrc/omp_state.hpp"

namespace {

namespace omp = sl::omp;

int failures = 0;
const float kNaN = std::numeric_limits<float>::quiet_NaN();

void expect(bool ok, const char* name) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s\n", name);
  }
}

// a = G^-1 b by Gaussian elimination with partial pivoting in long double
std::vector<long double> solve_direct(std::vector<long double> G, std::vector<long double> b, int n) {
  for (int c = 0; c < n; ++c) {
    int p = c;
    for (int r = c + 1; r < n; ++r)
      if (fabsl(G[r * n + c]) > fabsl(G[p * n + c])) p = r;
    for (int k = 0; k < n; ++k) std::swap(G[c * n + k], G[p * n + k]);
    std::swap(b[c], b[p]);
    for (int r = c + 1; r < n; ++r) {
      const long double f = G[r * n + c] / G[c * n + c];
      for (int k = c; k < n; ++k) G[r * n + k] -= f * G[c * n + k];
      b[r] -= f * b[c];
    }
  }
  std::vector<long double> a(n);
  for (int r = n - 1; r >= 0; --r) {
    long double v = b[r];
    for (int k = r + 1; k < n; ++k) v -= G[r * n + k] * a[k];
    a[r] = v / G[r * n + r];
  }
  return a;
}

// Random unit vectors with a shared direction mixed in (cosines of about `mix`^2: a Gram matrix that is not nearly the identity);
// rows appended one at a time, the weights after every append against the direct solve.  Bound: the solve's error is a few
// units of cond(G) x 2^-53; cond(G) stays below 100 here, so 1e-12 leaves two orders.
void check_append_and_solve(int D, double mix, unsigned seed) {
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal;
  const int s = omp::kMaxTerms;
  std::vector<double> common(D), W(s * D), x(D);
  for (double& v : common) v = normal(gen);
  auto unit = [&](double* row) {
    double n = 0;
    for (int d = 0; d < D; ++d) n += row[d] * row[d];
    n = std::sqrt(n);
    for (int d = 0; d < D; ++d) row[d] /= n;
  };
  unit(common.data());
  for (int i = 0; i < s; ++i) {
    for (int d = 0; d < D; ++d) W[i * D + d] = normal(gen) / std::sqrt((double)D) + mix * common[d];
    unit(&W[i * D]);
  }
  for (int d = 0; d < D; ++d) x[d] = normal(gen);
  unit(x.data());
  std::vector<double> L(omp::packed_size(s), 0.0), b(s), a(s), g(s);
  for (int t = 0; t < s; ++t) {
    for (int i = 0; i < t; ++i) {
      g[i] = 0;
      for (int d = 0; d < D; ++d) g[i] += W[t * D + d] * W[i * D + d];
    }
    double pivot = 0;
    const bool ok = omp::chol_append(L.data(), t, g.data(), &pivot);
    expect(ok && pivot > omp::kMinPivot && pivot <= 1.0 + 1e-15, "append: independent rows are accepted");
    b[t] = 0;
    for (int d = 0; d < D; ++d) b[t] += W[t * D + d] * x[d];
    const int n = t + 1;
    omp::chol_solve(L.data(), n, b.data(), a.data());
    std::vector<long double> G(n * n), bl(n);
    for (int i = 0; i < n; ++i) {
      bl[i] = 0;
      for (int d = 0; d < D; ++d) bl[i] += (long double)W[i * D + d] * x[d];
      for (int j = 0; j < n; ++j) {
        long double v = 0;
        for (int d = 0; d < D; ++d) v += (long double)W[i * D + d] * W[j * D + d];
        G[i * n + j] = i == j ? 1.0L : v;
      }
    }
    const std::vector<long double> want = solve_direct(G, bl, n);
    for (int i = 0; i < n; ++i) expect(fabsl(want[i] - a[i]) <= 1e-12L, "solve: weights against the long double normal equations");
    // L L^T = G on the rows so far
    for (int i = 0; i < n; ++i)
      for (int j = 0; j <= i; ++j) {
        long double v = 0;
        for (int k = 0; k <= j; ++k) v += (long double)L[omp::packed_at(i, k)] * L[omp::packed_at(j, k)];
        expect(fabsl(v - G[i * n + j]) <= 1e-13L, "append: L L^T reproduces the Gram matrix");
      }
  }
}

void check_pivot() {
  // two orthogonal unit rows chosen; a third with cosines (c, 0): z = (c, 0), pivot = 1 - c^2
  double L[omp::packed_size(3)] = {1.0, 0.0, 1.0, 9.0, 9.0, 9.0};
  double pivot = 0;
  const double just_above = std::sqrt(1.0 - 1.5e-10), just_below = std::sqrt(1.0 - 0.5e-10);
  double g[2] = {just_above, 0.0};
  expect(omp::chol_append(L, 2, g, &pivot) && pivot > omp::kMinPivot && pivot < 2e-10, "pivot just above 1e-10 is accepted");
  expect(std::fabs(L[omp::packed_at(2, 2)] - std::sqrt(pivot)) == 0.0 && L[omp::packed_at(2, 0)] == just_above, "accepted row is written");
  g[0] = just_below;
  expect(!omp::chol_append(L, 2, g, &pivot) && pivot < omp::kMinPivot && pivot > 0.0, "pivot just below 1e-10 stops");
  expect(L[0] == 1.0 && L[1] == 0.0 && L[2] == 1.0, "a refused append leaves the rows before it alone");
  g[0] = 1.0;  // an exact duplicate of the first row
  expect(!omp::chol_append(L, 2, g, &pivot) && pivot == 0.0, "a duplicate row has pivot 0");
  g[0] = std::numeric_limits<double>::quiet_NaN();
  expect(!omp::chol_append(L, 2, g, &pivot), "a NaN cosine stops");
  expect(omp::pivot_stops(0.99e-10) && !omp::pivot_stops(1e-10) && !omp::pivot_stops(1.0), "pivot_stops at the constant");
  expect(omp::residual_done(1e-8) && omp::residual_done(0.0) && !omp::residual_done(1.0000001e-8) && !omp::residual_done(std::nan("")),
         "residual_done at the constant");
  expect(omp::word_usable(1.0) && !omp::word_usable(0.0) && !omp::word_usable(INFINITY) && !omp::word_usable(std::nan("")), "word_usable");
  double one[1];
  expect(omp::chol_append(one, 0, nullptr, &pivot) && pivot == 1.0 && one[0] == 1.0, "the first row: pivot 1");
}

struct Case {
  const char* name;
  float vals[4];
  int64_t ids[4];
  int k_cand;
  int64_t chosen[3];
  int t;
  int64_t V;
  double min_correlation;
  int slot, stop;
};

const Case kTable[] = {
    {"first candidate taken", {0.9f, 0.8f}, {7, 3}, 2, {3}, 1, 10, 0.0, 0, omp::kTake},
    {"nothing chosen yet", {0.9f}, {7}, 1, {}, 0, 10, 0.0, 0, omp::kTake},
    {"first already chosen, second taken", {0.9f, 0.8f}, {7, 3}, 2, {7}, 1, 10, 0.0, 1, omp::kTake},
    {"two chosen, third taken", {0.9f, 0.8f, 0.7f}, {7, 3, 5}, 3, {3, 7}, 2, 10, 0.0, 2, omp::kTake},
    {"all chosen", {0.9f, 0.8f}, {7, 3}, 2, {3, 7}, 2, 10, 0.0, -1, omp::kStopNoCandidate},
    {"nan stops", {kNaN, 0.8f}, {7, 3}, 2, {}, 0, 10, 0.0, -1, omp::kStopNaN},
    {"a chosen nan is passed over", {kNaN, 0.8f}, {7, 3}, 2, {7}, 1, 10, 0.0, 1, omp::kTake},
    {"value exactly min_correlation stops", {0.25f, 0.2f}, {7, 3}, 2, {}, 0, 10, 0.25, -1, omp::kStopCorrelation},
    {"value just above min_correlation", {0.25000003f, 0.2f}, {7, 3}, 2, {}, 0, 10, 0.25, 0, omp::kTake},
    {"value below min_correlation stops, a later larger one is not looked at", {0.1f, 0.9f}, {7, 3}, 2, {}, 0, 10, 0.25, -1, omp::kStopCorrelation},
    {"zero stops at min_correlation 0", {0.0f}, {7}, 1, {}, 0, 10, 0.0, -1, omp::kStopCorrelation},
    {"negative zero stops at min_correlation 0", {-0.0f}, {7}, 1, {}, 0, 10, 0.0, -1, omp::kStopCorrelation},
    {"negative value stops", {-0.5f}, {7}, 1, {}, 0, 10, 0.0, -1, omp::kStopCorrelation},
    {"id -1 is an empty slot", {0.9f, 0.8f}, {-1, 3}, 2, {}, 0, 10, 0.0, 1, omp::kTake},
    {"only empty slots", {-INFINITY, -INFINITY}, {-1, -1}, 2, {}, 0, 10, 0.0, -1, omp::kStopNoCandidate},
    {"id V is an empty slot", {0.9f, 0.8f}, {10, 3}, 2, {}, 0, 10, 0.0, 1, omp::kTake},
    {"id far above V", {0.9f, 0.8f}, {(1ll << 40), 3}, 2, {}, 0, 10, 0.0, 1, omp::kTake},
    {"id V - 1 is a word", {0.9f, 0.8f}, {9, 3}, 2, {}, 0, 10, 0.0, 0, omp::kTake},
    {"id below -1", {0.9f, 0.8f}, {-5, 3}, 2, {}, 0, 10, 0.0, 1, omp::kTake},
    {"chosen first, then an empty slot", {0.9f, -INFINITY}, {7, -1}, 2, {7}, 1, 10, 0.0, -1, omp::kStopNoCandidate},
};

}  // namespace

int main() {
  static_assert(omp::packed_size(16) == 136 && omp::packed_at(0, 0) == 0 && omp::packed_at(2, 1) == 4 && omp::packed_at(15, 15) == 135,
                "packed lower triangle, row by row");
  for (const Case& c : kTable) {
    const omp::Choice got = omp::choose(c.vals, c.ids, c.k_cand, c.chosen, c.t, c.V, c.min_correlation);
    expect(got.slot == c.slot && got.stop == c.stop, c.name);
  }
  check_pivot();
  for (unsigned seed = 0; seed < 8; ++seed) {
    check_append_and_solve(64, 0.0, seed);
    check_append_and_solve(32, 0.5, 100 + seed);
    check_append_and_solve(130, 1.0, 200 + seed);
  }
  std::printf("failures=%d\n", failures);
  return failures != 0;
}
