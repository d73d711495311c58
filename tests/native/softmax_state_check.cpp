// csrc/softmax_state.hpp compiled for the host: the rule that merges two (m, a, b, n) states, as the kernel's lanes, waves and
// workspace folds run it.  The empty state is the identity bit for bit; 10 000 random logits cut into shuffled groups and merged
// in shuffled orders agree with a long double log-sum-exp and entropy within the bound derived below; NaN, +inf and "nothing
// above -inf" survive every merge order.
//   g++ -O2 -std=c++17 -o softmax_state_check softmax_state_check.cpp && ./softmax_state_check   -> "failures=0"
//
// Bound (u = 2^-53).  A group's state is summed here in double against its own maximum: at most g u relative in a for g terms.
// A combine multiplies a by exp(dm) (1 ulp of exp, 1 of dm, dm <= 0 so the factor is at most 1: an error of dm u in the
// exponent gives |dm| u relative), rounds the product and the sum: (|dm| + 4) u relative per combine, |dm| <= G = the logits'
// range.  An entry passes through every combine above it, at most `merges` of them, and all terms are positive, so
//   |d log a| <= (g + merges (G + 4)) u.
// b takes the same factors and the product dm * a: |d b| / a <= (g + merges (G + 4)) u * (|b| / a + G), and |b| / a <= G.  Hence
//   |d entropy| <= (1 + 2 G) (g + merges (G + 4)) u   (the quotient's own rounding is below that).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <random>
#include <vector>

#include "../../semanticlens_amd/csrc/softmax_state.hpp"

namespace {

using sl::softmax::State;
namespace sm = sl::softmax;

int failures = 0;
const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();

void expect(bool ok, const char* name, const char* what) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s: %s\n", name, what);
  }
}

bool same_bits(const State& x, const State& y) { return std::memcmp(&x, &y, sizeof(State)) == 0; }

// the state of a list of logits, summed in double against the list's maximum (what a wave holds at the end of its segment)
State state_of(const double* l, size_t count) {
  double m = -kInf, a = 0.0, b = 0.0;
  bool nan = false, inf = false;
  for (size_t i = 0; i < count; ++i) {
    nan = nan || l[i] != l[i];
    inf = inf || l[i] == kInf;
    if (l[i] < kInf && l[i] > m) m = l[i];
  }
  if (m > -kInf)
    for (size_t i = 0; i < count; ++i)
      if (l[i] > -kInf && l[i] < kInf) a += std::exp(l[i] - m), b += (l[i] - m) * std::exp(l[i] - m);
  return sm::make(m, nan ? kNaN : inf ? kInf : a, b, (double)count);
}

enum Kind { kRegular, kEmpty, kPosInf, kNan };
Kind kind_of(const State& s) {
  if (s.m != s.m) return kNan;
  if (s.m == kInf) return kPosInf;
  if (s.m == -kInf) return kEmpty;
  return kRegular;
}

// merge the states in a random tree: repeatedly replace two random entries by their combine
State merge_shuffled(std::vector<State> v, std::mt19937_64& rng) {
  while (v.size() > 1) {
    const size_t i = rng() % v.size();
    std::swap(v[i], v.back());
    const State x = v.back();
    v.pop_back();
    const size_t j = rng() % v.size();
    v[j] = (rng() & 1) ? sm::combine(x, v[j]) : sm::combine(v[j], x);
  }
  return v[0];
}

void check_identity() {
  const State e = sm::empty_state();
  const double l[3] = {0.25, -3.0, 7.5};
  const State cases[] = {state_of(l, 3), sm::nan_state(4), sm::inf_state(2), sm::empty_state(), State{-kInf, 0.0, 0.0, 5.0}};
  for (const State& s : cases) {
    expect(same_bits(sm::combine(e, s), s), "identity", "combine(empty, s) != s");
    expect(same_bits(sm::combine(s, e), s), "identity", "combine(s, empty) != s");
  }
  expect(sm::log_z(e) == -kInf && sm::entropy(e) != sm::entropy(e), "identity", "the empty state's log_z / entropy");
  expect(sm::prob(e, -kInf, 0.0) == 0.0, "identity", "an empty slot's probability");
  // two states on one maximum: combine is the plain sum
  const State s = state_of(l, 3);
  expect(same_bits(sm::combine(s, s), sm::sum_same_max(s, s)), "identity", "combine on equal maxima is not sum_same_max");
}

void check_random(uint64_t seed, double range) {
  std::mt19937_64 rng(seed);
  const size_t n = 10000;
  std::vector<double> l(n);
  std::uniform_real_distribution<double> uni(-range, range);
  for (double& v : l) v = uni(rng);
  for (size_t i = 0; i < 50; ++i) l[rng() % n] = range - 1e-3 * (double)i;  // a cluster near the maximum
  long double m = -kInf, a = 0.0L, b = 0.0L;
  for (double v : l) m = std::max<long double>(m, v);
  for (double v : l) a += expl(v - m), b += (v - m) * expl(v - m);
  const long double want_lz = m + logl(a), want_h = logl(a) - b / a;
  const double G = 2.0 * range, u = std::ldexp(1.0, -53);
  for (size_t groups : {(size_t)1, (size_t)7, (size_t)64, (size_t)1000, n}) {
    std::shuffle(l.begin(), l.end(), rng);
    std::vector<size_t> cut{0, n};
    while (cut.size() < groups + 1) cut.push_back(1 + rng() % (n - 1));  // empty groups allowed
    std::sort(cut.begin(), cut.end());
    std::vector<State> parts;
    size_t largest = 0;
    for (size_t g = 0; g + 1 < cut.size(); ++g) {
      parts.push_back(state_of(l.data() + cut[g], cut[g + 1] - cut[g]));
      largest = std::max(largest, cut[g + 1] - cut[g]);
    }
    const State got = merge_shuffled(parts, rng);
    const double rel = ((double)largest + (double)parts.size() * (G + 4.0)) * u;
    const double bound_lz = rel + 4.0 * u * std::fabs((double)want_lz), bound_h = (1.0 + 2.0 * G) * rel;
    const double err_lz = std::fabs((double)(sm::log_z(got) - want_lz)), err_h = std::fabs((double)(sm::entropy(got) - want_h));
    std::printf("range %g groups %zu: log_z err %.3g (bound %.3g), entropy err %.3g (bound %.3g)\n", range, parts.size(), err_lz,
                bound_lz, err_h, bound_h);
    expect(err_lz <= bound_lz, "random", "log_z outside the bound");
    expect(err_h <= bound_h, "random", "entropy outside the bound");
    expect(got.n == (double)n, "random", "the count is not the number of candidates");
    double psum = 0.0;
    for (double v : l) psum += sm::prob(got, v, 0.0);
    expect(std::fabs(psum - 1.0) <= (double)n * 4.0 * u + bound_lz, "random", "probabilities do not sum to 1");
  }
}

void check_special() {
  std::mt19937_64 rng(7);
  const double reg[4] = {1.0, -2.0, 0.5, 3.0}, neg[3] = {-kInf, -kInf, -kInf}, mixed[4] = {-kInf, 2.0, -kInf, 1.0};
  const double with_nan[3] = {1.0, kNaN, 2.0}, with_inf[3] = {kInf, 0.0, -kInf}, both[3] = {kInf, kNaN, 1.0};
  expect(kind_of(state_of(neg, 3)) == kEmpty && state_of(neg, 3).n == 3.0, "special", "all -inf is not the empty kind with n = 3");
  expect(kind_of(state_of(with_nan, 3)) == kNan && kind_of(state_of(both, 3)) == kNan, "special", "a NaN candidate");
  expect(kind_of(state_of(with_inf, 3)) == kPosInf, "special", "a +inf candidate");
  {  // -inf candidates add nothing but their count
    const double fin[2] = {2.0, 1.0};
    const State x = state_of(mixed, 4), y = state_of(fin, 2);
    expect(x.m == y.m && x.a == y.a && x.b == y.b && x.n == 4.0, "special", "-inf candidates changed the sums");
  }
  struct Case {
    std::vector<State> parts;
    Kind want;
    const char* name;
  };
  const std::vector<Case> cases = {
      {{state_of(reg, 4), state_of(with_nan, 3), state_of(neg, 3), state_of(with_inf, 3), sm::empty_state()}, kNan, "NaN absorbs"},
      {{state_of(reg, 4), state_of(neg, 3), state_of(with_inf, 3), sm::empty_state(), state_of(mixed, 4)}, kPosInf, "+inf absorbs"},
      {{state_of(neg, 3), sm::empty_state(), state_of(neg, 3)}, kEmpty, "nothing above -inf"},
      {{state_of(neg, 3), state_of(reg, 4), sm::empty_state()}, kRegular, "regular"},
  };
  for (const Case& c : cases) {
    double n = 0.0;
    for (const State& s : c.parts) n += s.n;
    for (int rep = 0; rep < 200; ++rep) {
      const State got = merge_shuffled(c.parts, rng);
      expect(kind_of(got) == c.want, c.name, "the kind depends on the merge order");
      expect(got.n == n, c.name, "the count");
      const double lz = sm::log_z(got), h = sm::entropy(got), p = sm::prob(got, 1.0, 0.0);
      if (c.want == kNan) expect(lz != lz && h != h && p != p, c.name, "log_z, entropy and probs must be NaN");
      if (c.want == kPosInf) expect(lz == kInf && h != h && p != p, c.name, "log_z must be +inf, entropy and probs NaN");
      if (c.want == kEmpty) expect(lz == -kInf && h != h && p != p, c.name, "log_z must be -inf, entropy and probs NaN");
      if (c.want == kRegular) expect(std::fabs(lz - sm::log_z(state_of(reg, 4))) < 1e-15 * 8, c.name, "log_z of the regular part");
      expect(sm::prob(got, -kInf, n) == 0.0, c.name, "an empty slot must have probability 0");
    }
  }
}

}  // namespace

int main() {
  check_identity();
  for (double range : {1.0, 100.0, 1000.0}) check_random(11 + (uint64_t)range, range);
  check_special();
  std::printf("failures=%d\n", failures);
  return failures == 0 ? 0 : 1;
}
