// The running softmax statistics of K25 (softmax.hip) and the ONE rule that merges two of them.  Needs only <cmath>: the
// kernel's lane, wave and workspace combines and the host program tests/native/softmax_state_check.cpp run the same code, so
// the rule is checkable on the CPU, as packed_best.hpp's order and unionfind.hpp's forest are.
//
// For a set of logits l_j the state holds
//   m = max_j l_j,   a = sum_j exp(l_j - m),   b = sum_j (l_j - m) exp(l_j - m),   n = how many candidates were folded,
// from which  log_z = m + log a,  entropy = log a - b / a  (nats)  and  p_j = exp(l_j - log_z).  Every term of a lies in (0, 1] and
// the maximum's own term is 1, so a >= 1 and nothing overflows whatever the logits' size.  n counts every candidate, -inf
// and NaN included: a top-k state (K17) is sorted with its empty slots last, so slot i of a row is empty iff i >= n.
//
// Four kinds of state, told apart by m alone:
//   regular   m finite, a >= 1, b <= 0
//   empty     m = -inf, a = b = 0: nothing above -inf was seen (nothing at all, or only -inf candidates, which add to n alone)
//   +inf      m = +inf, a = b = NaN: a +inf candidate was seen and no NaN
//   NaN       m = a = b = NaN: a NaN candidate was seen
// combine() is commutative; NaN absorbs everything, +inf everything but NaN, and the empty state is the identity (bit for
// bit).  These follow torch.logsumexp / torch.softmax in float64.
//
// Rebase: moving a regular state to a larger reference m' >= m multiplies every term by f = exp(m - m'):
//   a' = a f,   b' = sum_j (l_j - m') exp(l_j - m') = (b + (m - m') a) f.
// Two states on the SAME reference add component by component (sum_same_max); combine() is rebase to the larger m, then that sum.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SL_SM_FN __host__ __device__ inline
#else
#define SL_SM_FN inline
#endif

namespace sl {
namespace softmax {

struct State {
  double m, a, b, n;
};

SL_SM_FN double pos_inf() { return __builtin_inf(); }
SL_SM_FN double quiet_nan() { return __builtin_nan(""); }
SL_SM_FN bool is_nan(double x) { return x != x; }

SL_SM_FN State empty_state() { return State{-pos_inf(), 0.0, 0.0, 0.0}; }
SL_SM_FN State nan_state(double n) { return State{quiet_nan(), quiet_nan(), quiet_nan(), n}; }
SL_SM_FN State inf_state(double n) { return State{pos_inf(), quiet_nan(), quiet_nan(), n}; }

SL_SM_FN bool is_regular(const State& s) { return s.m > -pos_inf() && s.m < pos_inf(); }  // false for a NaN m

// The canonical state of raw sums taken against the reference m: a NaN among them means a NaN candidate, an infinite a (a
// sum of non-negative terms) a +inf candidate; sums against m = -inf saw nothing finite.
SL_SM_FN State make(double m, double a, double b, double n) {
  if (is_nan(m) || is_nan(a)) return nan_state(n);
  if (m == pos_inf() || a == pos_inf()) return inf_state(n);
  if (m == -pos_inf()) return State{m, 0.0, 0.0, n};
  return State{m, a, b, n};
}

// a state with finite sums (regular, or sums against m = -inf), moved to the finite reference m >= s.m
SL_SM_FN State rebase(const State& s, double m) {
  if (s.m == m) return s;
  if (s.m == -pos_inf() || s.a == 0.0) return State{m, 0.0, 0.0, s.n};
  const double dm = s.m - m;
  const double f = exp(dm);
  return State{m, s.a * f, (s.b + dm * s.a) * f, s.n};
}

// two states on one finite reference (x.m == y.m)
SL_SM_FN State sum_same_max(const State& x, const State& y) { return State{x.m, x.a + y.a, x.b + y.b, x.n + y.n}; }

SL_SM_FN State combine(const State& x, const State& y) {
  const double n = x.n + y.n;
  if (is_nan(x.m) || is_nan(y.m)) return nan_state(n);
  const double m = x.m > y.m ? x.m : y.m;
  if (m == pos_inf()) return inf_state(n);
  if (m == -pos_inf()) return State{m, 0.0, 0.0, n};
  return sum_same_max(rebase(x, m), rebase(y, m));
}

SL_SM_FN double log_z(const State& s) { return is_regular(s) ? s.m + log(s.a) : s.m; }  // -inf, +inf and NaN pass through
SL_SM_FN double entropy(const State& s) { return is_regular(s) ? log(s.a) - s.b / s.a : quiet_nan(); }

// probability of the candidate with the logit l under the state; slot = its position in the row's sorted top-k state
SL_SM_FN double prob(const State& s, double l, double slot) {
  if (slot >= s.n) return 0.0;  // an empty slot
  return is_regular(s) ? exp(l - log_z(s)) : quiet_nan();
}

}  // namespace softmax
}  // namespace sl
