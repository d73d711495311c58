// K28 (omp.hip): the state one component carries through an orthogonal matching pursuit and the rules that change it, as plain
// functions.  Needs only <cmath> and <cstdint>: the kernel (lane-uniform, one wave per component) and the host program
// tests/native/omp_state_check.cpp run the same code, as softmax_state.hpp's merge and rank_order.hpp's order are.
//
// After t accepted terms a component holds
//   S      the t chosen vocabulary ids, in the order chosen,
//   L      the Cholesky factor of G = W_S W_S^T (rows of W_S: the chosen words, each divided by its norm; unit diagonal), lower
//          triangular and packed row by row: entry (i, j), j <= i, at i (i + 1) / 2 + j; s (s + 1) / 2 doubles for s terms,
//   b      W_S x, x the component divided by its norm: t doubles.
// A step appends one word: chol_append extends L by the row z that solves L z = g (g: the new word's cosines to the chosen ones)
// and the diagonal sqrt(1 - z.z); then chol_solve gives the least-squares weights a from L L^T a = b.
//
// Two design constants, not measurements:
//   kMinPivot      1e-10: a pivot d^2 = 1 - z.z below it means the word is, to five digits of its sine, a linear combination of the
//                  chosen ones (a duplicate vocabulary entry gives d^2 of about 1e-16); dividing by its root would amplify rounding.
//   kResidualDone  1e-8: |r|^2 at or below it means the chosen words span the component to four digits; the next pass would rank
//                  the vocabulary by the direction of rounding noise.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SL_OMP_FN __host__ __device__ inline
#else
#define SL_OMP_FN inline
#endif

namespace sl {
namespace omp {

constexpr int kMaxTerms = 16;
constexpr double kMinPivot = 1e-10;
constexpr double kResidualDone = 1e-8;

constexpr int packed_size(int s) { return s * (s + 1) / 2; }
constexpr int packed_at(int i, int j) { return i * (i + 1) / 2 + j; }

// NaN (a word of zero or non-finite norm) stops like a small pivot
SL_OMP_FN bool pivot_stops(double d2) { return !(d2 >= kMinPivot); }
SL_OMP_FN bool residual_done(double r2) { return r2 <= kResidualDone; }
// a row can be divided by its norm: the sum of its squares is a positive finite number (false for NaN)
SL_OMP_FN bool word_usable(double sum_of_squares) { return sum_of_squares > 0.0 && sum_of_squares < __builtin_inf(); }

// Extend the factor of t rows by row t.  g[0..t): the cosines of the new unit vector to the t chosen ones; its own is 1.
// *pivot = 1 - z.z.  Returns false, leaving rows [0, t) as they were, when pivot_stops(*pivot); row t is then not meaningful.
SL_OMP_FN bool chol_append(double* L, int t, const double* g, double* pivot) {
  double* z = L + packed_at(t, 0);
  double zz = 0.0;
  for (int i = 0; i < t; ++i) {
    double v = g[i];
    for (int j = 0; j < i; ++j) v -= L[packed_at(i, j)] * z[j];
    v /= L[packed_at(i, i)];
    z[i] = v;
    zz += v * v;
  }
  const double d2 = 1.0 - zz;
  *pivot = d2;
  if (pivot_stops(d2)) return false;
  z[t] = sqrt(d2);
  return true;
}

// a[0..t) from L L^T a = b for the factor's first t rows
SL_OMP_FN void chol_solve(const double* L, int t, const double* b, double* a) {
  for (int i = 0; i < t; ++i) {
    double v = b[i];
    for (int j = 0; j < i; ++j) v -= L[packed_at(i, j)] * a[j];
    a[i] = v / L[packed_at(i, i)];
  }
  for (int i = t - 1; i >= 0; --i) {
    double v = a[i];
    for (int j = i + 1; j < t; ++j) v -= L[packed_at(j, i)] * a[j];
    a[i] = v / L[packed_at(i, i)];
  }
}

// ---- which candidate a step takes ----------------------------------------------------------------------------------------------
// Candidates come best first in K17's order (NaN before every number, then the larger value).  A slot whose id is outside [0, V)
// is empty (K17 writes -1 there) and is passed over without its id being used for anything else.
enum Stop : int { kTake = 0, kStopNoCandidate = 1, kStopNaN = 2, kStopCorrelation = 3, kStopPivot = 4, kStopResidual = 5 };

struct Choice {
  int slot;  // the candidate to append; -1 when the component stops
  int stop;  // kTake, or why it stops
};

SL_OMP_FN bool is_chosen(int64_t id, const int64_t* chosen, int t) {
  for (int i = 0; i < t; ++i)
    if (chosen[i] == id) return true;
  return false;
}

// The first candidate that is a vocabulary id and not among the t chosen ones; the component stops when there is none, when that
// candidate's value is NaN or when it is <= min_correlation.
SL_OMP_FN Choice choose(const float* vals, const int64_t* ids, int k_cand, const int64_t* chosen, int t, int64_t V,
                        double min_correlation) {
  for (int j = 0; j < k_cand; ++j) {
    const int64_t id = ids[j];
    if (id < 0 || id >= V || is_chosen(id, chosen, t)) continue;
    const float v = vals[j];
    if (v != v) return Choice{-1, kStopNaN};
    if ((double)v <= min_correlation) return Choice{-1, kStopCorrelation};
    return Choice{j, kTake};
  }
  return Choice{-1, kStopNoCandidate};
}

}  // namespace omp
}  // namespace sl
