// The score K29 (topk.hip: sl_topk_merge_biased) ranks a cosine by, stated once: CSLS, cross-domain similarity local scaling
// (Conneau et al. 2018), of the cosine c of a (row, column) pair under the row's bias r and the column's bias q,
//   score = (2.0f * c - r) - q        fp32, two roundings.
// Needs nothing but the compiler: a host program can include it (tests/native/biased_score_check.cpp holds the table), and the
// function is constexpr, which hipcc takes as host and device.
//
// 2.0f * c is exact for |c| < 2^127 (a change of the exponent; a denormal doubles exactly), so a contracted fma(2, c, -r) rounds
// the same real number once as the product-then-subtraction does: both forms give the same bits and the rule needs no
// contraction pragma, whatever -ffp-contract says.  (A finite |c| >= 2^127, which no cosine comes near, doubles to an infinity in
// the two-step form and not inside an fma; the rule is stated for the range below it.)
//
// NaN and the infinities follow IEEE arithmetic: inf - inf = NaN, and a NaN in any operand gives NaN.  The score is ordered by
// K17's total order (packed_best.hpp f32_order_key): NaN first, then the larger score, -0.0 == +0.0, ties by the smaller id.
#pragma once

namespace sl {

constexpr float biased_score(float c, float r, float q) { return (2.0f * c - r) - q; }

}  // namespace sl
