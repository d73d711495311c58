// K26 (rank.hip): which candidates stand before a given (value, id) key in K17's order, as pure functions.  Needs only
// <cstdint>: a host compiler can include it (tests/native/rank_order_check.cpp holds the table), and the functions are constexpr,
// which hipcc takes as host and device.
// Order (packed_best.hpp): NaN before every number, then the larger value, -0.0 == +0.0, equal values by the smaller id.  The
// rank of a key is the number of candidates that order before it; the candidate with the key's own id is never counted, whatever
// value it carries, so the rank is the 0-based position the key holds in the fully sorted row.
#pragma once
#include <cstdint>

#include "packed_best.hpp"

namespace sl {
namespace rank_order {

// *_key: f32_order_key of the value
constexpr bool orders_before(uint32_t cand_key, int64_t cand_id, uint32_t key, int64_t key_id) {
  return cand_id != key_id && (cand_key > key || (cand_key == key && cand_id < key_id));
}

// The same rule in the 32-bit column arithmetic of a stretch of n columns whose first column has the id `first_id`.
// key_column: where the key's id falls, -1 = before the stretch, n = after it, else the column.
constexpr int32_t key_column(int64_t key_id, int64_t first_id, int32_t n) {
  const int64_t d = key_id - first_id;
  return d < 0 ? -1 : d >= n ? n : (int32_t)d;
}

// A candidate left of the key's column wins a tie, one right of it does not: "orders before" is cand_key > threshold.  Every
// real value's key is >= 0x007FFFFF, so key - 1 does not wrap, and the key 0 (a column outside the tile) is above no threshold.
constexpr uint32_t threshold(uint32_t key, bool left_of_key) { return left_of_key ? key - 1u : key; }

// orders_before(cand_key, first_id + col, key, key_id) for col in [0, n) and key_col = key_column(key_id, first_id, n)
constexpr bool column_orders_before(uint32_t cand_key, int32_t col, uint32_t key, int32_t key_col) {
  return col != key_col && cand_key > threshold(key, col < key_col);
}

}  // namespace rank_order
}  // namespace sl
