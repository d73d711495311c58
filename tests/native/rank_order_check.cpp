// csrc/rank_order.hpp compiled for the host: which candidate orders before a (value, id) key (K26, rank.hip), on a table, and the
// 32-bit column form the kernel runs against the rule itself, exhaustively over a small tile.
//   g++ -O2 -std=c++17 -o rank_order_check rank_order_check.cpp && ./rank_order_check   -> "failures=0"
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../semanticlens_amd/csrc/rank_order.hpp"

namespace {

using sl::f32_order_key;
namespace ro = sl::rank_order;

int failures = 0;
const float kInf = std::numeric_limits<float>::infinity();
const float kNaN = std::numeric_limits<float>::quiet_NaN();

struct Case {
  const char* name;
  float cand;
  int64_t cand_id;
  float key;
  int64_t key_id;
  bool before;
};

constexpr int64_t kBig = (1ll << 32) + 7;  // ids above 2^32

const Case kTable[] = {
    // NaN against NaN: equal keys, the smaller id first
    {"nan before nan, smaller id", kNaN, 3, kNaN, 5, true},
    {"nan after nan, larger id", kNaN, 5, kNaN, 3, false},
    {"negative nan is a nan", -kNaN, 3, kNaN, 5, true},
    // NaN before every number
    {"nan before +inf", kNaN, 9, kInf, 0, true},
    {"+inf not before nan", kInf, 0, kNaN, 9, false},
    {"nan before 0.5", kNaN, 9, 0.5f, 0, true},
    {"-inf not before nan", -kInf, 0, kNaN, 9, false},
    // +-0 are one value: the id decides
    {"-0 before +0 by id", -0.0f, 1, 0.0f, 2, true},
    {"+0 before -0 by id", 0.0f, 1, -0.0f, 2, true},
    {"-0 not before +0, larger id", -0.0f, 2, 0.0f, 1, false},
    {"+0 not before -0, larger id", 0.0f, 2, -0.0f, 1, false},
    {"+0 before -1", 0.0f, 7, -1.0f, 0, true},
    {"-0 before -1", -0.0f, 7, -1.0f, 0, true},
    {"-0 not before 0.25", -0.0f, 0, 0.25f, 7, false},
    // +-inf
    {"+inf before 0.5", kInf, 9, 0.5f, 0, true},
    {"0.5 not before +inf", 0.5f, 0, kInf, 9, false},
    {"+inf ties +inf, smaller id", kInf, 1, kInf, 2, true},
    {"+inf ties +inf, larger id", kInf, 2, kInf, 1, false},
    {"-inf not before -1", -kInf, 0, -1.0f, 9, false},
    {"-1 before -inf", -1.0f, 9, -kInf, 0, true},
    {"-inf ties -inf, smaller id", -kInf, 1, -kInf, 2, true},
    {"-inf ties -inf, larger id", -kInf, 2, -kInf, 1, false},
    // equal values on both sides of the id
    {"equal value, id below", 0.5f, 4, 0.5f, 5, true},
    {"equal value, id above", 0.5f, 6, 0.5f, 5, false},
    {"larger value, id above", 0.75f, 6, 0.5f, 5, true},
    {"smaller value, id below", 0.25f, 4, 0.5f, 5, false},
    {"negative values: -1 before -2", -1.0f, 6, -2.0f, 5, true},
    {"negative values: -2 not before -1", -2.0f, 4, -1.0f, 5, false},
    // the key's own id is never counted, whatever value sits there
    {"own id, equal value", 0.5f, 5, 0.5f, 5, false},
    {"own id, larger value", 0.75f, 5, 0.5f, 5, false},
    {"own id, nan", kNaN, 5, 0.5f, 5, false},
    {"own id, nan key", kNaN, 5, kNaN, 5, false},
    // ids above 2^32: compared as 64-bit numbers, not by their low words
    {"big ids, equal value, id below", 0.5f, kBig - 1, 0.5f, kBig, true},
    {"big ids, equal value, id above", 0.5f, kBig + 1, 0.5f, kBig, false},
    {"big id against small id with the same low word", 0.5f, 7, 0.5f, kBig, true},
    {"small id key against big id with the same low word", 0.5f, kBig, 0.5f, 7, false},
    {"big own id", 0.75f, kBig, 0.5f, kBig, false},
    {"big ids, larger value", 0.75f, kBig + 1, 0.5f, kBig, true},
};

void expect(bool ok, const char* name) {
  if (!ok) {
    ++failures;
    std::printf("FAIL %s\n", name);
  }
}

static_assert(ro::orders_before(f32_order_key(1.0f), 0, f32_order_key(0.5f), 1), "usable in constant expressions");
static_assert(!ro::orders_before(f32_order_key(1.0f), 1, f32_order_key(0.5f), 1), "the key's own id");

}  // namespace

int main() {
  for (const Case& c : kTable) expect(ro::orders_before(f32_order_key(c.cand), c.cand_id, f32_order_key(c.key), c.key_id) == c.before, c.name);

  // key_column: before / inside / after a stretch of n columns, with first ids and key ids above 2^32 and 2^40
  expect(ro::key_column(4, 5, 8) == -1, "key_column: before");
  expect(ro::key_column(5, 5, 8) == 0, "key_column: first");
  expect(ro::key_column(12, 5, 8) == 7, "key_column: last");
  expect(ro::key_column(13, 5, 8) == 8, "key_column: after");
  expect(ro::key_column(0, (1ll << 40), 1024) == -1, "key_column: far before");
  expect(ro::key_column((1ll << 40) + 1023, (1ll << 40), 1024) == 1023, "key_column: big ids, last");
  expect(ro::key_column((1ll << 62), 0, 1024) == 1024, "key_column: far after");
  expect(ro::key_column(kBig, 7, 1024) == 1024, "key_column: same low word, far after");
  expect(ro::key_column(2, -3, 1024) == 5, "key_column: a stretch that starts left of id 0");

  // the column form against the rule: every special value as candidate and as key, the key's id before, at every column of,
  // and after a stretch of 6 columns that starts at several first ids
  const float values[] = {kNaN, kInf, 0.5f, 0.25f, 0.0f, -0.0f, -1.0f, -kInf};
  const int n = 6;
  const int64_t firsts[] = {0, 3, (1ll << 31) + 5, (1ll << 40)};
  for (int64_t first : firsts)
    for (int64_t key_id = first > 2 ? first - 2 : 0; key_id <= first + n + 1; ++key_id)
      for (float key : values)
        for (float cand : values)
          for (int col = 0; col < n; ++col) {
            const bool rule = ro::orders_before(f32_order_key(cand), first + col, f32_order_key(key), key_id);
            const bool form = ro::column_orders_before(f32_order_key(cand), col, f32_order_key(key), ro::key_column(key_id, first, n));
            expect(rule == form, "column form differs from orders_before");
            // a column outside the tile carries the key 0 and is counted nowhere
            expect(!ro::column_orders_before(0u, col, f32_order_key(key), ro::key_column(key_id, first, n)), "key 0 counted");
          }
  std::printf("failures=%d\n", failures);
  return failures != 0;
}
