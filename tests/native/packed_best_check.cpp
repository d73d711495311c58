// Host-side check of semanticlens_amd/csrc/packed_best.hpp: the fp32 order key and its inverse, the packed (value, id) entry of the
// K20 / K22 states, and the id range it holds.  Built and run by tests/test_host_logic.py with g++.
// The expectations are written from the documented order (NaN before every number, then the larger value, -0.0 == +0.0, equal
// values by the smaller id) with float compares, not from the header's bit tricks.
#include <cfloat>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../semanticlens_amd/csrc/packed_best.hpp"

using namespace sl;
using namespace sl::packed_best;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      if (++failures <= 20) {                  \
        std::printf("line %d: ", __LINE__);    \
        std::printf(__VA_ARGS__);              \
        std::printf("\n");                     \
      }                                        \
    }                                          \
  } while (0)

static float as_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
static bool is_nan(uint32_t u) { return (u & 0x7FFFFFFFu) > 0x7F800000u; }

// the documented order: -1 = a ranks before b, 0 = they rank alike, 1 = a ranks after b
static int order(uint32_t a, uint32_t b) {
  if (is_nan(a) || is_nan(b)) return is_nan(a) == is_nan(b) ? 0 : is_nan(a) ? -1 : 1;
  const float fa = as_float(a), fb = as_float(b);
  return fa > fb ? -1 : fa < fb ? 1 : 0;  // -0.0 == +0.0 as floats
}
// what an entry decodes to: -0 -> +0, any NaN -> the canonical quiet NaN
static uint32_t canonical(uint32_t u) { return is_nan(u) ? 0x7FC00000u : u == 0x80000000u ? 0u : u; }

static void check_pair(uint32_t a, uint32_t b) {
  const uint32_t ka = f32_bits_order_key(a), kb = f32_bits_order_key(b);
  const int want = order(a, b), got = ka > kb ? -1 : ka < kb ? 1 : 0;
  CHECK(got == want, "key order of %08x / %08x: keys %08x / %08x give %d, the documented order %d", a, b, ka, kb, got, want);
  // combine rule: the larger entry is the better (value, then smaller id) pair
  static const int64_t ids[] = {0, 1, 7, (int64_t)1 << 31, kMaxPackedId};
  for (int64_t ia : ids)
    for (int64_t ib : ids) {
      const uint64_t ea = pack(ka, id_low(ia)), eb = pack(kb, id_low(ib));
      const int pair_want = want ? want : ia < ib ? -1 : ia > ib ? 1 : 0;
      const int pair_got = ea > eb ? -1 : ea < eb ? 1 : 0;
      CHECK(pair_got == pair_want, "combine of (%08x, %lld) / (%08x, %lld): entries give %d, expected %d", a, (long long)ia, b,
            (long long)ib, pair_got, pair_want);
    }
}

int main() {
  const uint32_t specials[] = {
      0x00000000u, 0x80000000u,                            // +-0
      0x00000001u, 0x80000001u,                            // +-denormal minimum
      0x007FFFFFu, 0x807FFFFFu, 0x00800000u, 0x80800000u,  // largest denormal, FLT_MIN
      0x3F800000u, 0xBF800000u,                            // +-1
      0x3F7FFFFFu, 0x3F800001u, 0xBF7FFFFFu, 0xBF800001u,  // next to +-1
      bits_of(FLT_MAX), bits_of(-FLT_MAX), 0x7F800000u, 0xFF800000u,
      0x7FC00000u, 0xFFC00000u, 0x7FC12345u, 0xFFC54321u, 0x7FFFFFFFu, 0xFFFFFFFFu,  // quiet NaNs
      0x7F800001u, 0xFF800001u, 0x7FA00000u, 0xFFA0BEEFu, 0x7FBFFFFFu, 0xFFBFFFFFu,  // signalling NaNs
  };
  std::vector<uint32_t> table(specials, specials + sizeof(specials) / sizeof(specials[0]));
  uint64_t s = 0x9E3779B97F4A7C15ull;  // xorshift64*, fixed seed
  for (int i = 0; i < 4000; ++i) {
    s ^= s >> 12, s ^= s << 25, s ^= s >> 27;
    table.push_back((uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32));
  }

  for (uint32_t v : table) {
    const uint32_t key = f32_bits_order_key(v);
    CHECK(f32_order_key(as_float(v)) == key, "f32_order_key(float) of %08x differs from the key of its bits", v);
    CHECK(key >= 0x007FFFFFu, "key %08x of %08x is below -inf's: 0 would not be free for the empty entry", key, v);
    CHECK(order_key_f32_bits(key) == canonical(v), "key %08x of %08x decodes to %08x", key, v, order_key_f32_bits(key));
    for (int64_t id : {(int64_t)0, (int64_t)1, (int64_t)1 << 31, ((int64_t)1 << 32) - 2}) {
      const uint64_t e = pack(key, (uint32_t)(0xFFFFFFFFll - id));
      uint32_t bits = 1;
      int64_t got = -2;
      unpack(e, bits, got);
      CHECK(e != 0, "(%08x, %lld) packs to the empty entry", v, (long long)id);
      CHECK(bits == canonical(v) && got == id, "(%08x, %lld) comes back as (%08x, %lld)", v, (long long)id, bits, (long long)got);
    }
  }
  CHECK(f32_bits_order_key(0xFF800000u) == 0x007FFFFFu, "-inf's key is %08x", f32_bits_order_key(0xFF800000u));
  CHECK(order_key_f32_bits(0xFFFFFFFFu) == 0x7FC00000u && order_key_f32_bits(f32_bits_order_key(0x80000000u)) == 0u,
        "all ones must decode to the quiet NaN and a zero's key to +0.0");
  {
    uint32_t bits = 1;
    int64_t id = 0;
    unpack(0, bits, id);
    CHECK(bits == 0xFF800000u && id == -1, "the empty entry decodes to (%08x, %lld), expected (-inf, -1)", bits, (long long)id);
    CHECK(pack(0, 0x12345678u) == 0, "key 0 must pack to the empty entry");
  }

  // every special against the whole table, every random pattern against its neighbour
  const size_t n_special = sizeof(specials) / sizeof(specials[0]);
  for (size_t i = 0; i < n_special; ++i)
    for (uint32_t v : table) check_pair(table[i], v);
  for (size_t i = n_special; i + 1 < table.size(); ++i) check_pair(table[i], table[i + 1]);

  // the id range, at the edges tests/test_compare_host.py and tests/test_audit_host.py use
  const int64_t MAX_ID = ((int64_t)1 << 32) - 2;
  CHECK(kMaxPackedId == MAX_ID, "kMaxPackedId = %lld", (long long)kMaxPackedId);
  CHECK(!ids_fit(-1, 4) && !ids_fit(-1, 0), "a negative base must not fit");
  CHECK(!ids_fit(MAX_ID - 2, 4) && ids_fit(MAX_ID - 2, 3) && ids_fit(MAX_ID - 3, 4), "4 ids fit from MAX_ID - 3, not from MAX_ID - 2");
  CHECK(ids_fit(MAX_ID, 0) && ids_fit(MAX_ID, 1) && !ids_fit(MAX_ID, 2), "MAX_ID is the last id");
  CHECK(!ids_fit(MAX_ID + 1, 0) && ids_fit(0, MAX_ID + 1) && !ids_fit(0, MAX_ID + 2), "the range is [0, MAX_ID]");
  CHECK(id_low(0) == 0xFFFFFFFFu && id_low(MAX_ID) == 1u, "low words run from all ones down to 1");

  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
