// The packed "best so far" entry of K20 (mutualmax.hip) and K22 (segmax.hip) and the fp32 order key under it (K17, topk.hip,
// ranks by the same key), as pure functions.  Needs only <cstdint>: a host compiler can include it
// (tests/native/packed_best_check.cpp holds the table), and the functions are constexpr, which hipcc takes as host and device.
// Order: NaN before every number, then the larger value, -0.0 == +0.0, equal values by the smaller id.
// Entry: one uint64, (f32_order_key(value) << 32) | (0xFFFFFFFF - id); 0 is the empty entry (every real value's key is
// >= 0x007FFFFF).  Under this packing "better" is the plain unsigned maximum, which is associative and commutative: whatever
// the order in which lanes, waves, workgroups, tiles and the memory side's 64-bit atomic max combine the entries, a state is
// the maximum of the set of entries seen, bit for bit.  Ids are limited to [0, 2^32 - 2].  The packing carries neither the sign
// of a zero nor a NaN's payload: a decoded +-0.0 is +0.0, a decoded NaN is the canonical quiet NaN (0x7FC00000).
#pragma once
#include <cstdint>

namespace sl {

// monotone 32-bit key of an fp32: larger key == ranks earlier.  NaN -> all ones, -0.0 -> +0.0's key; every real value's key
// is >= 0x007FFFFF (-inf), so 0 is free for the empty slot (K17's slots, the packed entries below)
constexpr uint32_t f32_bits_order_key(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;
  if (u == 0x80000000u) return 0x80000000u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
constexpr uint32_t f32_order_key(float v) { return f32_bits_order_key(__builtin_bit_cast(uint32_t, v)); }

// the inverse, as fp32 bits: NaN -> the canonical quiet NaN; the keys of +0.0 and -0.0 coincide and decode as +0.0
constexpr uint32_t order_key_f32_bits(uint32_t key) {
  return key == 0xFFFFFFFFu ? 0x7FC00000u : (key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key;
}

namespace packed_best {

constexpr int64_t kMaxPackedId = 0xFFFFFFFEll;  // 2^32 - 1 is left out: its low word would be 0

// the low word of an id; an id `d` further on has the low word `id_low(id) - d`
constexpr uint32_t id_low(int64_t id) { return (uint32_t)(0xFFFFFFFFll - id); }

// key 0 (no value seen) packs to the empty entry whatever the low word
constexpr uint64_t pack(uint32_t key, uint32_t low) { return key ? ((uint64_t)key << 32) | low : 0ull; }

// (value bits, id) of an entry; the empty entry is (-inf, -1), K17's empty slot
constexpr void unpack(uint64_t entry, uint32_t& value_bits, int64_t& id) {
  value_bits = entry ? order_key_f32_bits((uint32_t)(entry >> 32)) : 0xFF800000u;
  id = entry ? (int64_t)(0xFFFFFFFFu - (uint32_t)entry) : -1;
}

// do the n ids from `base` on stay inside [0, kMaxPackedId]?
constexpr bool ids_fit(int64_t base, int64_t n) { return base >= 0 && base <= kMaxPackedId && n <= kMaxPackedId + 1 - base; }

}  // namespace packed_best
}  // namespace sl
