// Host-side table of semanticlens_amd/csrc/biased_score.hpp: prints, per line, the bits of c, r, q and of biased_score(c, r, q)
// for every triple of the operand table below (finite operands stay below 2^127, the header's domain).  Built twice by
// tests/test_hubness_host.py (-ffp-contract=off and -ffp-contract=fast), which compares the two outputs with each other and with
// numpy's fp32 arithmetic.  The operands are read through a volatile so that the compiler evaluates the rule at run time, in the
// arithmetic its flags select.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../semanticlens_amd/csrc/biased_score.hpp"

static const uint32_t kOperands[] = {
    0x00000000u,  // +0.0
    0x80000000u,  // -0.0
    0x3F800000u,  // 1.0
    0xBF800000u,  // -1.0
    0x3F000000u,  // 0.5
    0x3E800001u,  // 0.25 + 1 ulp
    0x3F7FFFFFu,  // 1 - 2^-24
    0x3EAAAAABu,  // 1/3
    0xBF2AAAABu,  // -2/3
    0x3DCCCCCDu,  // 0.1
    0x00000001u,  // the smallest denormal
    0x80000001u,  // its negative
    0x007FFFFFu,  // the largest denormal
    0x00800000u,  // the smallest normal
    0x00400001u,  // a denormal whose double is normal
    0x7E7FFFFFu,  // just under 2^126: the largest magnitudes whose double is finite (the header's domain)
    0xFE7FFFFFu,
    0x7F800000u,  // +inf
    0xFF800000u,  // -inf
    0x7FC00000u,  // NaN
    0x4B800001u,  // 2^24 + 2: c - r cancellations at large magnitude
    0x4B800000u,
    0x33800000u,  // 2^-24
};

static float from_bits(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  const int n = (int)(sizeof(kOperands) / sizeof(kOperands[0]));
  volatile float vc, vr, vq;
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b)
      for (int d = 0; d < n; ++d) {
        vc = from_bits(kOperands[a]), vr = from_bits(kOperands[b]), vq = from_bits(kOperands[d]);
        const float c = vc, r = vr, q = vq;
        std::printf("%08x %08x %08x %08x\n", kOperands[a], kOperands[b], kOperands[d], bits_of(sl::biased_score(c, r, q)));
      }
  return 0;
}
