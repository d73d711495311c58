// Host-side check of semanticlens_amd/csrc/gemm_choice.hpp: which kernel (and which cut) the GEMM launchers pick per shape.
// Built and run by tests/test_host_logic.py with g++.  The expected values were recorded from the if-chains of launch_gemm3_nt /
// launch_gemm_nt as they stood before gemm_choice.hpp existed (commit d129c81), not from this header.
#include <cstdint>
#include <cstdio>

#include "../../semanticlens_amd/csrc/gemm_choice.hpp"

using namespace sl::gemm_choice;

static int failures = 0;
static const char* const kG3Names[] = {"Reg128", "Dma256", "Phase8", "W4", "Ring64", "Ring128"};
static const char* const kF32Names[] = {"Phase8", "Vec128", "Scalar128"};

// one launch of the split-bf16 GEMM: the kernel of the whole, or (cut > 0) of columns [0, cut) and of the strip [cut, N)
struct G3Case {
  int cus, forced;
  bool strip_off;
  int64_t M, N, K;
  int64_t cut;
  G3Kernel kernel;  // cut == 0: of the whole GEMM; cut > 0: of the main part
  G3Kernel strip;   // cut > 0 only
};

static void check_g3(const G3Case& c, int line) {
  const int64_t Kp = (c.K + 31) & ~(int64_t)31;
  const G3Choice got = choose_g3(c.M, c.N, Kp, c.cus, c.forced, c.strip_off, G3Part::Whole);
  bool ok = got.cut == c.cut;
  G3Kernel main = got.kernel, strip = c.strip;
  if (ok && c.cut > 0) {
    const G3Choice m = choose_g3(c.M, c.cut, Kp, c.cus, c.forced, c.strip_off, G3Part::Main);
    const G3Choice s = choose_g3(c.M, c.N - c.cut, Kp, c.cus, c.forced, c.strip_off, G3Part::Strip);
    ok = m.cut == 0 && s.cut == 0;  // neither side of a cut is cut again
    main = m.kernel, strip = s.kernel;
  }
  if (!ok || main != c.kernel || (c.cut > 0 && strip != c.strip)) {
    std::printf("line %d: (%lld, %lld, %lld) cus=%d forced=%d: cut %lld kernel %s strip %s, expected cut %lld kernel %s strip %s\n", line,
                (long long)c.M, (long long)c.N, (long long)c.K, c.cus, c.forced, (long long)got.cut, kG3Names[(int)main],
                kG3Names[(int)strip], (long long)c.cut, kG3Names[(int)c.kernel], kG3Names[(int)c.strip]);
    ++failures;
  }
}
#define G3(...) check_g3(G3Case{__VA_ARGS__}, __LINE__)

static void check_f32(int cus, int forced, bool aligned16, int64_t M, int64_t N, int64_t K, F32Kernel want, int line) {
  const F32Kernel got = choose_f32(M, N, K, aligned16, cus, forced);
  if (got != want) {
    std::printf("line %d: f32 (%lld, %lld, %lld) cus=%d forced=%d aligned=%d: %s, expected %s\n", line, (long long)M, (long long)N,
                (long long)K, cus, forced, (int)aligned16, kF32Names[(int)got], kF32Names[(int)want]);
    ++failures;
  }
}
#define F32(...) check_f32(__VA_ARGS__, __LINE__)

int main() {
  const G3Kernel none = G3Kernel::Reg128;  // the strip field of a case without a cut
  // ---- split-bf16, 256 CUs (MI355X), by grid size
  G3(256, 0, false, 130, 257, 256, 0, G3Kernel::Ring64, none);      // 15 tiles of 64 x 64, 8 k-tiles
  G3(256, 0, false, 1, 5, 4096, 0, G3Kernel::Ring64, none);         // one tile, long k loop
  G3(256, 0, false, 2304, 1024, 256, 0, G3Kernel::Ring128, none);   // 144 tiles of 128 x 128: below half a 256 x 256 tile per CU
  G3(256, 0, false, 2304, 1024, 200, 0, G3Kernel::Reg128, none);    // the same grid with 7 k-tiles: too short for a ring
  G3(256, 0, false, 161, 257, 20, 0, G3Kernel::Reg128, none);       // one k-tile
  G3(256, 0, false, 12800, 768, 256, 0, G3Kernel::W4, none);        // 150 tiles of 256 x 256 -> 240 of 160 x 256 in one round
  G3(256, 0, false, 8192, 2048, 256, 0, G3Kernel::Phase8, none);    // 256 tiles: one round
  G3(256, 0, false, 10000, 9216, 1152, 0, G3Kernel::Phase8, none);  // 1440 tiles
  // 64 x 4.5 column tiles: cut at 1024; the 128-column strip is 512 tiles of 64 x 64 = two per CU, so it runs on the 64 x 64 ring
  G3(256, 0, false, 16384, 1152, 256, 1024, G3Kernel::Phase8, G3Kernel::Ring64);
  G3(256, 0, true, 16384, 1152, 256, 0, G3Kernel::Phase8, none);    // g3_strip_off = 1
  G3(256, 0, false, 65536, 3456, 1152, 0, G3Kernel::Phase8, none);  // 3584 tiles = 14 whole rounds: nothing to gain from a cut
  G3(256, 0, false, 65536, 4304, 1152, 0, G3Kernel::Phase8, none);  // 4352 tiles = 17 whole rounds
  // an operand of 4 GB or more: no kernel with 32-bit lane offsets
  G3(256, 0, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Dma256, none);
  G3(256, 0, false, (int64_t)1 << 20, (int64_t)1 << 20, 1152, 0, G3Kernel::Dma256, none);
  G3(256, 0, false, 65536, 65536, 16384, 0, G3Kernel::Dma256, none);  // exactly 4 GB
  // ---- other CU counts
  G3(304, 0, false, 16384, 1152, 256, 0, G3Kernel::W4, none);
  G3(304, 0, false, 12800, 768, 256, 0, G3Kernel::Ring128, none);
  G3(64, 0, false, 2304, 1024, 256, 0, G3Kernel::W4, none);
  G3(64, 0, false, 16384, 1152, 256, 512, G3Kernel::Phase8, G3Kernel::Ring128);
  G3(64, 0, false, 65536, 3456, 1152, 2816, G3Kernel::Phase8, G3Kernel::Ring128);  // the cut two full tiles early
  // ---- option g3_tile; 512 names no kernel and gets the register-staged one, like 128
  G3(256, 0, false, 300, 301, 104, 0, G3Kernel::Reg128, none);
  G3(256, 8, false, 300, 301, 104, 0, G3Kernel::Phase8, none);
  G3(256, 64, false, 300, 301, 104, 0, G3Kernel::Ring64, none);
  G3(256, 128, false, 300, 301, 104, 0, G3Kernel::Reg128, none);
  G3(256, 160, false, 300, 301, 104, 0, G3Kernel::W4, none);
  G3(256, 256, false, 300, 301, 104, 0, G3Kernel::Dma256, none);
  G3(256, 512, false, 300, 301, 104, 0, G3Kernel::Reg128, none);
  G3(256, 1280, false, 300, 301, 104, 0, G3Kernel::Ring128, none);
  G3(256, 128, false, 16384, 1152, 256, 0, G3Kernel::Reg128, none);  // a forced GEMM is not cut
  // forced onto a kernel the operand does not fit: the register-staged one; 256 x 128 has 64-bit offsets
  G3(256, 8, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Reg128, none);
  G3(256, 64, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Reg128, none);
  G3(256, 160, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Reg128, none);
  G3(256, 1280, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Reg128, none);
  G3(256, 256, false, (int64_t)1 << 20, 300, 1152, 0, G3Kernel::Dma256, none);

  // ---- fp32-input MFMA mode
  F32(256, 0, true, 8192, 2048, 256, F32Kernel::Phase8);
  F32(256, 0, true, 130, 257, 72, F32Kernel::Vec128);      // K % 4 == 0, not whole 128-byte lines
  F32(256, 0, true, 129, 128, 73, F32Kernel::Scalar128);   // K % 4 != 0
  F32(256, 0, false, 130, 257, 72, F32Kernel::Scalar128);  // an operand not 16-byte aligned
  F32(256, 0, true, 2304, 1024, 256, F32Kernel::Vec128);   // 36 tiles of 256 x 256: too few
  F32(256, 0, true, 8192, 18432, 256, F32Kernel::Phase8);  // 9 whole rounds
  F32(256, 0, true, (int64_t)1 << 20, (int64_t)1 << 20, 1152, F32Kernel::Vec128);  // operands past 4 GB
  // option f32_tile
  F32(256, 8, true, 130, 257, 64, F32Kernel::Phase8);
  F32(256, 8, true, 130, 257, 72, F32Kernel::Vec128);        // 8 forced, rows are not whole lines
  F32(256, 8, false, 8192, 2048, 256, F32Kernel::Scalar128);  // 8 forced, unaligned operand
  F32(256, 128, true, 8192, 2048, 256, F32Kernel::Vec128);

  // ---- the predicates on their own
  if (fits(65536, 65536, 65536) || !fits(65536, 65536, 65535) || tiles_of(257, 256) != 2 || !worth_it(2304, 3840, 256) ||
      worth_it(2304, 3584, 256) || strip_split_columns(16384, 1152, 256, false) != 1024 || strip_split_columns(16384, 1152, 256, true) != 0) {
    std::printf("line %d: predicate\n", __LINE__);
    ++failures;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
