// Host-side check of semanticlens_amd/csrc/gemm_choice.hpp, the two rules of the split-bf16 launcher side by side: by makespan on an
// empty chip (the default, as tests/native/gemm_choice_check.cpp pins it) and by chip time for a launch that shares the GPU with
// another stream (option g3_shared).  Built and run by tests/test_gemm_choice_shared.py with g++.
// The expected values are worked out by hand from the rules' statements: a launch of w workgroups of time t costs w x t; a
// 160 x 256 tile takes 0.85 of a 256 x 256 tile's time, a 128 x 128 ring tile 0.40; 160-row tiles are
// chosen only where items x t160 < tiles x t256, a cut only where its summed chip time is below the uncut launch's.
#include <cstdint>
#include <cstdio>

#include "../../semanticlens_amd/csrc/gemm_choice.hpp"

using namespace sl::gemm_choice;

static int failures = 0;
static const char* const kG3Names[] = {"Reg128", "Dma256", "Phase8", "W4", "Ring64", "Ring128"};

// what one rule makes of a GEMM: the kernel of the whole, or (cut > 0) of columns [0, cut) and of the strip [cut, N)
struct Want {
  int64_t cut;
  G3Kernel kernel;  // cut == 0: of the whole GEMM; cut > 0: of the main part
  G3Kernel strip;   // cut > 0 only
};

static void check_rule(int cus, int forced, int64_t M, int64_t N, int64_t K, bool shared, const Want& w, int line) {
  const int64_t Kp = (K + 31) & ~(int64_t)31;
  const G3Choice got = choose_g3(M, N, Kp, cus, forced, false, G3Part::Whole, shared);
  bool ok = got.cut == w.cut;
  G3Kernel main = got.kernel, strip = w.strip;
  if (ok && w.cut > 0) {
    const G3Choice m = choose_g3(M, w.cut, Kp, cus, forced, false, G3Part::Main, shared);
    const G3Choice s = choose_g3(M, N - w.cut, Kp, cus, forced, false, G3Part::Strip, shared);
    ok = m.cut == 0 && s.cut == 0;  // neither side of a cut is cut again
    main = m.kernel, strip = s.kernel;
  }
  if (!ok || main != w.kernel || (w.cut > 0 && strip != w.strip)) {
    std::printf("line %d: (%lld, %lld, %lld) cus=%d forced=%d %s rule: cut %lld kernel %s strip %s, expected cut %lld kernel %s strip %s\n",
                line, (long long)M, (long long)N, (long long)K, cus, forced, shared ? "chip-time" : "makespan", (long long)got.cut,
                kG3Names[(int)main], kG3Names[(int)strip], (long long)w.cut, kG3Names[(int)w.kernel], kG3Names[(int)w.strip]);
    ++failures;
  }
}
// one shape under both rules: {cus, forced, M, N, K}, the makespan rule's choice, the chip-time rule's choice
#define BOTH(cus, forced, M, N, K, alone, shared)                    \
  do {                                                               \
    check_rule(cus, forced, M, N, K, false, Want alone, __LINE__);   \
    check_rule(cus, forced, M, N, K, true, Want shared, __LINE__);   \
  } while (0)

int main() {
  const G3Kernel none = G3Kernel::Reg128;  // the strip field of a case without a cut
  const G3Kernel P8 = G3Kernel::Phase8, W4 = G3Kernel::W4, R64 = G3Kernel::Ring64, R128 = G3Kernel::Ring128;

  // ---- the four GEMMs of a ViT-B/32 block at 256 images (M = 12 800 token rows), 256 CUs: sharing, every one is the 8-phase kernel, uncut
  // qkv: 450 tiles against 720 items x 0.85 = 612; no partial column tile, and a cut at 2048 costs 400 + 0.40 x 200 = 480 > 450
  BOTH(256, 0, 12800, 2304, 768, ({0, P8, none}), ({0, P8, none}));
  // out-projection: 150 tiles in one round; 240 items of 160 rows save the makespan 20 % and cost 240 x 0.85 = 204 > 150 of chip time
  BOTH(256, 0, 12800, 768, 768, ({0, W4, none}), ({0, P8, none}));
  // fc1: 600 tiles = 2.34 rounds; alone 500 tiles (1.95 rounds) + a 512-column strip of 400 small tiles is shorter, sharing it costs
  // 500 + 0.40 x 400 = 660 > 600
  BOTH(256, 0, 12800, 3072, 768, ({2560, P8, R128}), ({0, P8, none}));
  // fc2: as the out-projection with four times the k loop
  BOTH(256, 0, 12800, 768, 3072, ({0, W4, none}), ({0, P8, none}));
  // the patch embedding (49 patches of 3 x 32 x 32 per image): 147 tiles against 237 items x 0.85 = 201
  BOTH(256, 0, 12544, 768, 3072, ({0, W4, none}), ({0, P8, none}));

  // ---- SigLIP-so400m's out-projection at 64 images (N = 1152 = 4.5 column tiles): the cut pays under both rules, 256 + 0.40 x 128 =
  // 307 < 320 tiles; the 128-column strip is 512 tiles of 64 x 64 = two per CU and stays on the 64 x 64 ring
  BOTH(256, 0, 16384, 1152, 1152, ({1024, P8, R64}), ({1024, P8, R64}));
  // a partial column tile wider than 128 columns is no cheaper cut off: 4 x 0.40 > 1 per row tile (N = 1216: 64 x 4 + 0.40 x 256 = 358 > 320)
  check_rule(256, 0, 16384, 1216, 1152, true, Want{0, P8, none}, __LINE__);

  // ---- other CU counts
  // 304 CUs: 320 tiles are two rounds, 515 items of 160 rows are two shorter ones; sharing, 515 x 0.85 = 438 > 320 and the cut pays
  BOTH(304, 0, 16384, 1152, 256, ({0, W4, none}), ({1024, P8, R64}));
  BOTH(304, 0, 12800, 3072, 768, ({0, P8, none}), ({0, P8, none}));  // 600 tiles: 1.99 rounds, no cut helps
  // 64 CUs: 36 tiles against 60 items x 0.85 = 51
  BOTH(64, 0, 2304, 1024, 256, ({0, W4, none}), ({0, P8, none}));
  // 64 CUs, 320 tiles = 5 rounds: alone the cut falls two tiles early (128 tiles = two whole rounds), sharing it falls at the last full tile
  BOTH(64, 0, 16384, 1152, 256, ({512, P8, R128}), ({1024, P8, R128}));

  // ---- below half a 256 x 256 tile per CU neither big-tile rule applies: both rules agree
  BOTH(256, 0, 130, 257, 256, ({0, R64, none}), ({0, R64, none}));
  BOTH(256, 0, 1, 5, 4096, ({0, R64, none}), ({0, R64, none}));
  BOTH(256, 0, 2304, 1024, 256, ({0, R128, none}), ({0, R128, none}));           // 36 tiles
  BOTH(256, 0, 2304, 1024, 200, ({0, G3Kernel::Reg128, none}), ({0, G3Kernel::Reg128, none}));
  BOTH(256, 0, 10752, 768, 768, ({0, R128, none}), ({0, R128, none}));           // 126 tiles: the last row count below half a tile per CU
  BOTH(304, 0, 12800, 768, 768, ({0, R128, none}), ({0, R128, none}));           // 150 tiles on 304 CUs
  // the first shape above it: 129 tiles, 207 items of 160 rows
  BOTH(256, 0, 11008, 768, 768, ({0, W4, none}), ({0, P8, none}));

  // ---- where 160-row tiles are fewer items than their time ratio they are kept: M = 320 is two row tiles either way, 256 x 0.85 < 256
  BOTH(256, 0, 320, 32768, 768, ({0, W4, none}), ({0, W4, none}));
  // ---- a forced kernel and an operand past 32-bit offsets do not depend on the rule
  BOTH(256, 160, 12800, 768, 768, ({0, W4, none}), ({0, W4, none}));
  BOTH(256, 1280, 12800, 3072, 768, ({0, R128, none}), ({0, R128, none}));
  BOTH(256, 0, (int64_t)1 << 20, 300, 1152, ({0, G3Kernel::Dma256, none}), ({0, G3Kernel::Dma256, none}));
  // g3_strip_off = 1 under the chip-time rule
  if (choose_g3(16384, 1152, 1152, 256, 0, true, G3Part::Whole, true).cut != 0) {
    std::printf("line %d: strip_off\n", __LINE__);
    ++failures;
  }
  // the trailing parameter defaults to the makespan rule
  {
    const G3Choice a = choose_g3(12800, 768, 768, 256, 0, false, G3Part::Whole);
    const G3Choice b = choose_g3(12800, 768, 768, 256, 0, false, G3Part::Whole, false);
    if (a.kernel != W4 || b.kernel != W4 || a.cut != 0 || b.cut != 0) {
      std::printf("line %d: default rule\n", __LINE__);
      ++failures;
    }
  }

  // ---- the predicates on their own
  if (w4_prefer_shared(12800, 768, 256) || !w4_prefer_shared(320, 32768, 256) || w4_prefer_shared(320, 768, 256) ||
      strip_split_columns_shared(16384, 1152, false) != 1024 || strip_split_columns_shared(16384, 1152, true) != 0 ||
      strip_split_columns_shared(12800, 3072, false) != 0 || strip_split_columns_shared(12800, 200, false) != 0) {
    std::printf("line %d: predicate\n", __LINE__);
    ++failures;
  }
  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
