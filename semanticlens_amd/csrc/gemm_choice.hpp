// Which MFMA GEMM kernel a shape gets: the size rules of the split-bf16 launcher (choose_g3, for gemm_bf16x3.hpp) and of the fp32
// launcher (choose_f32, for gemm_f32.hpp) as pure functions of the shape, the CU count and the option values.
// Needs only <cstdint>: a host compiler can include it (tests/native/gemm_choice_check.cpp holds the table, and
// tests/native/gemm_choice_shared_check.cpp the one of choose_g3's two rules side by side).
// Every kernel of a family gives the same bits (tests/test_gpu_parity.py); the rules below only decide speed.
#pragma once
#include <cstdint>

namespace sl {
namespace gemm_choice {

// ---- predicates ----------------------------------------------------------------------------------------------------------
// the LDS-DMA ring kernels (8-phase, w4, ring) address an operand with 32-bit lane offsets
inline bool fits(int64_t M, int64_t N, int64_t row_bytes) { return (M > N ? M : N) * row_bytes < (1ll << 32); }
// 256 x 256 tiles
inline int64_t tiles_of(int64_t M, int64_t N) { return ((M + 255) / 256) * ((N + 255) / 256); }

// the 8-phase kernel from half a tile per CU upwards (the encoder's 150-600-tile GEMMs gain, ViT-B/32 image encode
// 9.66 -> 9.08 ms)
inline bool worth_it(int64_t M, int64_t N, int64_t cus) { return tiles_of(M, N) * 2 >= cus; }

// fp32-input MFMA mode: a tile takes 5.3x longer than in bf16x3 mode and the 128 x 128 kernel reaches 0.76-0.83 of peak on
// its own, so the big kernel only pays when its last round is nearly full or there is a single round
// (tools/native/gemm3_lab, K = 1152: 150 tiles 84 vs 79 TFLOP/s, 600 tiles 112 vs 120, 1280 tiles 140 vs 126, 1440 tiles
// 132 vs 123).
inline bool worth_it_f32(int64_t M, int64_t N, int64_t cus) {
  if (!worth_it(M, N, cus)) return false;
  const int64_t t = tiles_of(M, N);
  const int64_t rounds = (t + cus - 1) / cus;
  return rounds == 1 || t * 10 >= rounds * cus * 9;
}

// gemm_w4.hpp: 160-row tiles when they shorten the makespan: rounds x tile time.  A 160 x 256 tile does 0.625 of the work of a
// 256 x 256 one and measures 0.80 (K = 768) to 0.87 (K = 3072) of its time (tools/enc_gemm_lab.py, bare epilogue: o-proj
// 51 -> 41 us, fc2 147 -> 128 us), so it is chosen only where a whole round is saved.
inline bool w4_prefer(int64_t M, int64_t N, int64_t cus) {
  const int64_t t256 = tiles_of(M, N), t160 = ((M + 159) / 160) * ((N + 255) / 256);
  if (t256 * 2 < cus) return false;  // small grids stay on the 128 x 128 kernel's side of the choice
  const double c256 = (double)((t256 + cus - 1) / cus);
  const double c160 = (double)((t160 + cus - 1) / cus) * 0.88;
  return c160 < c256 * 0.97;
}

// gemm_skinny.hpp, 64 x 64 tiles: up to two of them per CU, k loops (ns k-tiles of 32) long enough for the ring to matter;
// beyond that the 128 x 128 instance is as fast or faster.  Measured on the ViT-B/32 block shapes (tools/enc_gemm_lab.py <M>,
// SL_OPTIONS=g3_tile= 64 / 1280 / 128 = that kernel / its 128 x 128 instance / the register-staged 128 x 128 kernel), us:
//   M =   256: o-proj  8 /  - / 30, fc2 22 /  - / 90, qkv  9 /  - / 30, fc1  9 /  - / 35
//   M = 1 600: o-proj 19 / 29 / 32, fc2 48 / 68 / 89 (300 tiles); qkv 34 / 29 / 33 (900), fc1 47 / 50 / 53 (1 200)
//   M = 3 200: o-proj 28 / 24 / 36, fc2 74 / 67 / 95 (600 tiles); qkv 67 / 45 / 50, fc1 88 / 69 / 73
inline bool ring_prefer(int64_t M, int64_t N, int64_t ns, int64_t cus) {
  const int64_t t64 = ((M + 63) / 64) * ((N + 63) / 64);
  return t64 <= 2 * cus && ns >= 8;
}

// ---- column-strip split (round 5) ----------------------------------------------------------------------------------------
// The 256 x 256 kernel runs whole rounds of tiles; a trailing partial column tile (N = 1152 = 4.5 tiles: SigLIP-so400m's o-proj and
// fc2) costs a whole extra column of tiles, and with 64 row tiles (a 64-image call) 320 tiles are 1.25 rounds that take 1.77.  When
// the model below says so, the GEMM is cut at the last full column tile: columns [0, 256 n) keep the big kernel (256 tiles = ONE
// round) and the remainder strip — the same A, B rows from 256 n on, the epilogue shifted by 256 n columns — goes to whatever the
// grid-size rules pick for a strip that narrow (128 x 128 tiles, or the 64 x 64 ring).  Every output element keeps its accumulation
// order (all tile variants are bit-identical), so results do not change.  Measured (`tools/gemm_strip_lab.py`, profiles/r05_gemm_strip_lab.txt):
// M = 16 384: o-proj 173 -> 98 + 31 us, fc2 514 -> 310 + 96 us; M = 65 536: 495 -> 384 + 80, 1 523 -> 1 194 + 257.
// The cut may also fall one or two FULL tiles earlier when that lands the big kernel on whole rounds.
// Cost model, in rounds of the big kernel: t tiles cost floor(t / CUs) + (0.7 + 0.3 f) for a partial round filling a fraction f of
// the CUs; a strip of s 128 x 128 tiles costs 0.12 + 0.0014 s.  Option g3_strip_off = 1 switches the split off.
inline double g8_rounds_model(int64_t tiles, int64_t cus) {
  const int64_t full = tiles / cus, rem = tiles % cus;
  return (double)full + (rem ? 0.7 + 0.3 * (double)rem / (double)cus : 0.0);
}
// the column at which to cut, 0 = no cut
inline int64_t strip_split_columns(int64_t M, int64_t N, int64_t cus, bool strip_off) {
  const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256;
  if (strip_off || tn < 2) return 0;
  const double whole = g8_rounds_model(tm * tn, cus);
  // cut after m full column tiles, the strip up to three tiles wide: so400m's QKV at 64 images (N = 3456 = 13.5 tiles, 896 tiles =
  // 3.5 rounds) runs 12 column tiles in exactly three rounds and a 384-column strip
  int64_t best_m = 0;
  double best = 0.97 * whole;
  for (int64_t m = tn - 1; m >= 1 && m >= tn - 3; --m) {
    const int64_t rest = N - m * 256;
    const int64_t strip_tiles = ((M + 127) / 128) * ((rest + 127) / 128);
    const double cut = g8_rounds_model(tm * m, cus) + 0.12 + 0.0014 * (double)strip_tiles;
    if (cut < best) best = cut, best_m = m;
  }
  return best_m * 256;
}

// ---- a launch that shares the chip (option g3_shared) ------------------------------------------------------------------------
// Every rule above prices a launch by its makespan on an otherwise empty chip.  A big-tile workgroup owns its CU (the 8-phase kernel
// takes the whole register file, the 160 x 256 kernel the whole LDS), so when another stream has work queued the two streams take
// turns on whole CUs: CUs a launch leaves idle run the other stream, and what the launch costs the step is its CHIP TIME, workgroups
// x time per workgroup.  Per-workgroup times in units of one 256 x 256 tile of the 8-phase kernel, measured on the ViT-B/32 block
// shapes at M = 12 800 with no other stream (tools/enc_gemm_lab.py 12800, SL_OPTIONS=g3_tile= 8 / 160 / 1280;
// profiles/k11_shared_gemm_ratios.txt), us, bare epilogue / the block's own epilogue:
//   160 x 256 tile (0.625 of the work), one round of 240 items against one round of 150 tiles:
//     o-proj (K = 768) 43.4 / 51.9 against 51.3 / 60.2 = 0.85 / 0.86;  fc2 (K = 3072) 135.1 / 141.8 against 158.3 / 167.7 = 0.85 / 0.85
//   128 x 128 ring tile (0.25 of the work), one workgroup per CU:
//     fc1 2 400 tiles = 10 rounds in 210.6 against 600 tiles = 3 rounds in 161.5: 21.1 against 53.8 = 0.39
//     o-proj 600 tiles = 3 rounds in 65.0 against one round in 51.3: 21.7 against 51.3 = 0.42
// So 160-row tiles only pay where the rows quantise to as many items as tiles (M <= 160, or 256 < M <= 320), and a cut only where the
// strip is at most 128 columns wide (2 x 0.40 per row tile against 1).
constexpr double kW4TileTime = 0.85;
constexpr double kRing128TileTime = 0.40;
inline bool w4_prefer_shared(int64_t M, int64_t N, int64_t cus) {
  const int64_t t256 = tiles_of(M, N), t160 = ((M + 159) / 160) * ((N + 255) / 256);
  if (t256 * 2 < cus) return false;  // small grids: as w4_prefer
  return (double)t160 * kW4TileTime < (double)t256;
}
// the column at which to cut, 0 = no cut: the candidates of strip_split_columns, priced in tiles instead of rounds
inline int64_t strip_split_columns_shared(int64_t M, int64_t N, bool strip_off) {
  const int64_t tm = (M + 255) / 256, tn = (N + 255) / 256;
  if (strip_off || tn < 2) return 0;
  int64_t best_m = 0;
  double best = (double)(tm * tn);
  for (int64_t m = tn - 1; m >= 1 && m >= tn - 3; --m) {
    const int64_t rest = N - m * 256;
    const int64_t strip_tiles = ((M + 127) / 128) * ((rest + 127) / 128);
    const double cut = (double)(tm * m) + kRing128TileTime * (double)strip_tiles;
    if (cut < best) best = cut, best_m = m;
  }
  return best_m * 256;
}

// ---- split-bf16 (gemm_bf16x3.hpp: launch_gemm3_nt) -------------------------------------------------------------------------
enum class G3Kernel {
  Reg128,   // gemm3_nt_kernel: 128 x 128 tiles staged through registers
  Dma256,   // gemm3_nt_dma256_kernel: 256 x 128 tiles, LDS-DMA, single buffer
  Phase8,   // gemm8::gemm_nt_8phase_kernel<MODE_BF16X3>: 256 x 256
  W4,       // gemmw4::gemm3_nt_w4_kernel<5>: 160 x 256
  Ring64,   // gemmsk::gemm3_nt_skinny_kernel<1>: 64 x 64, eight-slot ring
  Ring128,  // gemmsk::gemm3_nt_skinny_kernel<2>: 128 x 128, four-slot ring
};
// which part of a GEMM a launch covers: all of it (a strip may be cut off), or one side of a cut (neither is cut again)
enum class G3Part { Whole, Main, Strip };
struct G3Choice {
  G3Kernel kernel;  // meaningful when cut == 0
  int64_t cut;      // > 0: columns [0, cut) run as G3Part::Main, columns [cut, N) as G3Part::Strip
};

// A (M rows), B (N rows): split matrices of Kp (a multiple of 32) columns; `forced` = option g3_tile, 0 = by grid size;
// `shared`: the launch shares the chip with another stream, so the two big-tile choices (160-row tiles, the strip cut) go by chip
// time instead of makespan; the small-grid rules are the same either way
inline G3Choice choose_g3(int64_t M, int64_t N, int64_t Kp, int64_t cus, int forced, bool strip_off, G3Part part,
                          bool shared = false) {
  const int64_t ns = Kp / 32;             // k-tiles
  const bool fit = fits(M, N, 4 * Kp);    // a row of a split matrix is 2 Kp bf16 = 4 Kp bytes, one 128-byte line per k-tile
  if (forced) {
    // g3_tile = 8 / 160 / 64 / 1280 / 256 / 128 names a kernel and is never cut.  A value that names none (g3_tile = 512, once
    // the ping-pong kernel) is NOT rejected: like 128, and like a ring kernel whose offsets the operand does not fit, it gets Reg128.
    if (fit && forced == 64) return {G3Kernel::Ring64, 0};
    if (fit && forced == 1280) return {G3Kernel::Ring128, 0};
    if (fit && forced == 160) return {G3Kernel::W4, 0};
    if (fit && forced == 8) return {G3Kernel::Phase8, 0};
    return {forced == 256 ? G3Kernel::Dma256 : G3Kernel::Reg128, 0};
  }
  const bool ring64 = fit && ring_prefer(M, N, ns, cus);  // small grids with long k loops
  // 150-tile GEMMs of the encoder: 240 items in one round (on a shared chip: 240 items x 0.85 against 150 tiles, so not there)
  const bool w4 = fit && (shared ? w4_prefer_shared(M, N, cus) : w4_prefer(M, N, cus));
  const bool big = fit && worth_it(M, N, cus);
  const bool ring128 = fit && ns >= 8;
  // a strip is priced as 128 x 128 tiles and runs as such unless the 64 x 64 ring wants it: no big-tile rule applies to it
  if (part == G3Part::Strip && ring128 && !ring64) return {G3Kernel::Ring128, 0};
  if (part == G3Part::Whole && big && !w4 && !ring64) {
    const int64_t c0 = shared ? strip_split_columns_shared(M, N, strip_off) : strip_split_columns(M, N, cus, strip_off);
    if (c0 > 0) return {G3Kernel::Phase8, c0};
  }
  if (ring64) return {G3Kernel::Ring64, 0};
  if (w4) return {G3Kernel::W4, 0};
  if (big) return {G3Kernel::Phase8, 0};
  // without the ring: 256 x 128 tiles from 8 of them per CU
  if (((M + 255) / 256) * ((N + 127) / 128) >= 8 * cus) return {G3Kernel::Dma256, 0};
  // mid-size grids: 128 x 128 tiles behind the four-stage LDS-DMA ring (5-30 % under the register-staged kernel from 450 to
  // 2 400 tiles, equal at 4 800; tools/enc_gemm_lab.py <M> with SL_OPTIONS=g3_tile= 128 / 1280)
  if (ring128) return {G3Kernel::Ring128, 0};
  return {G3Kernel::Reg128, 0};
}

// ---- fp32-input MFMA (gemm_f32.hpp: launch_gemm_nt) ------------------------------------------------------------------------
enum class F32Kernel {
  Phase8,     // gemm8::gemm_nt_8phase_kernel<MODE_F32>: large grids whose rows are whole 128-byte lines
  Vec128,     // gemm::gemm_nt_kernel<true>: 128 x 128, 16-byte loads
  Scalar128,  // gemm::gemm_nt_kernel<false>
};
// `forced` = option f32_tile: 8 / 128 force the 8-phase / the 128 x 128 kernel where the shape allows, 0 = by grid size
inline F32Kernel choose_f32(int64_t M, int64_t N, int64_t K, bool aligned16, int64_t cus, int forced) {
  const bool vec = K % 4 == 0 && aligned16;
  if (vec && K % 32 == 0 && K > 0 && fits(M, N, K * 4) && (forced ? forced == 8 : worth_it_f32(M, N, cus))) return F32Kernel::Phase8;
  return vec ? F32Kernel::Vec128 : F32Kernel::Scalar128;
}

}  // namespace gemm_choice
}  // namespace sl
