// Host-side check of the pure part of semanticlens_amd/csrc/rowseg_tile.hpp: how K17, K25 and K26 split a row over waves, which
// columns a segment holds, and where a wave's walk starts.  Built and run by tests/test_host_logic.py with g++.
// The split table was recorded from the three kernels' own (identical) splits() before the header took it over.
#include <cstdint>
#include <cstdio>

#include "../../semanticlens_amd/csrc/rowseg_tile.hpp"

using namespace sl::rowseg;

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

struct Split {
  int64_t R, B, S;
};

static void check_splits(int64_t cus, const Split* table, int n) {
  for (int i = 0; i < n; ++i) {
    const int64_t got = splits(table[i].R, table[i].B, cus);
    CHECK(got == table[i].S, "splits(%lld, %lld, %lld) = %lld, recorded %lld", (long long)table[i].R, (long long)table[i].B,
          (long long)cus, (long long)got, (long long)table[i].S);
  }
}

int main() {
  // ---- split table: R <= 0; B = 2047 / 2048; R = 8 cus and one below; the `want`-bound row of 2^26 columns; many rows of few
  // columns (tests/test_label_distribution_host.py pins that one through the library); and a few points between
  static const int64_t M = 1 << 20;
  static const Split t64[] = {{0, M, 1},   {-3, M, 1},          {1, 2047, 1}, {1, 2048, 2},   {1, 4096, 4},   {512, M, 1},        {511, M, 2},
                              {1, 1 << 26, 512}, {1, M, 512}, {7, 50000, 48}, {3, M, 171}, {100000, 341, 1}, {100, 5000, 4}, {64, 16384, 8}};
  static const Split t256[] = {{0, M, 1},   {-3, M, 1},           {1, 2047, 1}, {1, 2048, 2},   {1, 4096, 4},   {2048, M, 1},       {2047, M, 2},
                               {1, 1 << 26, 2048}, {1, M, 1024}, {7, 50000, 48}, {3, M, 683}, {100000, 341, 1}, {100, 5000, 4}, {256, 16384, 8}};
  static const Split t304[] = {{0, M, 1},   {-3, M, 1},           {1, 2047, 1}, {1, 2048, 2},   {1, 4096, 4},   {2432, M, 1},       {2431, M, 2},
                               {1, 1 << 26, 2432}, {1, M, 1024}, {7, 50000, 48}, {3, M, 811}, {100000, 341, 1}, {100, 5000, 4}, {304, 16384, 8}};
  check_splits(64, t64, sizeof(t64) / sizeof(t64[0]));
  check_splits(256, t256, sizeof(t256) / sizeof(t256[0]));
  check_splits(304, t304, sizeof(t304) / sizeof(t304[0]));
  static_assert(kMinSegment == 1024 && kChunk == 1024, "the segment floor and the chunk width are part of the recorded table");

  // ---- segment cover: the S segments hold every column of [0, B) exactly once, in order; only trailing ones may be empty
  static const int64_t widths[] = {1, 3, 1023, 1024, 1025, 2048, 2049, 5000, M + 7};
  for (int64_t B : widths) {
    int64_t s_max = B / 1024 < 40 ? B / 1024 : 40;
    if (s_max < 1) s_max = 1;  // S = 1 is always a launch
    for (int64_t S = 1; S <= s_max; ++S) {
      const int64_t seg = segment(B, S);
      CHECK(S > 1 || seg == B, "segment(%lld, 1) = %lld", (long long)B, (long long)seg);
      CHECK(seg == (B + S - 1) / S, "segment(%lld, %lld) = %lld", (long long)B, (long long)S, (long long)seg);
      int64_t next = 0;  // the first column no segment has held yet
      bool seen_empty = false;
      for (int64_t s = 0; s < S; ++s) {
        const Bounds b = segment_bounds(s, seg, B);
        CHECK(b.hi - b.lo <= seg && b.hi <= B, "B %lld S %lld s %lld: [%lld, %lld) is wider than seg %lld or passes B", (long long)B,
              (long long)S, (long long)s, (long long)b.lo, (long long)b.hi, (long long)seg);
        if (b.hi <= b.lo) {
          seen_empty = true;
          continue;
        }
        CHECK(!seen_empty, "B %lld S %lld: segment %lld holds columns after an empty one", (long long)B, (long long)S, (long long)s);
        CHECK(b.lo == next, "B %lld S %lld: segment %lld starts at %lld, the columns so far end at %lld", (long long)B, (long long)S,
              (long long)s, (long long)b.lo, (long long)next);
        next = b.hi;
      }
      CHECK(next == B, "B %lld S %lld: the segments end at %lld", (long long)B, (long long)S, (long long)next);
    }
  }

  // ---- chunk start: at most three columns before lo, on a 16-byte boundary, for a row that starts 0..3 elements past one
  for (uintptr_t off = 0; off < 4; ++off) {
    const uintptr_t row_addr = 0x10000 + 4 * off;  // the address of column 0
    static const int64_t los[] = {0, 1, 5, 1024};
    for (int64_t lo : los) {
      const int64_t a0 = chunk_start(row_addr + 4 * (uintptr_t)lo, lo);
      CHECK(a0 <= lo && lo - a0 < 4, "offset %d lo %lld: the walk starts at %lld", (int)off, (long long)lo, (long long)a0);
      CHECK(((row_addr + 4 * (uintptr_t)a0) & 15) == 0, "offset %d lo %lld: column %lld is not on a 16-byte boundary", (int)off,
            (long long)lo, (long long)a0);  // a0 may be negative: the unsigned sum wraps to the right address
    }
  }

  // ---- grid: min(items, cus * waves per CU * 4)
  CHECK(wave_grid(5, 256, 32) == 5 && wave_grid(1 << 20, 256, 32) == 256 * 32 * 4 && wave_grid(256 * 4, 256, 1) == 256 * 4 &&
            wave_grid(256 * 4 + 1, 256, 1) == 256 * 4,
        "wave_grid caps at four items per wave slot");

  std::printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
