// The row path that K17 (topk.hip), K25 (softmax.hip) and K26 (rank.hip) share: how the rows of a cosine tile are cut into
// one-wave work items, how a wave walks its row segment, and the host side of a launch.  The row family's counterpart of
// colmax_tile.hpp.
//
// One wavefront (a 64-thread workgroup) owns item w = row * S + s: columns [lo, hi) of one row of a row-major fp32 tile (R,B),
// the s-th of the row's S segments of seg = ceil(B / S) columns (a trailing segment can be empty).  S > 1 only for few rows of
// very many columns (splits).  The wave walks its segment in chunks of kChunk = 1024 columns, 16 per lane in four 16-byte pieces
// at 16-byte aligned addresses: the walk starts at chunk_start, up to three columns before lo, and load_chunk reads a piece that
// is not wholly inside [lo, hi) element by element, so nothing outside the segment is touched and the columns outside it read
// as `pad`.  K17 and K25 call load_chunk (their chunk loops compile to the instructions they had with the load written out, in
// the same registers' worth).  K26 keeps its load written out, the wave-uniform fast path and the guarded edge branch both: with
// load_chunk at the edges and the keys converted afterwards rank_tile_kernel<1> went from 85 to 106 VGPRs and the other two
// instances changed their fast path.
//
// The first part needs only <cstdint>: a host compiler can include it (tests/native/rowseg_tile_check.cpp holds the tables), and
// the functions are constexpr, which hipcc takes as host and device.
#pragma once
#include <cstdint>

namespace sl {
namespace rowseg {

constexpr int kChunk = 1024;           // columns a wave holds in registers at a time: 16 per lane
constexpr int64_t kMinSegment = 1024;  // columns per wave when a row is split
constexpr int64_t kMaxItems = 0x7FFFFFFFll;

// waves per row: enough to give every CU eight waves, each with at least kMinSegment columns
constexpr int64_t splits(int64_t R, int64_t B, int64_t cus) {
  if (R <= 0) return 1;
  const int64_t want = (cus * 8 + R - 1) / R;
  const int64_t can = B / kMinSegment;
  const int64_t s = want < can ? want : can;
  return s < 2 ? 1 : s;
}

// columns per segment
constexpr int64_t segment(int64_t B, int64_t S) { return S == 1 ? B : (B + S - 1) / S; }

struct Bounds {
  int64_t lo, hi;
};
// columns [lo, hi) of segment s; hi <= lo for a trailing segment that is empty
constexpr Bounds segment_bounds(int64_t s, int64_t seg, int64_t B) {
  const int64_t lo = s * seg;
  return Bounds{lo, lo + seg < B ? lo + seg : B};
}

// the column, at most three before lo, whose element lies on a 16-byte boundary; first_elem_addr is the address of column lo
constexpr int64_t chunk_start(uintptr_t first_elem_addr, int64_t lo) { return lo - (int64_t)((first_elem_addr >> 2) & 3); }

// grid of one-wave workgroups: a few items per wave slot evens out items that take longer than others
constexpr int64_t wave_grid(int64_t items, int64_t cus, int64_t per_cu_waves) {
  const int64_t cap = cus * per_cu_waves * 4;
  return items < cap ? items : cap;
}

}  // namespace rowseg
}  // namespace sl

#if defined(__HIPCC__)
#include "common.hpp"

namespace sl {
namespace rowseg {

static_assert(kChunk == 16 * kWave, "a chunk is four 16-byte pieces per lane");

// ---- host side of a launch ---------------------------------------------------------------------------------------------------
// The refusals of a candidate tile, in two steps because every entry point has checks of its own between them (its ids, its
// scale, R == 0 as a no-op before any pointer is looked at) and the order in which a call is refused is part of its behaviour.
inline int check_tile_shape(const char* fn, int64_t B, int64_t ld) {
  SL_REQUIRE(B >= 1, "%s: B = %lld, a tile has at least one column", fn, (long long)B);
  SL_REQUIRE(ld >= B, "%s: row stride %lld below B = %lld", fn, (long long)ld, (long long)B);
  return 0;
}
inline int check_tile_ptr(const char* fn, const float* d_cand) {
  SL_REQUIRE(d_cand, "%s: null candidate tile", fn);
  SL_REQUIRE(((uintptr_t)d_cand & 3) == 0, "%s: candidate tile is not 4-byte aligned", fn);
  return 0;
}

inline int check_items(const char* fn, int64_t R, int64_t S) {
  SL_REQUIRE(R <= kMaxItems / S, "%s: %lld rows in %lld segments are more than 2^31 - 1 items; cut the tile", fn, (long long)R,
             (long long)S);
  return 0;
}

// a split row's workspace starts on the first 256-byte boundary of the caller's buffer (the *_ws_bytes leave room for it)
inline void* align_ws(void* d_ws) { return (void*)(((uintptr_t)d_ws + 255) & ~(uintptr_t)255); }

// ---- device side -----------------------------------------------------------------------------------------------------------------
struct Item {
  int64_t row;
  int s;
  int64_t lo, hi;
};
__device__ inline Item item(int64_t w, int S, int64_t seg, int64_t B) {
  const int s = (int)(w % S);
  const Bounds b = segment_bounds(s, seg, B);
  return Item{w / S, s, b.lo, b.hi};
}

// The chunk at column `base` of the row at rowp: lane `lane` gets columns [base + (u * 64 + lane) * 4, + 4) in x[u], `pad` where
// a column is outside [lo, hi).
__device__ inline void load_chunk(const float* __restrict__ rowp, int64_t base, int64_t lo, int64_t hi, int lane, float pad,
                                  f4 (&x)[4]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int64_t c = base + (int64_t)(u * kWave + lane) * 4;
    if (c >= lo && c + 4 <= hi) {
      x[u] = *reinterpret_cast<const f4*>(rowp + c);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) x[u][j] = (c + j >= lo && c + j < hi) ? rowp[c + j] : pad;
    }
  }
}

}  // namespace rowseg
}  // namespace sl
#endif
