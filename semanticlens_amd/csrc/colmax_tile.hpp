// The column path that K20 (mutualmax.hip) and K22 (segmax.hip) share: how a cosine tile is cut into workgroups and lanes, the
// fold of a value into a column's running best, and the host side of a launch.
//
// A 256-thread workgroup owns kRowBlock = 64 rows x kStrip = 1024 columns of a row-major fp32 tile (R,B) (256 KB).  Lane t owns
// columns [4 t, 4 t + 4) of the strip: one 16-byte piece per row, kBatch = 16 rows' pieces in flight at a time.  Walking down
// the rows it keeps the running best (key, row low word) of each of its four columns in registers (packed_best.hpp: the order).
//
// Loads are guarded as in topk_tile_kernel: a piece that is not wholly inside [0,B) of its row, or whose address is not
// 16-byte aligned (a row stride that is no multiple of 4 shifts the alignment from row to row), is read element by element;
// nothing outside [0,B) of a row is touched.  ALIGNED instances: the tile starts on a 16-byte boundary and ld is a multiple
// of 4, so every piece inside [0,B) is aligned.  Those eight lines stay written out in both kernels: as a function, in every
// form tried, they left the unaligned instances 30 VGPRs lower with their blocks in another order, K22 2 % slower at run
// length 1.  The helpers here are free functions over the kernels' own locals, which keep registers, LDS and the row loop.
#pragma once
#include "common.hpp"
#include "packed_best.hpp"

namespace sl {

typedef unsigned long long u64;

namespace coltile {

constexpr int kThreads = 256;
constexpr int kStrip = kThreads * 4;  // columns per workgroup
constexpr int kRowBlock = 64;         // rows per workgroup
constexpr int kBatch = 16;            // rows whose loads are issued back to back
constexpr int64_t kMaxItems = 0x7FFFFFFFll;

// Workgroup blockIdx.x = rb * strips + strip owns rows [r0, r1) of the tile; its lane tid owns columns [c0, c0 + 4), of which
// valid[j] says whether c0 + j is below B and `full` whether all four are.
__device__ inline void lane_geometry(int64_t strips, int64_t R, int64_t B, int tid, int64_t& strip, int64_t& c0, int64_t& r0,
                                     int64_t& r1, bool& full, bool (&valid)[4]) {
  strip = (int64_t)blockIdx.x % strips;
  const int64_t rb = (int64_t)blockIdx.x / strips;
  c0 = strip * kStrip + (int64_t)tid * 4;
  r0 = rb * kRowBlock, r1 = r0 + kRowBlock < R ? r0 + kRowBlock : R;
  full = c0 + 4 <= B;
#pragma unroll
  for (int j = 0; j < 4; ++j) valid[j] = c0 + j < B;
}

// Fold the value v of the row with the low word rlow into a column's running best (ck, cr); returns v's key, 0 for a column at
// or beyond B.  Rows ascend: an equal key keeps the earlier row.
__device__ inline uint32_t fold_column(bool valid, float v, uint32_t rlow, uint32_t& ck, uint32_t& cr) {
  const uint32_t k = valid ? f32_order_key(v) : 0u;
  if (k > ck) ck = k, cr = rlow;
  return k;
}

// ---- host side of a launch ---------------------------------------------------------------------------------------------------
inline int check_ids(const char* fn, const char* what, int64_t base, int64_t n) {
  SL_REQUIRE(packed_best::ids_fit(base, n), "%s: %s ids from %lld leave [0, 2^32 - 2], the range a packed state entry holds", fn, what,
             (long long)base);
  return 0;
}

// one workgroup per (row block, strip) of a non-empty tile
inline int tile_grid(const char* fn, int64_t R, int64_t B, int64_t& strips, dim3& grid) {
  strips = (B + kStrip - 1) / kStrip;
  const int64_t blocks = (R + kRowBlock - 1) / kRowBlock;
  SL_REQUIRE(blocks <= kMaxItems / strips, "%s: a (%lld, %lld) tile has more than 2^31 - 1 workgroups; cut it", fn, (long long)R,
             (long long)B);
  grid = dim3((unsigned)(strips * blocks));
  return 0;
}

// may the ALIGNED instance of a tile kernel run?
inline bool tile_aligned(const float* d_cand, int64_t ld) { return ((uintptr_t)d_cand & 15) == 0 && ld % 4 == 0; }

}  // namespace coltile
}  // namespace sl
