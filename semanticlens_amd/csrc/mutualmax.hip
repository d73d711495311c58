// K20 — mutual best matches out of one cosine tile: the selection behind compare_concept_dbs (lens.py).
//
// One launch reads a row-major fp32 tile (R,B) once and folds BOTH its row maxima and its column maxima into two states that
// survive across tiles: row_state (R,) = the best column seen so far for every row, col_state (B,) = the best row seen so far
// for every column.  Row r has the id row_id_base + r, column j the id col_id_base + j.
//
// Order: K17's (topk.hip) — NaN before every number, then the larger value, -0.0 == +0.0, equal values by the smaller id.
//
// State entry: one uint64, (f32_order_key(value) << 32) | (0xFFFFFFFF - id); 0 is the empty entry (every real value's key is
// >= 0x007FFFFF).  Under this packing "better" is the plain unsigned maximum, which is associative and commutative: whatever
// the order in which lanes, waves, workgroups, tiles and the memory side's 64-bit atomic max combine the entries, the state is
// the maximum of the set of entries seen, bit for bit.  Ids are limited to [0, 2^32 - 2].  The packing carries neither the sign
// of a zero nor a NaN's payload: a decoded +-0.0 is +0.0, a decoded NaN is the canonical quiet NaN (0x7FC00000).
//
// Shape of the work: a 256-thread workgroup owns kRowBlock = 64 rows x kStrip = 1024 columns (256 KB of the tile).  Lane t
// owns columns [4 t, 4 t + 4) of the strip: one 16-byte piece per row.  Walking down the rows it keeps the running best
// (key, row) of each of its four columns in registers — rows come in ascending id, so "strictly larger key" is the whole
// test — and hands the best of its four columns of a row to LDS.  After kBatch = 16 rows the workgroup reduces the 16 x 256
// LDS entries (16 threads per row, then four cross-lane steps) and ONE 64-bit atomic max per row leaves the CU; after the last
// row the column bests are transposed through LDS, so that a wave's atomic instruction covers 64 consecutive entries (512
// contiguous bytes), and one atomic max per column leaves the CU.  Atomic bytes per workgroup: (64 + 1024) x 8 = 8.5 KB
// against 256 KB read, 1/30 of the tile bytes.
//
// Loads are guarded as in topk_tile_kernel: a piece that is not wholly inside [0,B) of its row, or whose address is not
// 16-byte aligned (a row stride that is no multiple of 4 shifts the alignment from row to row), is read element by element;
// nothing outside [0,B) of a row is touched.  All stores are vector stores or vector atomics.
#include "common.hpp"

namespace sl {
namespace {

constexpr int kThreads = 256;
constexpr int kStrip = kThreads * 4;  // columns per workgroup
constexpr int kRowBlock = 64;         // rows per workgroup
constexpr int kBatch = 16;            // rows between two row reductions
constexpr int kPad = 8;               // LDS row padding (entries): the 16 row groups of a reduction start in different banks
constexpr int64_t kMaxPackedId = 0xFFFFFFFEll;
constexpr int64_t kMaxItems = 0x7FFFFFFFll;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

__device__ inline u64 pack(uint32_t key, uint32_t low) { return key ? ((u64)key << 32) | low : 0ull; }
__device__ inline u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// low words: row_low = 0xFFFFFFFF - row_id_base, col_low = 0xFFFFFFFF - col_id_base (the host checked that no id passes 2^32 - 2).
// ALIGNED: the tile starts on a 16-byte boundary and ld is a multiple of 4, so every piece inside [0,B) is aligned and the
// batch's 16 loads are issued back to back before the first is used.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mutualmax_tile_kernel(u64* __restrict__ row_state, u64* __restrict__ col_state, int64_t R,
                                                                  int64_t B, const float* __restrict__ cand, int64_t ld,
                                                                  uint32_t row_low, uint32_t col_low, int64_t strips) {
  __shared__ u64 part[kBatch][kThreads + kPad];
  const int tid = threadIdx.x;
  const int64_t strip = (int64_t)blockIdx.x % strips, rb = (int64_t)blockIdx.x / strips;
  const int64_t c0 = strip * kStrip + (int64_t)tid * 4;
  const int64_t r0 = rb * kRowBlock, r1 = r0 + kRowBlock < R ? r0 + kRowBlock : R;
  const bool full = c0 + 4 <= B;
  bool valid[4];
  uint32_t clow[4], ck[4], cr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    valid[j] = c0 + j < B;
    clow[j] = col_low - (uint32_t)(c0 + j);
    ck[j] = 0u, cr[j] = 0u;
  }
  for (int64_t rbatch = r0; rbatch < r1; rbatch += kBatch) {
    f4 x[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      x[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (r < r1) {  // uniform over the workgroup
        const float* p = cand + r * ld + c0;
        if (full && (ALIGNED || ((uintptr_t)p & 15) == 0)) {
          x[i] = *reinterpret_cast<const f4*>(p);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (valid[j]) x[i][j] = p[j];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      uint32_t bk = 0u, bl = 0u;
      if (r < r1) {
        const uint32_t rlow = row_low - (uint32_t)r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t k = valid[j] ? f32_order_key(x[i][j]) : 0u;
          if (k > ck[j]) ck[j] = k, cr[j] = rlow;  // rows ascend: an equal key keeps the earlier row
          if (k > bk) bk = k, bl = clow[j];         // columns ascend within the lane
        }
      }
      part[i][tid] = pack(bk, bl);
    }
    __syncthreads();
    {
      const int row = tid >> 4, sub = tid & 15;
      u64 m = 0ull;
#pragma unroll
      for (int q = 0; q < kThreads / 16; ++q) m = umax64(m, part[row][sub + 16 * q]);
#pragma unroll
      for (int d = 8; d > 0; d >>= 1) m = umax64(m, (u64)__shfl_xor((unsigned long long)m, d, 16));
      if (sub == 0 && m != 0ull && rbatch + row < r1) atomicMax(row_state + rbatch + row, m);
    }
    __syncthreads();
  }
  // column bests: lane-major in registers -> column-major through LDS, so that one atomic instruction covers 64 consecutive entries
  u64* colbuf = &part[0][0];  // kStrip entries of the kBatch * (kThreads + kPad) there
#pragma unroll
  for (int j = 0; j < 4; ++j) colbuf[tid * 4 + j] = pack(ck[j], cr[j]);
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = q * kThreads + tid;
    const u64 v = colbuf[idx];
    if (v != 0ull) atomicMax(col_state + strip * kStrip + idx, v);  // v != 0 only for columns below B
  }
}

__global__ __launch_bounds__(256) void mutualmax_finish_kernel(const u64* __restrict__ state, int64_t n, float* __restrict__ vals,
                                                                 int64_t* __restrict__ ids) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const u64 s = state[i];
    const uint32_t key = (uint32_t)(s >> 32);
    float v = -INFINITY;
    int64_t id = -1;
    if (s != 0ull) {
      id = (int64_t)(0xFFFFFFFFu - (uint32_t)s);
      // the inverse of f32_order_key: NaN -> the canonical quiet NaN; the keys of +0.0 and -0.0 coincide and decode as +0.0
      v = key == 0xFFFFFFFFu ? bits_f32(0x7FC00000u) : bits_f32((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
    }
    vals[i] = v;
    ids[i] = id;
  }
}

int check_ids(const char* fn, const char* what, int64_t base, int64_t n) {
  SL_REQUIRE(base >= 0 && base <= kMaxPackedId && n <= kMaxPackedId + 1 - base,
             "%s: %s ids from %lld leave [0, 2^32 - 2], the range a packed state entry holds", fn, what, (long long)base);
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_mutualmax_merge(uint64_t* d_row_state, uint64_t* d_col_state, int64_t R, int64_t B, const float* d_cand, int64_t ld,
                              int64_t row_id_base, int64_t col_id_base, void* stream) {
  SL_REQUIRE(R >= 0 && B >= 0, "sl_mutualmax_merge: negative tile shape (%lld, %lld)", (long long)R, (long long)B);
  SL_REQUIRE(ld >= B, "sl_mutualmax_merge: row stride %lld below B = %lld", (long long)ld, (long long)B);
  if (int rc = check_ids("sl_mutualmax_merge", "row", row_id_base, R)) return rc;
  if (int rc = check_ids("sl_mutualmax_merge", "column", col_id_base, B)) return rc;
  if (R == 0 || B == 0) return 0;
  SL_REQUIRE(d_row_state && d_col_state, "sl_mutualmax_merge: null state");
  SL_REQUIRE(d_cand, "sl_mutualmax_merge: null candidate tile");
  SL_REQUIRE(((uintptr_t)d_cand & 3) == 0, "sl_mutualmax_merge: candidate tile is not 4-byte aligned");
  SL_REQUIRE((((uintptr_t)d_row_state | (uintptr_t)d_col_state) & 7) == 0, "sl_mutualmax_merge: a state is not 8-byte aligned");
  const int64_t strips = (B + kStrip - 1) / kStrip, blocks = (R + kRowBlock - 1) / kRowBlock;
  SL_REQUIRE(blocks <= kMaxItems / strips, "sl_mutualmax_merge: a (%lld, %lld) tile has more than 2^31 - 1 workgroups; cut it",
             (long long)R, (long long)B);
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const dim3 grid((unsigned)(strips * blocks));
  const uint32_t row_low = (uint32_t)(0xFFFFFFFFll - row_id_base), col_low = (uint32_t)(0xFFFFFFFFll - col_id_base);
  if (((uintptr_t)d_cand & 15) == 0 && ld % 4 == 0)
    SL_LAUNCH(prof, mutualmax_tile_kernel<true>, grid, dim3(kThreads), 0, st, (u64*)d_row_state, (u64*)d_col_state, R, B, d_cand, ld,
              row_low, col_low, strips);
  else
    SL_LAUNCH(prof, mutualmax_tile_kernel<false>, grid, dim3(kThreads), 0, st, (u64*)d_row_state, (u64*)d_col_state, R, B, d_cand, ld,
              row_low, col_low, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_mutualmax_finish(const uint64_t* d_state, int64_t n, float* d_vals, int64_t* d_ids, void* stream) {
  SL_REQUIRE(n >= 0, "sl_mutualmax_finish: negative entry count");
  if (n == 0) return 0;
  SL_REQUIRE(d_state && d_vals && d_ids, "sl_mutualmax_finish: null pointer");
  SL_REQUIRE(((uintptr_t)d_state & 7) == 0, "sl_mutualmax_finish: the state is not 8-byte aligned");
  int64_t blocks = (n + 255) / 256;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (blocks > cap) blocks = cap;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)n * 20);
  SL_LAUNCH(prof, mutualmax_finish_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (const u64*)d_state, n, d_vals, d_ids);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
