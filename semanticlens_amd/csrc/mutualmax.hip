// K20 — mutual best matches out of one cosine tile: the selection behind compare_concept_dbs (lens.py).
//
// One launch reads a row-major fp32 tile (R,B) once and folds BOTH its row maxima and its column maxima into two states that
// survive across tiles: row_state (R,) = the best column seen so far for every row, col_state (B,) = the best row seen so far
// for every column.  Row r has the id row_id_base + r, column j the id col_id_base + j.  Order and state entry: packed_best.hpp.
//
// The cut into workgroups and lanes, the column fold and the host side of a launch are colmax_tile.hpp's,
// which also says how the loads are guarded and why that load is written out here.  What is K20's own: the row
// path and the way the column bests leave.  A lane hands the best of its four columns of a row to LDS.  After kBatch = 16 rows
// the workgroup reduces the 16 x 256 LDS entries (16 threads per row, then four cross-lane steps) and ONE 64-bit atomic max per
// row leaves the CU; after the last row the column bests are transposed through LDS, so that a wave's atomic instruction covers
// 64 consecutive entries (512 contiguous bytes), and one atomic max per column leaves the CU.  Atomic bytes per workgroup:
// (64 + 1024) x 8 = 8.5 KB against 256 KB read, 1/30 of the tile bytes.  All stores are vector stores or vector atomics.
#include "colmax_tile.hpp"

namespace sl {
namespace {

using namespace coltile;
using packed_best::pack;

constexpr int kPad = 8;  // LDS row padding (entries): the 16 row groups of a reduction start in different banks

__device__ inline u64 umax64(u64 a, u64 b) { return a > b ? a : b; }

// low words: row_low = id_low(row_id_base), col_low = id_low(col_id_base) (the host checked that no id passes 2^32 - 2).
// ALIGNED: the batch's 16 loads are issued back to back before the first is used.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void mutualmax_tile_kernel(u64* __restrict__ row_state, u64* __restrict__ col_state, int64_t R,
                                                                  int64_t B, const float* __restrict__ cand, int64_t ld,
                                                                  uint32_t row_low, uint32_t col_low, int64_t strips) {
  __shared__ u64 part[kBatch][kThreads + kPad];
  const int tid = threadIdx.x;
  int64_t strip, c0, r0, r1;
  bool full, valid[4];
  lane_geometry(strips, R, B, tid, strip, c0, r0, r1, full, valid);
  uint32_t clow[4], ck[4], cr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    clow[j] = col_low - (uint32_t)(c0 + j);
    ck[j] = 0u, cr[j] = 0u;
  }
  for (int64_t rbatch = r0; rbatch < r1; rbatch += kBatch) {
    f4 x[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      x[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (r < r1) {  // uniform over the workgroup; the guarded load of colmax_tile.hpp, in step with the other kernel's
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
          const uint32_t k = fold_column(valid[j], x[i][j], rlow, ck[j], cr[j]);
          if (k > bk) bk = k, bl = clow[j];  // columns ascend within the lane
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
    uint32_t bits;
    packed_best::unpack(state[i], bits, ids[i]);
    vals[i] = bits_f32(bits);
  }
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
  int64_t strips;
  dim3 grid;
  if (int rc = tile_grid("sl_mutualmax_merge", R, B, strips, grid)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const uint32_t row_low = packed_best::id_low(row_id_base), col_low = packed_best::id_low(col_id_base);
  const auto kernel = tile_aligned(d_cand, ld) ? mutualmax_tile_kernel<true> : mutualmax_tile_kernel<false>;
  SL_LAUNCH(prof, kernel, grid, dim3(kThreads), 0, st, (u64*)d_row_state, (u64*)d_col_state, R, B, d_cand, ld,
              row_low, col_low, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_mutualmax_finish(const uint64_t* d_state, int64_t n, float* d_vals, int64_t* d_ids, void* stream) {
  SL_REQUIRE(n >= 0, "sl_mutualmax_finish: negative entry count");
  if (n == 0) return 0;
  SL_REQUIRE(d_state && d_vals && d_ids, "sl_mutualmax_finish: null pointer");
  SL_REQUIRE(((uintptr_t)d_state & 7) == 0, "sl_mutualmax_finish: the state is not 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)n * 20);
  SL_LAUNCH(prof, mutualmax_finish_kernel, dim3(stride_grid_256(n)), dim3(256), 0, st, (const u64*)d_state, n, d_vals, d_ids);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
