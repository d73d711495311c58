// K22 — per-segment column maxima of a cosine tile: the selection behind audit_concepts (lens.py).
//
// One launch reads a row-major fp32 tile (R,B) once — rows are prompts, columns are components — and folds the maximum of every
// column PER SEGMENT into a state (G, ·) that survives across tiles: entry (g, j) = the best row of segment g seen so far for
// column j.  Row r has the id row_id_base + r and belongs to segment row_seg[r]; a row whose segment is outside [0,G) is ignored.
// Order and state entry: packed_best.hpp; sl_mutualmax_finish decodes the state.
//
// The cut into workgroups and lanes, the column fold and the host side of a launch are colmax_tile.hpp's,
// which also says how the loads are guarded and why that load is written out here.  What is K22's own: a row's
// segment is the same for the whole workgroup (one scalar load per row).  Whenever it changes, and after the last row, the
// bests are flushed: one 64-bit atomic max per column that saw something, into state[g * state_ld + column], and the registers
// start over.  A flush can come every row (runs of one), so it has no workgroup barrier: each wave transposes its own 256 bests
// through its own 2 KB of LDS, lane-major in and column-major out, so that an atomic instruction covers 64 consecutive entries
// (512 contiguous bytes) instead of every fourth entry of 2 KB.  Atomic bytes: 8 per column per segment run per row block, against
// 4 per column per row read.  All stores are vector atomics.
#include "colmax_tile.hpp"

namespace sl {
namespace {

using namespace coltile;
using packed_best::pack;

// orders a wave's own LDS writes and reads for the compiler; the hardware executes them in order
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row_low = id_low(row_id_base) (the host checked that no id passes 2^32 - 2).
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void segmax_tile_kernel(u64* __restrict__ state, int64_t state_ld, int64_t G, int64_t R,
                                                               int64_t B, const float* __restrict__ cand, int64_t ld,
                                                               const int32_t* __restrict__ row_seg, uint32_t row_low,
                                                               int64_t strips) {
  __shared__ u64 xpose[kThreads / kWave][kWave * 4];  // per wave: its 256 column bests, lane-major in, column-major out
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  int64_t strip, c0, r0, r1;
  bool full, valid[4];
  lane_geometry(strips, R, B, tid, strip, c0, r0, r1, full, valid);
  uint32_t ck[4] = {0u, 0u, 0u, 0u}, cr[4] = {0u, 0u, 0u, 0u};
  int64_t cur = -1;  // the segment the registers belong to; -1: none (ck is all zero then)
  // The wave's 256 bests go lane-major into its own LDS slice and come back column-major, so that one atomic instruction covers
  // 64 consecutive entries (512 contiguous bytes); one atomic max per column that saw a row of segment `cur`.  A wave's LDS
  // instructions execute in order, so the exchange needs no s_barrier: the fences only keep the compiler from reordering it.
  auto flush = [&]() {
    u64* buf = xpose[wave];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      buf[lane * 4 + j] = pack(ck[j], cr[j]);
      ck[j] = 0u;
    }
    wave_sync();
    u64* dst = state + cur * state_ld + strip * kStrip + wave * (kWave * 4) + lane;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const u64 v = buf[q * kWave + lane];
      if (v != 0ull) atomicMax(dst + q * kWave, v);  // v != 0 only for columns below B
    }
    wave_sync();
  };
  for (int64_t rbatch = r0; rbatch < r1; rbatch += kBatch) {
    f4 x[kBatch];
    int32_t seg[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      x[i] = f4{0.f, 0.f, 0.f, 0.f};
      seg[i] = -1;
      if (r < r1) {  // uniform over the workgroup
        seg[i] = row_seg[r];
        const float* p = cand + r * ld + c0;  // the guarded load of colmax_tile.hpp, in step with mutualmax.hip's
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
      if (r < r1) {
        const int64_t g = (seg[i] >= 0 && (int64_t)seg[i] < G) ? (int64_t)seg[i] : -1;
        if (g != cur) {  // uniform over the workgroup
          if (cur >= 0) flush();
          cur = g;
        }
        if (g >= 0) {
          const uint32_t rlow = row_low - (uint32_t)r;
#pragma unroll
          for (int j = 0; j < 4; ++j) fold_column(valid[j], x[i][j], rlow, ck[j], cr[j]);
        }
      }
    }
  }
  if (cur >= 0) flush();
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_segmax_merge(uint64_t* d_state, int64_t state_ld, int64_t G, int64_t R, int64_t B, const float* d_cand, int64_t ld,
                           const int32_t* d_row_seg, int64_t row_id_base, void* stream) {
  SL_REQUIRE(R >= 0 && B >= 0 && G >= 0, "sl_segmax_merge: negative shape (G = %lld, R = %lld, B = %lld)", (long long)G, (long long)R,
             (long long)B);
  SL_REQUIRE(ld >= B, "sl_segmax_merge: row stride %lld below B = %lld", (long long)ld, (long long)B);
  SL_REQUIRE(state_ld >= B, "sl_segmax_merge: state stride %lld below B = %lld", (long long)state_ld, (long long)B);
  if (int rc = check_ids("sl_segmax_merge", "row", row_id_base, R)) return rc;
  if (R == 0 || B == 0 || G == 0) return 0;
  SL_REQUIRE(d_state, "sl_segmax_merge: null state");
  SL_REQUIRE(d_cand, "sl_segmax_merge: null candidate tile");
  SL_REQUIRE(d_row_seg, "sl_segmax_merge: null segment table");
  SL_REQUIRE((((uintptr_t)d_cand | (uintptr_t)d_row_seg) & 3) == 0, "sl_segmax_merge: the tile or the segment table is not 4-byte aligned");
  SL_REQUIRE(((uintptr_t)d_state & 7) == 0, "sl_segmax_merge: the state is not 8-byte aligned");
  int64_t strips;
  dim3 grid;
  if (int rc = tile_grid("sl_segmax_merge", R, B, strips, grid)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const uint32_t row_low = packed_best::id_low(row_id_base);
  const auto kernel = tile_aligned(d_cand, ld) ? segmax_tile_kernel<true> : segmax_tile_kernel<false>;
  SL_LAUNCH(prof, kernel, grid, dim3(kThreads), 0, st, (u64*)d_state, state_ld, G, R, B, d_cand, ld, d_row_seg,
              row_low, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
