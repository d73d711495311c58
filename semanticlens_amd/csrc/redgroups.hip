// K24 — redundancy groups out of cosine tiles: the connected components of the graph "cosine >= threshold" over one layer's
// components, and every component's degree in it.  The selection behind scores.redundancy_groups.
//
// State across tiles: parent (n,) int32, the union-find forest of unionfind.hpp (which holds the hook rule and why nothing
// here can loop or wait), degree (n,) int32, and one int32 status word that a lane raises when a loop passes its cap.
// One launch reads a row-major fp32 tile (R,B) once, cut as K20's (colmax_tile.hpp: 64 rows x 1024 columns per workgroup,
// lane t owns four columns, 16 rows' 16-byte pieces in flight, the same guarded loads).  Row r has the id row_id_base + r,
// column c the id col_id_base + c; an element is an edge iff row id < column id and v >= threshold: the upper triangle only,
// so a pair is counted once, a NaN is never an edge and the diagonal never is.
//
// A lane gathers the edges of its 16 x 4 elements of a batch into one 64-bit mask.  At the thresholds this is for almost every
// mask is zero: a wave whose ballot of non-empty masks is empty does nothing but read, and a workgroup with no such wave skips
// the row reduction.  Otherwise only the lanes with a bit set call unite, once per bit.  Degrees: a column's count grows in a
// register down the rows and leaves after the last row, transposed through LDS so that a wave's atomic covers consecutive
// words, one atomic per non-zero column per workgroup; a row's count is summed over the row's 256 lanes through LDS as K20
// reduces its row maxima, one atomic per non-zero row per workgroup.  parent is read with agent-scope relaxed atomic loads and
// written with agent-scope atomic minima only.  All stores are vector stores or vector atomics.
//
// The second pass (cohesion) reads the tiles again with the final labels: for an upper-triangle element whose row and column
// carry one label, one 32-bit atomic min of the value's order key (packed_best.hpp) into state[label].  Such pairs are rare,
// so the atomics leave per lane.
#include "colmax_tile.hpp"
#include "unionfind.hpp"

namespace sl {
namespace {

using namespace coltile;

constexpr int kPad = 8;  // LDS row padding (entries), as K20's
constexpr uint32_t kEmptyKey = 0xFFFFFFFFu;

struct DeviceOps {
  using word = int32_t;
  static __device__ inline int32_t load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  static __device__ inline int32_t fetch_min(int32_t* p, int32_t v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

__device__ inline void raise_status(int32_t* status) { __hip_atomic_fetch_or(status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void unionfind_init_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ degree,
                                                               int32_t* __restrict__ status, int64_t n) {
  const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (first == 0) *status = 0;
  for (int64_t i = first; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    __hip_atomic_store(parent + i, (int32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    degree[i] = 0;
  }
}

__global__ __launch_bounds__(256) void unionfind_flatten_kernel(int32_t* __restrict__ parent, int64_t n, int32_t* __restrict__ status) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    if (!unionfind::flatten<DeviceOps>(parent, (int32_t)i, (int32_t)n)) raise_status(status);
}

// bit 4 i + j of a lane's mask: row i of the batch, column j of the lane
constexpr u64 kColumnBits = 0x1111111111111111ull;

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void threshold_union_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ degree,
                                                                   int32_t* __restrict__ status, int32_t n, int64_t R, int64_t B,
                                                                   const float* __restrict__ cand, int64_t ld, int64_t row_id_base,
                                                                   int64_t col_id_base, float threshold, int64_t strips) {
  __shared__ int32_t part[kBatch][kThreads + kPad];
  const int tid = threadIdx.x;
  int64_t strip, c0, r0, r1;
  bool full, valid[4];
  lane_geometry(strips, R, B, tid, strip, c0, r0, r1, full, valid);
  // a workgroup whose last column id is not above its first row id holds no element of the upper triangle
  const int64_t strip_end = (strip + 1) * kStrip < B ? (strip + 1) * kStrip : B;
  if (col_id_base + strip_end - 1 <= row_id_base + r0) return;
  const int64_t cid0 = col_id_base + c0;
  int32_t cdeg[4] = {0, 0, 0, 0};
  bool any_edge = false;  // uniform over the workgroup
  for (int64_t rbatch = r0; rbatch < r1; rbatch += kBatch) {
    f4 x[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      x[i] = f4{0.f, 0.f, 0.f, 0.f};
      if (r < r1) {  // uniform over the workgroup; the guarded load of colmax_tile.hpp, in step with K20's
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
    u64 mask = 0ull;
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      if (r < r1) {
        const int64_t above = cid0 - (row_id_base + r);  // column j is right of the diagonal iff above + j > 0
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (valid[j] && above + j > 0 && x[i][j] >= threshold) mask |= 1ull << (4 * i + j);
      }
    }
    const bool wave_edge = __ballot(mask != 0ull) != 0ull;
    if (!__syncthreads_or(wave_edge)) continue;  // the usual case: nothing but the read
    any_edge = true;
    if (wave_edge) {
#pragma unroll
      for (int i = 0; i < kBatch; ++i) part[i][tid] = __popcll(mask & (0xFull << (4 * i)));
    } else {
#pragma unroll
      for (int i = 0; i < kBatch; ++i) part[i][tid] = 0;
    }
    if (mask != 0ull) {
#pragma unroll
      for (int j = 0; j < 4; ++j) cdeg[j] += __popcll(mask & (kColumnBits << j));
      for (u64 m = mask; m != 0ull; m &= m - 1) {
        const int bit = __ffsll((unsigned long long)m) - 1;
        const int32_t rid = (int32_t)(row_id_base + rbatch + (bit >> 2)), cid = (int32_t)(cid0 + (bit & 3));
        if (!unionfind::unite<DeviceOps>(parent, rid, cid, n)) {
          raise_status(status);
          break;
        }
      }
    }
    __syncthreads();
    {
      const int row = tid >> 4, sub = tid & 15;
      int32_t s = 0;
#pragma unroll
      for (int q = 0; q < kThreads / 16; ++q) s += part[row][sub + 16 * q];
#pragma unroll
      for (int d = 8; d > 0; d >>= 1) s += __shfl_xor(s, d, 16);
      if (sub == 0 && s != 0) atomicAdd(degree + row_id_base + rbatch + row, s);  // s != 0 only for rows below r1
    }
    __syncthreads();
  }
  if (!any_edge) return;
  // column degrees: lane-major in registers -> column-major through LDS, so that one atomic instruction covers consecutive words
  int32_t* colbuf = &part[0][0];  // kStrip entries of the kBatch * (kThreads + kPad) there
#pragma unroll
  for (int j = 0; j < 4; ++j) colbuf[tid * 4 + j] = cdeg[j];
  __syncthreads();
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int idx = q * kThreads + tid;
    const int32_t v = colbuf[idx];
    if (v != 0) atomicAdd(degree + col_id_base + strip * kStrip + idx, v);  // v != 0 only for columns below B
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void group_min_kernel(uint32_t* __restrict__ state, const int32_t* __restrict__ labels, int32_t n,
                                                             int64_t R, int64_t B, const float* __restrict__ cand, int64_t ld,
                                                             int64_t row_id_base, int64_t col_id_base, int64_t strips) {
  const int tid = threadIdx.x;
  int64_t strip, c0, r0, r1;
  bool full, valid[4];
  lane_geometry(strips, R, B, tid, strip, c0, r0, r1, full, valid);
  const int64_t strip_end = (strip + 1) * kStrip < B ? (strip + 1) * kStrip : B;
  if (col_id_base + strip_end - 1 <= row_id_base + r0) return;
  const int64_t cid0 = col_id_base + c0;
  int32_t clab[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) clab[j] = valid[j] ? labels[cid0 + j] : -1;
  for (int64_t rbatch = r0; rbatch < r1; rbatch += kBatch) {
    f4 x[kBatch];
    int32_t rlab[kBatch];
#pragma unroll
    for (int i = 0; i < kBatch; ++i) {
      const int64_t r = rbatch + i;
      x[i] = f4{0.f, 0.f, 0.f, 0.f};
      rlab[i] = -2;
      if (r < r1) {  // uniform over the workgroup; the guarded load of colmax_tile.hpp
        rlab[i] = labels[row_id_base + r];
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
      const int64_t above = cid0 - (row_id_base + rbatch + i);
#pragma unroll
      for (int j = 0; j < 4; ++j)  // rlab is -2 past r1 and clab -1 past B: neither equals the other or a label
        if (rlab[i] == clab[j] && above + j > 0 && (uint32_t)clab[j] < (uint32_t)n) atomicMin(state + clab[j], f32_order_key(x[i][j]));
    }
  }
}

__global__ __launch_bounds__(256) void group_min_finish_kernel(const uint32_t* __restrict__ state, const int32_t* __restrict__ labels,
                                                                 int64_t n, float* __restrict__ cohesion) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t lab = (uint32_t)labels[i];
    cohesion[i] = bits_f32(order_key_f32_bits(lab < (uint32_t)n ? state[lab] : kEmptyKey));  // the empty entry decodes as NaN
  }
}

constexpr int64_t kMaxN = 0x7FFFFFFFll;

// what both tile entry points require of a tile and its ids
int check_tile(const char* fn, int64_t n, const float* d_cand, int64_t ld, int64_t R, int64_t B, int64_t row_id_base, int64_t col_id_base) {
  SL_REQUIRE(n >= 0 && n <= kMaxN, "%s: n = %lld not in [0, 2^31 - 1]", fn, (long long)n);
  SL_REQUIRE(R >= 0 && B >= 0, "%s: negative tile shape (%lld, %lld)", fn, (long long)R, (long long)B);
  SL_REQUIRE(ld >= B, "%s: row stride %lld below B = %lld", fn, (long long)ld, (long long)B);
  SL_REQUIRE(row_id_base >= 0 && row_id_base <= n && R <= n - row_id_base, "%s: row ids from %lld leave [0, n = %lld)", fn,
             (long long)row_id_base, (long long)n);
  SL_REQUIRE(col_id_base >= 0 && col_id_base <= n && B <= n - col_id_base, "%s: column ids from %lld leave [0, n = %lld)", fn,
             (long long)col_id_base, (long long)n);
  if (R == 0 || B == 0) return 0;
  SL_REQUIRE(d_cand, "%s: null candidate tile", fn);
  SL_REQUIRE(((uintptr_t)d_cand & 3) == 0, "%s: candidate tile is not 4-byte aligned", fn);
  return 0;
}

// no element of the tile has a row id below its column id
inline bool below_diagonal(int64_t R, int64_t B, int64_t row_id_base, int64_t col_id_base) {
  return R == 0 || B == 0 || col_id_base + B - 1 <= row_id_base;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_unionfind_init(int32_t* d_parent, int32_t* d_degree, int32_t* d_status, int64_t n, void* stream) {
  SL_REQUIRE(n >= 0 && n <= kMaxN, "sl_unionfind_init: n = %lld not in [0, 2^31 - 1]", (long long)n);
  SL_REQUIRE(d_status && (n == 0 || (d_parent && d_degree)), "sl_unionfind_init: null state");
  SL_REQUIRE((((uintptr_t)d_parent | (uintptr_t)d_degree | (uintptr_t)d_status) & 3) == 0, "sl_unionfind_init: the state is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)n * 8);
  SL_LAUNCH(prof, unionfind_init_kernel, dim3(stride_grid_256(n > 0 ? n : 1)), dim3(256), 0, st, d_parent, d_degree, d_status, n);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_threshold_union_merge(int32_t* d_parent, int32_t* d_degree, int32_t* d_status, int64_t n, const float* d_cand, int64_t ld,
                                    int64_t R, int64_t B, int64_t row_id_base, int64_t col_id_base, float threshold, void* stream) {
  SL_REQUIRE(threshold - threshold == 0.f, "sl_threshold_union_merge: the threshold is not finite");
  if (int rc = check_tile("sl_threshold_union_merge", n, d_cand, ld, R, B, row_id_base, col_id_base)) return rc;
  if (below_diagonal(R, B, row_id_base, col_id_base)) return 0;
  SL_REQUIRE(d_parent && d_degree && d_status, "sl_threshold_union_merge: null state");
  SL_REQUIRE((((uintptr_t)d_parent | (uintptr_t)d_degree | (uintptr_t)d_status) & 3) == 0,
             "sl_threshold_union_merge: the state is not 4-byte aligned");
  int64_t strips;
  dim3 grid;
  if (int rc = tile_grid("sl_threshold_union_merge", R, B, strips, grid)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const auto kernel = tile_aligned(d_cand, ld) ? threshold_union_kernel<true> : threshold_union_kernel<false>;
  SL_LAUNCH(prof, kernel, grid, dim3(kThreads), 0, st, d_parent, d_degree, d_status, (int32_t)n, R, B, d_cand, ld, row_id_base,
            col_id_base, threshold, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_unionfind_flatten(int32_t* d_parent, int64_t n, int32_t* d_status, void* stream) {
  SL_REQUIRE(n >= 0 && n <= kMaxN, "sl_unionfind_flatten: n = %lld not in [0, 2^31 - 1]", (long long)n);
  if (n == 0) return 0;
  SL_REQUIRE(d_parent && d_status, "sl_unionfind_flatten: null state");
  SL_REQUIRE((((uintptr_t)d_parent | (uintptr_t)d_status) & 3) == 0, "sl_unionfind_flatten: the state is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)n * 8);
  SL_LAUNCH(prof, unionfind_flatten_kernel, dim3(stride_grid_256(n)), dim3(256), 0, st, d_parent, n, d_status);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_group_min_merge(uint32_t* d_state, const int32_t* d_labels, int64_t n, const float* d_cand, int64_t ld, int64_t R, int64_t B,
                              int64_t row_id_base, int64_t col_id_base, void* stream) {
  if (int rc = check_tile("sl_group_min_merge", n, d_cand, ld, R, B, row_id_base, col_id_base)) return rc;
  if (below_diagonal(R, B, row_id_base, col_id_base)) return 0;
  SL_REQUIRE(d_state && d_labels, "sl_group_min_merge: null state");
  SL_REQUIRE((((uintptr_t)d_state | (uintptr_t)d_labels) & 3) == 0, "sl_group_min_merge: the state is not 4-byte aligned");
  int64_t strips;
  dim3 grid;
  if (int rc = tile_grid("sl_group_min_merge", R, B, strips, grid)) return rc;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const auto kernel = tile_aligned(d_cand, ld) ? group_min_kernel<true> : group_min_kernel<false>;
  SL_LAUNCH(prof, kernel, grid, dim3(kThreads), 0, st, d_state, d_labels, (int32_t)n, R, B, d_cand, ld, row_id_base, col_id_base, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_group_min_finish(const uint32_t* d_state, const int32_t* d_labels, int64_t n, float* d_cohesion, void* stream) {
  SL_REQUIRE(n >= 0 && n <= kMaxN, "sl_group_min_finish: n = %lld not in [0, 2^31 - 1]", (long long)n);
  if (n == 0) return 0;
  SL_REQUIRE(d_state && d_labels && d_cohesion, "sl_group_min_finish: null pointer");
  SL_REQUIRE((((uintptr_t)d_state | (uintptr_t)d_labels | (uintptr_t)d_cohesion) & 3) == 0, "sl_group_min_finish: a pointer is not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)n * 12);
  SL_LAUNCH(prof, group_min_finish_kernel, dim3(stride_grid_256(n)), dim3(256), 0, st, d_state, d_labels, n, d_cohesion);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
