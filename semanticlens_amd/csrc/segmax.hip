// K22 — per-segment column maxima of a cosine tile: the selection behind audit_concepts (lens.py).
//
// One launch reads a row-major fp32 tile (R,B) once — rows are prompts, columns are components — and folds the maximum of every
// column PER SEGMENT into a state (G, ·) that survives across tiles: entry (g, j) = the best row of segment g seen so far for
// column j.  Row r has the id row_id_base + r and belongs to segment row_seg[r]; a row whose segment is outside [0,G) is ignored.
//
// Order, packing and the empty entry are K20's (mutualmax.hip): one uint64 (f32_order_key(value) << 32) | (0xFFFFFFFF - id), 0 for
// "nothing seen", "better" the plain unsigned maximum.  It is associative and commutative, so the state is the maximum of the set of
// entries seen, bit for bit, however the rows and columns are cut into tiles, in whatever order the tiles are folded and however
// workgroups interleave.  sl_mutualmax_finish decodes it.
//
// Shape of the work: K20's column path.  A 256-thread workgroup owns kRowBlock = 64 rows x kStrip = 1024 columns; lane t owns
// columns [4 t, 4 t + 4) of the strip, one 16-byte piece per row, 16 rows' pieces in flight at a time.  Walking down the rows the
// lane keeps the running best (key, row) of its four columns in registers — rows ascend, so "strictly larger key" is the whole test.
// A row's segment is the same for the whole workgroup (one scalar load per row).  Whenever it changes, and after the last row, the
// bests are flushed: one 64-bit atomic max per column that saw something, into state[g * state_ld + column], and the registers
// start over.  A flush can come every row (runs of one), so it has no workgroup barrier: each wave transposes its own 256 bests
// through its own 2 KB of LDS, lane-major in and column-major out, so that an atomic instruction covers 64 consecutive entries
// (512 contiguous bytes) instead of every fourth entry of 2 KB.  Atomic bytes: 8 per column per segment run per row block, against
// 4 per column per row read.
//
// Loads are guarded as in K20: a piece that is not wholly inside [0,B) of its row, or whose address is not 16-byte aligned, is read
// element by element; nothing outside [0,B) of a row is touched.  All stores are vector atomics.
#include "common.hpp"

namespace sl {
namespace {

constexpr int kThreads = 256;
constexpr int kStrip = kThreads * 4;  // columns per workgroup
constexpr int kRowBlock = 64;         // rows per workgroup
constexpr int kBatch = 16;            // rows whose loads are issued back to back
constexpr int64_t kMaxPackedId = 0xFFFFFFFEll;
constexpr int64_t kMaxItems = 0x7FFFFFFFll;

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

__device__ inline u64 pack(uint32_t key, uint32_t low) { return key ? ((u64)key << 32) | low : 0ull; }
// orders a wave's own LDS writes and reads for the compiler; the hardware executes them in order
__device__ inline void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row_low = 0xFFFFFFFF - row_id_base (the host checked that no id passes 2^32 - 2).  ALIGNED: the tile starts on a 16-byte
// boundary and ld is a multiple of 4, so every piece inside [0,B) is aligned.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void segmax_tile_kernel(u64* __restrict__ state, int64_t state_ld, int64_t G, int64_t R,
                                                               int64_t B, const float* __restrict__ cand, int64_t ld,
                                                               const int32_t* __restrict__ row_seg, uint32_t row_low,
                                                               int64_t strips) {
  __shared__ u64 xpose[kThreads / kWave][kWave * 4];  // per wave: its 256 column bests, lane-major in, column-major out
  const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
  const int64_t strip = (int64_t)blockIdx.x % strips, rb = (int64_t)blockIdx.x / strips;
  const int64_t c0 = strip * kStrip + (int64_t)tid * 4;
  const int64_t r0 = rb * kRowBlock, r1 = r0 + kRowBlock < R ? r0 + kRowBlock : R;
  const bool full = c0 + 4 <= B;
  bool valid[4];
  uint32_t ck[4], cr[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    valid[j] = c0 + j < B;
    ck[j] = 0u, cr[j] = 0u;
  }
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
      if (r < r1) {
        const int64_t g = (seg[i] >= 0 && (int64_t)seg[i] < G) ? (int64_t)seg[i] : -1;
        if (g != cur) {  // uniform over the workgroup
          if (cur >= 0) flush();
          cur = g;
        }
        if (g >= 0) {
          const uint32_t rlow = row_low - (uint32_t)r;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            { const uint32_t k = valid[j] ? f32_order_key(x[i][j]) : 0u; if (k > ck[j]) ck[j] = k, cr[j] = rlow; }  // rows ascend: an equal key keeps the earlier row
        }
      }
    }
  }
  if (cur >= 0) flush();
}

int check_ids(const char* fn, const char* what, int64_t base, int64_t n) {
  SL_REQUIRE(base >= 0 && base <= kMaxPackedId && n <= kMaxPackedId + 1 - base,
             "%s: %s ids from %lld leave [0, 2^32 - 2], the range a packed state entry holds", fn, what, (long long)base);
  return 0;
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
  const int64_t strips = (B + kStrip - 1) / kStrip, blocks = (R + kRowBlock - 1) / kRowBlock;
  SL_REQUIRE(blocks <= kMaxItems / strips, "sl_segmax_merge: a (%lld, %lld) tile has more than 2^31 - 1 workgroups; cut it", (long long)R,
             (long long)B);
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const dim3 grid((unsigned)(strips * blocks));
  const uint32_t row_low = (uint32_t)(0xFFFFFFFFll - row_id_base);
  if (((uintptr_t)d_cand & 15) == 0 && ld % 4 == 0)
    SL_LAUNCH(prof, segmax_tile_kernel<true>, grid, dim3(kThreads), 0, st, (u64*)d_state, state_ld, G, R, B, d_cand, ld, d_row_seg,
              row_low, strips);
  else
    SL_LAUNCH(prof, segmax_tile_kernel<false>, grid, dim3(kThreads), 0, st, (u64*)d_state, state_ld, G, R, B, d_cand, ld, d_row_seg,
              row_low, strips);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
