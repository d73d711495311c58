// What the LDS-DMA ring GEMM kernels (gemm_8phase.hpp, gemm_w4.hpp, gemm_skinny.hpp) share: the operand and LDS layout contract
// that makes them bit-identical, written once.  A kernel's schedule (MFMA order, where reads and DMA issues sit between them,
// the counted waits) is its content and stays in its own header.
//
// Layout contract.  A 32-wide k-tile of one operand row is ONE 128-byte line in memory ([hi32 | lo32] bf16, or 32 floats).  One
// LDS-DMA instruction (global_load_lds_dwordx4) moves eight whole lines: lane L lands at base + 16 L, i.e. in row L >> 3 of its
// group, 16-byte slot L & 7.  An LDS image is unpadded rows of 128 bytes whose slots are XOR-swizzled by (row >> 1) & 7, applied
// on the SOURCE address of the DMA (dma_chunk) and on the fragment read (swz): conflict-free ds_read_b128.  Rows past the
// matrix edge are clamped onto the last row; their products land in outputs the epilogue never stores.
#pragma once
#include "common.hpp"
#include "gemm_choice.hpp"
#include "gemm_epilogue.hpp"

namespace sl {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
// One 16-byte fragment register quad.  It must be an ext_vector type: read through HIP's struct `uint4`, hipcc (ROCm 7.2) cannot
// tell the fragment reads from the LDS-DMA writes apart and puts `s_waitcnt vmcnt(0)` in front of the first ds_read of every
// phase, which drains the ring (8-phase kernel: 455 instead of 407 cycles per slot).
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

namespace ring {

template <int N_>
struct IntC {
  static constexpr int value = N_;
};
template <int I, int N_, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N_) {
    f(IntC<I>());
    static_for<I + 1, N_>(f);
  }
}

// Raw s_barrier only: __syncthreads() would add vmcnt(0) and drain the ring.
__device__ __forceinline__ void raw_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// XCD-aware tile order (bijective for any grid): XCD x = blockIdx % 8 owns a contiguous range of tiles, walked in bands of
// GROUP_M tile rows so that the workgroups sharing an L2 share A and B panels (+2-3 % on the 8-phase kernel)
__device__ __forceinline__ void xcd_tile(int tiles_m, int tiles_n, int& tm_i, int& tn_i) {
  const int nwg = tiles_m * tiles_n;
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  constexpr int GROUP_M = 4;
  const int band = tile / (GROUP_M * tiles_n);
  const int first_m = band * GROUP_M;
  const int rows = tiles_m - first_m < GROUP_M ? tiles_m - first_m : GROUP_M;
  const int in_band = tile - band * GROUP_M * tiles_n;
  tm_i = first_m + in_band % rows;
  tn_i = in_band / rows;
}

// THE swizzle: 16-byte chunk c of image row `row` sits in slot c ^ swz(row).  Fragment reads spell their address out at the site,
// row * 128 + ((c ^ ring::swz(row)) << 4): wrapped in a helper of (row, c), hipcc (ROCm 7.2) orders the xor's operands the other
// way round and the kernels' instruction streams change.
__device__ __forceinline__ int swz(int row) { return (row >> 1) & 7; }

// LDS-DMA source: lane L of the instruction that fills image row `row` lands in slot L & 7, so it fetches this chunk of the line
__device__ __forceinline__ int dma_chunk(int lane, int row) { return (lane & 7) ^ swz(row); }
// at this byte offset in the first k-tile (operand of R rows, tile starting at row r0; rows past the edge are clamped; 32 bits:
// launch_tiles() checks < 4 GB).  `chunk` is a parameter: computed in here from the lane, the instruction streams changed too.
__device__ __forceinline__ uint32_t dma_src(int64_t r0, int row, int64_t R, int64_t row_bytes, int chunk) {
  return (uint32_t)((r0 + row < R ? r0 + row : R - 1) * row_bytes + chunk * 16);
}

// one LDS-DMA instruction: 16 bytes per lane from g (per lane) to l + 16 lane (l wave-uniform)
__device__ __forceinline__ void dma16(const unsigned char* g, unsigned char* l) {
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  __builtin_amdgcn_global_load_lds((glb_void*)g, (lds_void*)l, 16, 0, 0);
}

// Host: the launch of one workgroup per BM x BN tile behind the limits every ring kernel has (32-bit tile index, k-tile count and
// lane offsets); `go(tm, tn)` launches on tm x tn tiles and is not called for an empty grid.
template <class Go>
int launch_tiles(int64_t M, int64_t N, int BM, int BN, int64_t row_bytes, int64_t ns, Go&& go) {
  const int64_t tm = (M + BM - 1) / BM, tn = (N + BN - 1) / BN;
  SL_REQUIRE(tm * tn < (1ll << 31) && ns < (1ll << 29), "GEMM: too many tiles");
  SL_REQUIRE(gemm_choice::fits(M, N, row_bytes), "GEMM: operand larger than 4 GB (use another kernel)");
  if (tm * tn == 0) return 0;
  go(tm, tn);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace ring
}  // namespace sl
