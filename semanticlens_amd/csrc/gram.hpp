// Per-component Gram matrices H[c] = V_c V_c^T in fp64 (accumulation of exact fp32 products): the first launch of K9
// (kmeans.hip) and of K23 (silhouette.hip).  Two kernels with two summation orders — a caller that must stay bit-identical
// keeps the kernel it has.
#pragma once
#include "common.hpp"

namespace sl {
namespace {

constexpr int kGramStagedMaxN = 128;  // gram_kernel keeps a register array of pair accumulators sized for this n

// One workgroup per component; the (n x Dc) slab is staged in LDS (rows padded by one float) and each
// thread owns pairs p = t, t + 256, ... of the upper triangle.  n <= kGramStagedMaxN; dynamic LDS: n * (Dc + 1) floats.
__global__ __launch_bounds__(256) void gram_kernel(const float* __restrict__ V, int64_t C, int n, int64_t D, int Dc,
                                                    double* __restrict__ H) {
  extern __shared__ float s_v[];  // n x (Dc + 1)
  const int ld = Dc + 1;
  const int npairs = n * (n + 1) / 2;
  constexpr int kMaxPairsPerThread = (kGramStagedMaxN * (kGramStagedMaxN + 1) / 2 + 255) / 256;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const float* Vc = V + c * (int64_t)n * D;
    double acc[kMaxPairsPerThread];
#pragma unroll
    for (int a = 0; a < kMaxPairsPerThread; ++a) acc[a] = 0.0;
    for (int64_t d0 = 0; d0 < D; d0 += Dc) {
      const int dc = (int)((D - d0) < Dc ? (D - d0) : Dc);
      __syncthreads();
      for (int e = threadIdx.x; e < n * dc; e += 256) {
        const int i = e / dc, d = e % dc;
        s_v[i * ld + d] = Vc[(int64_t)i * D + d0 + d];
      }
      __syncthreads();
#pragma unroll
      for (int a = 0; a < kMaxPairsPerThread; ++a) {
        const int p = threadIdx.x + a * 256;
        if (p < npairs) {
          // p -> (i, j), i <= j, row-major upper triangle
          int i = 0, rem = p;
          while (rem >= n - i) {
            rem -= n - i;
            ++i;
          }
          const int j = i + rem;
          const float* a_ = s_v + i * ld;
          const float* b_ = s_v + j * ld;
          double s = 0.0;
          for (int d = 0; d < dc; ++d) s += (double)a_[d] * (double)b_[d];
          acc[a] += s;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < kMaxPairsPerThread; ++a) {
      const int p = threadIdx.x + a * 256;
      if (p < npairs) {
        int i = 0, rem = p;
        while (rem >= n - i) {
          rem -= n - i;
          ++i;
        }
        const int j = i + rem;
        H[(c * n + i) * n + j] = acc[a];
        H[(c * n + j) * n + i] = acc[a];
      }
    }
  }
}

// Gram matrices for any n: one thread per pair, rows read from L2.  Grid (pair tiles, C): C <= 65535.
__global__ __launch_bounds__(256) void gram_general_kernel(const float* __restrict__ V, int64_t C, int n, int64_t D,
                                                            double* __restrict__ H) {
  const int64_t c = blockIdx.y;
  const int64_t npairs = (int64_t)n * n;
  const float* Vc = V + c * (int64_t)n * D;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * 256) {
    const int i = (int)(p / n), j = (int)(p % n);
    if (j < i) continue;
    const float* a = Vc + (int64_t)i * D;
    const float* b = Vc + (int64_t)j * D;
    double s = 0.0;
    for (int64_t d = 0; d < D; ++d) s += (double)a[d] * (double)b[d];
    H[(c * n + i) * n + j] = s;
    H[(c * n + j) * n + i] = s;
  }
}

}  // namespace
}  // namespace sl
