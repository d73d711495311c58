// K21 — per-facet statistics of a clustered concept DB: what semanticlens/scores.py:167-168 takes from scikit-learn as
// `labels_` and `cluster_centers_`, plus clarity_score (scores.py:18-47) within each facet.
//
//   V (C,n,D) fp32, labels (C,n) int32 -> counts (C,kc), centres (C,kc,D) = mean of the RAW rows with label j,
//                                          clarity (C,kc) = clarity_score of those rows
//
// The traffic is K7 clarity's: C*n*D*4 bytes read once, kc/n of that written.  One workgroup reduces one component in a
// fixed order (grid-stride over components), so the results do not depend on the grid; there are no float atomics.
//
// Fast path (facet_rows_kernel<PPL, KCT>), modelled on clarity_multi_kernel: D % 4 == 0, 16-byte aligned slabs.  Wave w owns
// rows w, w + 4, ...; a row is 16-byte pieces, PPL per lane; all loads of a row batch are issued before the first use; the
// row's inverse norm is one xor-shuffle tree; the row's label is wave-uniform (a scalar load), and the wave folds the row
// into the two column sums of that cluster, raw and normalised, held in registers: 2 * KCT * PPL float4 per lane, KCT = kc
// rounded up to a power of two.  The four waves' sums meet in LDS, one cluster at a time.
//   Cut-off KCT * PPL <= 16 (128 accumulator VGPRs).  Compiler's register report at the edge of the cut-off (gfx950, -O3):
//   see DESIGN.md §K21.  kc = 2 takes this path for every D <= 2048 (PPL <= 8).
// General path (facet_cols_kernel): any D, any kc <= 16.  Pass 1 computes the inverse norms (as clarity_kernel); pass 2 walks
// each cluster's rows of the (L2-resident) slab, thread f owning columns f, f + 256, ...: every row is read once more.
#include "common.hpp"

namespace sl {
namespace {

constexpr int kMaxFacets = 16, kMaxFacetRows = 1024;
constexpr int kFastBudget = 16;  // KCT * PPL at most

__device__ inline float facet_block_sum(float v, float* s_red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s_red[w] = v;
  __syncthreads();
  const float r = s_red[0] + s_red[1] + s_red[2] + s_red[3];
  __syncthreads();
  return r;
}

// clarity_score of m unit rows whose column sums have the squared norm `sq` (scores.py:46 with n = m); NaN below two rows
__device__ inline float facet_clarity(float sq_of_mean, int m) {
  if (m < 2) return __builtin_nanf("");
  return (sq_of_mean - 1.f / (float)m) / (float)(m - 1) * (float)m;
}

// per-cluster sizes of one component into s_cnt[0..kc); labels outside [0, kc) belong to no facet.  Ends with a barrier.
__device__ inline void facet_counts(const int32_t* __restrict__ Lc, int n, int kc, int* s_cnt) {
  if (threadIdx.x < kMaxFacets) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  for (int i = threadIdx.x; i < n; i += 256) {
    const int lab = Lc[i];
    if (lab >= 0 && lab < kc) atomicAdd(&s_cnt[lab], 1);  // integer adds in LDS: the order does not matter
  }
  __syncthreads();
}

template <int PPL, int KCT>  // 16-byte pieces per lane and row; accumulator sets (a power of two >= kc)
__global__ __launch_bounds__(256) void facet_rows_kernel(const float* __restrict__ V, int64_t C, int n, int D,
                                                          const int32_t* __restrict__ labels, int kc,
                                                          float* __restrict__ centres, int32_t* __restrict__ counts,
                                                          float* __restrict__ clarity) {
  constexpr int RB = (16 / PPL) < 1 ? 1 : ((16 / PPL) > 8 ? 8 : (16 / PPL));  // rows per batch: <= 16 loads in flight per lane
  extern __shared__ __align__(16) float s_dyn[];  // [4 waves][raw, normalised][PPL * 256]
  __shared__ float s_red[4];
  __shared__ int s_cnt[kMaxFacets];
  constexpr int W = PPL * 256;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform for the compiler too: labels load as scalars
  const int pieces = D / 4;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const float4* Vc = reinterpret_cast<const float4*>(V + c * (int64_t)n * D);
    const int32_t* Lc = labels + c * (int64_t)n;
    facet_counts(Lc, n, kc, s_cnt);
    float4 raw[KCT][PPL], nrm[KCT][PPL];
#pragma unroll
    for (int j = 0; j < KCT; ++j)
#pragma unroll
      for (int p = 0; p < PPL; ++p) raw[j][p] = nrm[j][p] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j0 = w; j0 < n; j0 += 4 * RB) {
      float4 v[RB][PPL];
      int lab[RB];
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        const int j = j0 + 4 * r;
        lab[r] = j < n ? Lc[j] : -1;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          const int q = p * 64 + lane;
          v[r][p] = (j < n && q < pieces) ? Vc[(int64_t)j * pieces + q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        float s = 0.f;
#pragma unroll
        for (int p = 0; p < PPL; ++p) s += v[r][p].x * v[r][p].x + v[r][p].y * v[r][p].y + v[r][p].z * v[r][p].z + v[r][p].w * v[r][p].w;
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        const float rn = 1.f / fmaxf(sqrtf(s), 1e-12f);  // F.normalize, scores.py:45
#pragma unroll
        for (int j = 0; j < KCT; ++j) {
          if (lab[r] == j && j < kc) {  // wave-uniform
#pragma unroll
            for (int p = 0; p < PPL; ++p) {
              raw[j][p].x += v[r][p].x;
              raw[j][p].y += v[r][p].y;
              raw[j][p].z += v[r][p].z;
              raw[j][p].w += v[r][p].w;
              nrm[j][p].x += v[r][p].x * rn;
              nrm[j][p].y += v[r][p].y * rn;
              nrm[j][p].z += v[r][p].z * rn;
              nrm[j][p].w += v[r][p].w * rn;
            }
          }
        }
      }
    }
    // the four waves' sums meet in LDS, one cluster at a time; waves in the order 0, 1, 2, 3
#pragma unroll
    for (int j = 0; j < KCT; ++j) {
      if (j < kc) {
        float* mine = s_dyn + (size_t)w * 2 * W;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          *reinterpret_cast<float4*>(&mine[(p * 64 + lane) * 4]) = raw[j][p];
          *reinterpret_cast<float4*>(&mine[W + (p * 64 + lane) * 4]) = nrm[j][p];
        }
        __syncthreads();
        const int m = s_cnt[j];
        float* out = centres + (c * kc + j) * (int64_t)D;
        float part = 0.f;
        for (int f = threadIdx.x; f < D; f += 256) {
          const float r = s_dyn[f] + s_dyn[2 * W + f] + s_dyn[4 * W + f] + s_dyn[6 * W + f];
          const float u = s_dyn[W + f] + s_dyn[3 * W + f] + s_dyn[5 * W + f] + s_dyn[7 * W + f];
          out[f] = m > 0 ? r / (float)m : 0.f;
          const float mean = m > 0 ? u / (float)m : 0.f;
          part += mean * mean;
        }
        const float tot = facet_block_sum(part, s_red);  // ends with a barrier: s_dyn is free again
        if (threadIdx.x == 0) {
          counts[c * kc + j] = m;
          if (clarity) clarity[c * kc + j] = facet_clarity(tot, m);
        }
      }
    }
    __syncthreads();  // s_cnt is rewritten by the next component
  }
}

__global__ __launch_bounds__(256) void facet_cols_kernel(const float* __restrict__ V, int64_t C, int n, int64_t D,
                                                          const int32_t* __restrict__ labels, int kc,
                                                          float* __restrict__ centres, int32_t* __restrict__ counts,
                                                          float* __restrict__ clarity) {
  __shared__ float s_rn[kMaxFacetRows];
  __shared__ int s_lab[kMaxFacetRows];
  __shared__ float s_red[4];
  __shared__ int s_cnt[kMaxFacets];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t c = blockIdx.x; c < C; c += gridDim.x) {
    const float* Vc = V + c * (int64_t)n * D;
    const int32_t* Lc = labels + c * (int64_t)n;
    facet_counts(Lc, n, kc, s_cnt);
    for (int i = threadIdx.x; i < n; i += 256) {
      const int lab = Lc[i];
      s_lab[i] = (lab >= 0 && lab < kc) ? lab : -1;
    }
    for (int i = w; i < n; i += 4) {
      const float* p = Vc + (int64_t)i * D;
      float s = 0.f;
      for (int64_t f = lane; f < D; f += 64) s += p[f] * p[f];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (lane == 0) s_rn[i] = 1.f / fmaxf(sqrtf(s), 1e-12f);
    }
    __syncthreads();
    for (int j = 0; j < kc; ++j) {
      const int m = s_cnt[j];
      float* out = centres + (c * kc + j) * D;
      float part = 0.f;
      for (int64_t f = threadIdx.x; f < D; f += 256) {
        float r = 0.f, u = 0.f;
        for (int i = 0; i < n; ++i) {
          if (s_lab[i] == j) {  // the same for every thread of the workgroup
            const float v = Vc[(int64_t)i * D + f];
            r += v;
            u += v * s_rn[i];
          }
        }
        out[f] = m > 0 ? r / (float)m : 0.f;
        const float mean = m > 0 ? u / (float)m : 0.f;
        part += mean * mean;
      }
      const float tot = facet_block_sum(part, s_red);
      if (threadIdx.x == 0) {
        counts[c * kc + j] = m;
        if (clarity) clarity[c * kc + j] = facet_clarity(tot, m);
      }
    }
    __syncthreads();  // s_rn / s_lab / s_cnt are rewritten by the next component
  }
}

template <int PPL, int KCT>
int launch_rows(ProfScope& prof, unsigned blocks, hipStream_t st, const float* V, int64_t C, int n, int D, const int32_t* labels,
                int kc, float* centres, int32_t* counts, float* clarity) {
  const size_t smem = (size_t)4 * 2 * PPL * 256 * sizeof(float);
  if (smem > 48 * 1024)
    SL_CHECK_HIP(hipFuncSetAttribute((const void*)facet_rows_kernel<PPL, KCT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
  SL_LAUNCH(prof, (facet_rows_kernel<PPL, KCT>), dim3(blocks), dim3(256), smem, st, V, C, n, D, labels, kc, centres, counts, clarity);
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_facet_stats(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* d_labels, int n_clusters,
                          float* d_centres, int32_t* d_counts, float* d_clarity, void* stream) {
  SL_REQUIRE(C >= 0 && n >= 0 && D >= 0, "sl_facet_stats: negative shape");
  SL_REQUIRE(n_clusters >= 1 && n_clusters <= kMaxFacets, "sl_facet_stats: n_clusters=%d not in [1, %d]", n_clusters, kMaxFacets);
  SL_REQUIRE(n <= kMaxFacetRows, "sl_facet_stats: n_samples=%lld exceeds the supported maximum %d", (long long)n, kMaxFacetRows);
  if (C == 0) return 0;
  SL_REQUIRE(n >= 1 && D >= 1, "sl_facet_stats: n_samples=%lld, D=%lld: both must be at least 1", (long long)n, (long long)D);
  SL_REQUIRE(d_V && d_labels && d_centres && d_counts, "sl_facet_stats: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const int kc = n_clusters;
  int kct = 2;
  while (kct < kc) kct *= 2;
  const int64_t ppl = (D / 4 + 63) / 64;
  const bool fast = (D % 4) == 0 && ppl * kct <= kFastBudget && (((uintptr_t)d_V) & 15) == 0;
  ProfScope prof(SL_PROF_SCORES, st, (double)C * n * D * 4);
  int64_t blocks = C;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (blocks > cap) blocks = cap;
  if (!fast) {
    SL_LAUNCH(prof, facet_cols_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_V, C, (int)n, D, d_labels, kc, d_centres, d_counts,
              d_clarity);
    SL_CHECK_HIP(hipGetLastError());
    return 0;
  }
  int rc = 0;
#define SL_FACET(P_, K_)                                                                                                        \
  case P_:                                                                                                                      \
    rc = launch_rows<P_, K_>(prof, (unsigned)blocks, st, d_V, C, (int)n, (int)D, d_labels, kc, d_centres, d_counts, d_clarity); \
    break
  switch (kct) {
    case 2:
      switch ((int)ppl) {
        SL_FACET(1, 2);
        SL_FACET(2, 2);
        SL_FACET(3, 2);
        SL_FACET(4, 2);
        SL_FACET(5, 2);
        SL_FACET(6, 2);
        SL_FACET(7, 2);
        SL_FACET(8, 2);
      }
      break;
    case 4:
      switch ((int)ppl) {
        SL_FACET(1, 4);
        SL_FACET(2, 4);
        SL_FACET(3, 4);
        SL_FACET(4, 4);
      }
      break;
    case 8:
      switch ((int)ppl) {
        SL_FACET(1, 8);
        SL_FACET(2, 8);
      }
      break;
    default:
      rc = launch_rows<1, 16>(prof, (unsigned)blocks, st, d_V, C, (int)n, (int)D, d_labels, kc, d_centres, d_counts, d_clarity);
  }
#undef SL_FACET
  if (rc) return rc;
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
