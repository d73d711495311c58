// K16 — the probed model's inference BatchNorm as one pass over memory, with the ReLU and the residual add that follow it
// fused in.  y = scale * ((x - mean) * rsqrt(var + eps)) + bias over a contiguous NCHW fp32 tensor, then
//   EPI_PLAIN     nothing
//   EPI_RELU      clamp_min(y, 0)
//   EPI_ADD_RELU  clamp_min(y + residual, 0)
// HBM-bound: one read of x (and of the residual), one write of y.
//
// The contract is bit equality with what the model computes unfused (MIOpen's inference BatchNorm, then ATen's add and clamp_min),
// so the arithmetic below restates those kernels operation by operation and this file is compiled with -ffp-contract=off: the
// compiler may neither fuse the subtract/multiply nor split the multiply-add.  The forms below are the ones that matched on the
// device on a sweep of 6.6 x 10^6 random variances and inputs (DESIGN.md §K16 lists the candidates that did not).
//
// Per-channel constants are read from the module's tensors on every launch and the inverse standard deviation is computed here:
// every block builds a {mean, inv_std, scale, bias} table of the C channels in LDS (C <= 4096), nothing survives the launch.
#include "common.hpp"

namespace sl {
namespace {

typedef float f4 __attribute__((ext_vector_type(4)));

enum { EPI_PLAIN = 0, EPI_RELU = 1, EPI_ADD_RELU = 2 };
enum { POL_PLAIN = 0, POL_NT_STORE = 1, POL_NT_BOTH = 2 };

constexpr int kBlock = 256;
constexpr int kUnroll = 4;         // 16-byte pieces per lane in flight
constexpr int64_t kMaxC = 4096;    // 64 KiB of LDS for the table
constexpr int64_t kMaxTotal = (int64_t)1 << 31;

// MIOpen's form: the estimate is added in fp32 and the root is the hardware's v_rsq_f32 (not a divide by a square root, not the
// double-precision route: DESIGN.md K16 counts what each of those misses).
__device__ inline float bn_inv_std(float var, double eps) { return __builtin_amdgcn_rsqf(fabsf(var + (float)eps)); }

// k = {mean, inv_std, scale, bias}
__device__ inline float bn_value(float x, const f4 k) {
  const float xhat = (x - k.x) * k.y;
  return __fmaf_rn(k.z, xhat, k.w);  // one rounding: a separate multiply and add differs in a quarter of the elements
}

// ATen's clamp_min functor: NaN passes through with its bits, max(-0.0, 0) is +0.0
__device__ inline float relu_clamp(float v) { return v != v ? v : fmaxf(v, 0.f); }

template <int EPI>
__device__ inline float bn_finish(float x, const f4 k, float r) {
  float y = bn_value(x, k);
  if constexpr (EPI == EPI_ADD_RELU) y = y + r;  // y is an fp32 value here, as when it went through memory
  if constexpr (EPI != EPI_PLAIN) y = relu_clamp(y);
  return y;
}

template <int POL>
__device__ inline f4 ld4(const f4* p) {
  if constexpr (POL == POL_NT_BOTH) return __builtin_nontemporal_load(p);
  return *p;
}
template <int POL>
__device__ inline void st4(f4* p, f4 v) {
  if constexpr (POL != POL_PLAIN)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// ALIGNED: HW % 4 == 0, a 16-byte piece never leaves its (n, c) plane.  Pieces are dealt to waves in runs of 64 * kUnroll; a run
// of 64 pieces that lies inside one plane takes its constants once (a wave-uniform LDS read), every other run looks its channel
// up per lane.  Without ALIGNED (HW = 49) a piece may cross planes: the channel is advanced element by element.
template <int EPI, bool ALIGNED, int POL>
__global__ __launch_bounds__(kBlock) void batchnorm_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           float* __restrict__ y, const float* __restrict__ mean,
                                                           const float* __restrict__ var, const float* __restrict__ scale,
                                                           const float* __restrict__ bias, double eps, uint32_t C, uint32_t HW,
                                                           uint32_t total) {
  extern __shared__ f4 tab[];
  for (uint32_t c = threadIdx.x; c < C; c += kBlock) tab[c] = f4{mean[c], bn_inv_std(var[c], eps), scale[c], bias[c]};
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63;
  const uint32_t wave = blockIdx.x * (kBlock / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * (kBlock / 64);
  const uint32_t n4 = total / 4;
  const uint32_t per_plane = ALIGNED ? HW / 4 : 1;
  const f4* x4 = reinterpret_cast<const f4*>(x);
  const f4* r4 = reinterpret_cast<const f4*>(res);
  f4* y4 = reinterpret_cast<f4*>(y);

  // (n4 is below 2^29, so base + 64 * kUnroll cannot wrap)
  for (uint32_t base = wave * (64 * kUnroll); base < n4; base += nwaves * (64 * kUnroll)) {
    f4 v[kUnroll], r[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t i = base + u * 64 + lane;
      if (i < n4) {
        v[u] = ld4<POL>(x4 + i);
        if constexpr (EPI == EPI_ADD_RELU) r[u] = ld4<POL>(r4 + i);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const uint32_t first = base + u * 64, i = first + lane;
      if (first >= n4) break;  // wave-uniform
      f4 o;
      if constexpr (ALIGNED) {
        const uint32_t p0 = first / per_plane;  // wave-uniform
        const uint32_t last = first + 63 < n4 ? first + 63 : n4 - 1;
        uint32_t c;
        if (last - p0 * per_plane < per_plane)
          c = p0 % C;
        else
          c = (i < n4 ? i / per_plane : 0u) % C;
        if (i < n4) {
          const f4 k = tab[c];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = bn_finish<EPI>(v[u][j], k, EPI == EPI_ADD_RELU ? r[u][j] : 0.f);
        }
      } else {
        if (i < n4) {
          const uint32_t e = i * 4, p = e / HW;
          uint32_t off = e - p * HW, c = p % C;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = bn_finish<EPI>(v[u][j], tab[c], EPI == EPI_ADD_RELU ? r[u][j] : 0.f);
            if (++off == HW) {
              off = 0;
              if (++c == C) c = 0;
            }
          }
        }
      }
      if (i < n4) st4<POL>(y4 + i, o);
    }
  }
  // the last total % 4 elements (none when HW % 4 == 0)
  if (blockIdx.x == 0 && threadIdx.x < (total & 3u)) {
    const uint32_t e = (total & ~3u) + threadIdx.x;
    y[e] = bn_finish<EPI>(x[e], tab[(e / HW) % C], EPI == EPI_ADD_RELU ? res[e] : 0.f);
  }
}

template <int EPI, bool ALIGNED>
void launch_policy(ProfScope& prof, int pol, dim3 grid, size_t lds, hipStream_t st, const float* x, const float* res, float* y,
                   const float* mean, const float* var, const float* scale, const float* bias, double eps, uint32_t C,
                   uint32_t HW, uint32_t total) {
#define SL_BN_LAUNCH(P_) \
  SL_LAUNCH(prof, (batchnorm_kernel<EPI, ALIGNED, P_>), grid, dim3(kBlock), lds, st, x, res, y, mean, var, scale, bias, eps, C, HW, total)
  switch (pol) {
    case POL_PLAIN: SL_BN_LAUNCH(POL_PLAIN); break;
    case POL_NT_STORE: SL_BN_LAUNCH(POL_NT_STORE); break;
    default: SL_BN_LAUNCH(POL_NT_BOTH); break;
  }
#undef SL_BN_LAUNCH
}

int launch_batchnorm(int epi, const float* x, const float* res, float* y, const float* mean, const float* var,
                     const float* scale, const float* bias, double eps, int64_t B, int64_t C, int64_t HW, hipStream_t st,
                     const char* who) {
  SL_REQUIRE(B >= 0 && C >= 0 && HW >= 0, "%s: negative shape", who);
  const int64_t total = B * C * HW;
  if (total == 0) return 0;
  SL_REQUIRE(x && y && mean && var && scale && bias && (epi != EPI_ADD_RELU || res), "%s: null pointer", who);
  SL_REQUIRE(C <= kMaxC, "%s: %lld channels exceed the supported maximum of %lld", who, (long long)C, (long long)kMaxC);
  SL_REQUIRE(total < kMaxTotal, "%s: %lld elements exceed the supported maximum of 2^31 - 1", who, (long long)total);
  SL_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)res) & 15) == 0, "%s: tensors must be 16-byte aligned", who);
  const int passes = epi == EPI_ADD_RELU ? 3 : 2;
  ProfScope prof(SL_PROF_BATCHNORM, st, (double)total * 4 * passes);
  // sl_set_option("bn_policy", 1 plain / 2 non-temporal stores / 3 non-temporal loads and stores); 0 = the rule below
  int pol = (int)option(OPT_BN_POLICY) - 1;
  if (pol < 0 || pol > POL_NT_BOTH) pol = POL_PLAIN;
  const int64_t per_block = (int64_t)kBlock * kUnroll * 4;
  int64_t blocks = (total + per_block - 1) / per_block;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks);
  const size_t lds = (size_t)C * sizeof(f4);
#define SL_BN_EPI(E_)                                                                                                      \
  if (HW % 4 == 0)                                                                                                         \
    launch_policy<E_, true>(prof, pol, grid, lds, st, x, res, y, mean, var, scale, bias, eps, (uint32_t)C, (uint32_t)HW,   \
                            (uint32_t)total);                                                                              \
  else                                                                                                                     \
    launch_policy<E_, false>(prof, pol, grid, lds, st, x, res, y, mean, var, scale, bias, eps, (uint32_t)C, (uint32_t)HW,  \
                             (uint32_t)total)
  switch (epi) {
    case EPI_PLAIN: SL_BN_EPI(EPI_PLAIN); break;
    case EPI_RELU: SL_BN_EPI(EPI_RELU); break;
    default: SL_BN_EPI(EPI_ADD_RELU); break;
  }
#undef SL_BN_EPI
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_batchnorm_infer(const float* d_x, int64_t B, int64_t C, int64_t HW, const float* d_mean, const float* d_var,
                              const float* d_scale, const float* d_bias, double eps, int relu, float* d_y, void* stream) {
  return launch_batchnorm(relu ? EPI_RELU : EPI_PLAIN, d_x, nullptr, d_y, d_mean, d_var, d_scale, d_bias, eps, B, C, HW,
                          (hipStream_t)stream, "sl_batchnorm_infer");
}

SL_API int sl_batchnorm_infer_add_relu(const float* d_x, const float* d_residual, int64_t B, int64_t C, int64_t HW,
                                       const float* d_mean, const float* d_var, const float* d_scale, const float* d_bias,
                                       double eps, float* d_y, void* stream) {
  return launch_batchnorm(EPI_ADD_RELU, d_x, d_residual, d_y, d_mean, d_var, d_scale, d_bias, eps, B, C, HW, (hipStream_t)stream,
                          "sl_batchnorm_infer_add_relu");
}
