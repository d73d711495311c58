// K16 — the probed model's inference BatchNorm as one pass over memory, with the ReLU and the residual add that follow it
// fused in.  y = scale * ((x - mean) * rsqrt(var + eps)) + bias over a contiguous NCHW fp32 tensor, then
//   EPI_PLAIN     nothing
//   EPI_RELU      clamp_min(y, 0)
//   EPI_ADD_RELU  clamp_min(y + residual, 0)
//   EPI_ADD_BN_RELU  clamp_min(y + y_b, 0), y_b the BatchNorm of a second tensor under its own constants: the tail of a stage's
//                  first block, whose shortcut ends in a BatchNorm
// HBM-bound: one read of x (and of the residual or the second tensor), one write of y.
// K18 adds the stem's epilogue, max_pool2d(clamp_min(y, 0)): one read of x, one write of the pooled quarter;
// neither the normalised tensor nor ATen's int64 indices go through memory.
//
// The contract is bit equality with what the model computes unfused (MIOpen's inference BatchNorm, then ATen's add and clamp_min),
// so the arithmetic below restates those kernels operation by operation and this file is compiled with -ffp-contract=off: the
// compiler may neither fuse the subtract/multiply nor split the multiply-add.  The forms below are the ones that matched on the
// device on a sweep of 6.6 x 10^6 random variances and inputs (DESIGN.md §K16 lists the candidates that did not).
//
// Per-channel constants are read from the module's tensors on every launch and the inverse standard deviation is computed here:
// every block builds a {mean, inv_std, scale, bias} table of the C channels in LDS (C <= 4096), nothing survives the launch.
// EPI_ADD_BN_RELU keeps two such tables, one behind the other, and takes C <= 2048: the same 64 KiB.
//
// SL_PROF_BATCHNORM counts BatchNorm2d evaluations, so a call of EPI_ADD_BN_RELU leaves two records in the slot: the kernel's
// (its time, 3 x total x 4 bytes) and an empty one (work 0, its two events recorded back to back on the stream).  The slot's
// time and bytes are the kernels'; its time over its count is not a per-launch average.
#include "bn_apply.hpp"

namespace sl {
namespace {

enum { POL_PLAIN = 0, POL_NT_STORE = 1, POL_NT_BOTH = 2 };

constexpr int kBlock = 256;
constexpr int kUnroll = 4;         // 16-byte pieces per lane in flight
constexpr int64_t kMaxC = 4096;    // 64 KiB of LDS for the table
constexpr int64_t kMaxCDual = 2048;  // EPI_ADD_BN_RELU: two tables in the same 64 KiB
constexpr int64_t kLdsPerCu = 160 * 1024;
constexpr size_t kDualResidentFrom = 32 * 1024;  // EPI_ADD_BN_RELU: above this many bytes of tables the grid is the resident blocks
constexpr int64_t kMaxTotal = (int64_t)1 << 31;

// bn_inv_std, bn_value, relu_clamp, add_as_aten, BnParams and bn_finish: bn_apply.hpp (conv_tail.hip applies them too)

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
template <int POL>
__device__ inline float ld1(const float* p) {
  if constexpr (POL == POL_NT_BOTH) return __builtin_nontemporal_load(p);
  return *p;
}
template <int POL>
__device__ inline void st1(float* p, float v) {
  if constexpr (POL != POL_PLAIN)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}

// ALIGNED: HW % 4 == 0, a 16-byte piece never leaves its (n, c) plane.  Pieces are dealt to waves in runs of 64 * kUnroll; a run
// of 64 pieces that lies inside one plane takes its constants once (a wave-uniform LDS read), every other run looks its channel
// up per lane.  Without ALIGNED (HW = 49) a piece may cross planes: the channel is advanced element by element.
// EPI_ADD_BN_RELU: `res` is the second tensor, `b` its BatchNorm, and tab[C + c] holds b's constants of channel c.
template <int EPI, bool ALIGNED, int POL>
__global__ __launch_bounds__(kBlock) void batchnorm_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                           float* __restrict__ y, const BnParams a, const BnParams b, uint32_t C,
                                                           uint32_t HW, uint32_t total) {
  constexpr bool HAS_RES = EPI == EPI_ADD_RELU || EPI == EPI_ADD_BN_RELU;
  constexpr bool DUAL = EPI == EPI_ADD_BN_RELU;
  extern __shared__ f4 tab[];
  for (uint32_t c = threadIdx.x; c < C; c += kBlock) {
    tab[c] = bn_constants(a, c);
    if constexpr (DUAL) tab[C + c] = bn_constants(b, c);
  }
  __syncthreads();
  const uint32_t second = DUAL ? C : 0u;  // tab[second + c]: the second tensor's constants (unused otherwise)

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
        if constexpr (HAS_RES) r[u] = ld4<POL>(r4 + i);
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
          const f4 k = tab[c], kb = tab[second + c];
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = bn_finish<EPI>(v[u][j], k, HAS_RES ? r[u][j] : 0.f, kb);
        }
      } else {
        if (i < n4) {
          const uint32_t e = i * 4, p = e / HW;
          uint32_t off = e - p * HW, c = p % C;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = bn_finish<EPI>(v[u][j], tab[c], HAS_RES ? r[u][j] : 0.f, tab[second + c]);
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
    const uint32_t c = (e / HW) % C;
    y[e] = bn_finish<EPI>(x[e], tab[c], HAS_RES ? res[e] : 0.f, tab[second + c]);
  }
}

template <int EPI, bool ALIGNED>
void launch_policy(ProfScope& prof, int pol, dim3 grid, size_t lds, hipStream_t st, const float* x, const float* res, float* y,
                   const BnParams& a, const BnParams& b, uint32_t C, uint32_t HW, uint32_t total) {
#define SL_BN_LAUNCH(P_) \
  SL_LAUNCH(prof, (batchnorm_kernel<EPI, ALIGNED, P_>), grid, dim3(kBlock), lds, st, x, res, y, a, b, C, HW, total)
  switch (pol) {
    case POL_PLAIN: SL_BN_LAUNCH(POL_PLAIN); break;
    case POL_NT_STORE: SL_BN_LAUNCH(POL_NT_STORE); break;
    default: SL_BN_LAUNCH(POL_NT_BOTH); break;
  }
#undef SL_BN_LAUNCH
}

// sl_set_option("bn_policy", 1 plain / 2 non-temporal stores / 3 non-temporal loads and stores); 0 = the rule: non-temporal
// loads and stores for a tensor of 206 MB (256 x 64 x 56 x 56 fp32) or more, plain below.  Standalone the non-temporal form is
// faster from that size on and equal below; in the pipeline it won every interleaved headline run.
constexpr int64_t kNtFromBytes = (int64_t)256 * 64 * 56 * 56 * 4;

int bn_policy(int64_t tensor_bytes) {
  const int pol = (int)option(OPT_BN_POLICY) - 1;
  if (pol < 0 || pol > POL_NT_BOTH) return tensor_bytes >= kNtFromBytes ? POL_NT_BOTH : POL_PLAIN;
  return pol;
}

int launch_batchnorm(int epi, const float* x, const float* res, float* y, const BnParams& a, const BnParams& b, int64_t B,
                     int64_t C, int64_t HW, hipStream_t st, const char* who) {
  const bool dual = epi == EPI_ADD_BN_RELU;
  SL_REQUIRE(B >= 0 && C >= 0 && HW >= 0, "%s: negative shape", who);
  const int64_t total = B * C * HW;
  if (total == 0) return 0;
  SL_REQUIRE(x && y && a.mean && a.var && a.scale && a.bias && (epi < EPI_ADD_RELU || res), "%s: null pointer", who);
  SL_REQUIRE(!dual || (b.mean && b.var && b.scale && b.bias), "%s: null pointer", who);
  const int64_t max_c = dual ? kMaxCDual : kMaxC;
  SL_REQUIRE(C <= max_c, "%s: %lld channels exceed the supported maximum of %lld", who, (long long)C, (long long)max_c);
  SL_REQUIRE(total < kMaxTotal, "%s: %lld elements exceed the supported maximum of 2^31 - 1", who, (long long)total);
  SL_REQUIRE((((uintptr_t)x | (uintptr_t)y | (uintptr_t)res) & 15) == 0, "%s: tensors must be 16-byte aligned", who);
  const int passes = epi >= EPI_ADD_RELU ? 3 : 2;
  ProfScope prof(SL_PROF_BATCHNORM, st, (double)total * 4 * passes);
  const int pol = bn_policy(total * 4);
  const size_t lds = (size_t)C * sizeof(f4) * (dual ? 2 : 1);
  const int64_t per_block = (int64_t)kBlock * kUnroll * 4;
  int64_t blocks = (total + per_block - 1) / per_block;
  int64_t per_cu = 8;
  // every block builds both tables, 40 bytes read and two v_rsq_f32 per channel.  Above 32 KiB of tables (C > 1024) the grid
  // is the blocks resident at once (two per CU at C = 2048), so that a CU builds them once per resident block and not once
  // per round: 80 against 84 us at (256, 2048, 7, 7).  At 32 KiB, where five blocks are resident, the same cut cost 128
  // against 105 us at (256, 1024, 14, 14), so up to there the grid stays at 8 blocks per CU.
  if (dual && lds > kDualResidentFrom) per_cu = kLdsPerCu / (int64_t)lds;
  const int64_t cap = (int64_t)num_cus() * per_cu;
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks);
#define SL_BN_EPI(E_)                                                                                                \
  if (HW % 4 == 0)                                                                                                   \
    launch_policy<E_, true>(prof, pol, grid, lds, st, x, res, y, a, b, (uint32_t)C, (uint32_t)HW, (uint32_t)total);  \
  else                                                                                                               \
    launch_policy<E_, false>(prof, pol, grid, lds, st, x, res, y, a, b, (uint32_t)C, (uint32_t)HW, (uint32_t)total)
  switch (epi) {
    case EPI_PLAIN: SL_BN_EPI(EPI_PLAIN); break;
    case EPI_RELU: SL_BN_EPI(EPI_RELU); break;
    case EPI_ADD_RELU: SL_BN_EPI(EPI_ADD_RELU); break;
    default: SL_BN_EPI(EPI_ADD_BN_RELU); break;
  }
#undef SL_BN_EPI
  SL_CHECK_HIP(hipGetLastError());
  if (dual) {  // the second BatchNorm2d of this call: a record of its own with no work and no time (see the head of the file)
    ProfScope second(SL_PROF_BATCHNORM, st, 0.0);
    if (second.start) {
      SL_CHECK_HIP(hipEventRecord(second.start, st));
      SL_CHECK_HIP(hipEventRecord(second.stop, st));
    }
  }
  return 0;
}

// ---- K18: relu(bn(x)) staged in LDS, max-pooled from there ---------------------------------------------------------------------
// A block owns a band of output rows of one (n, c) plane (the whole plane when it fits: 112 x 112 is 49 KiB).  It loads the input
// rows the band's windows touch once, applies bn_value and relu_clamp once per element, keeps the result in LDS and pools out of
// it, so an element is normalised once however many windows cover it; bands of one plane re-read only the kh - sh rows they share.
// The plane's four constants are wave-uniform: no table.
//
// ATen's max_pool_forward_nchw: the window is clipped to the input, the maximum starts at -inf, elements are visited row-major
// and `v > max || isnan(v)` replaces it, so a window with NaNs yields the last one in scan order, payload included.  Positions
// outside the input read as -inf here, which that rule never selects (every window holds at least one real element: p <= k / 2).
constexpr int64_t kPoolLds = 64 * 1024;  // staged rows per block
constexpr int64_t kPoolMaxW = 4096;      // so that kh <= 3 rows always fit

struct PoolGeom {
  uint32_t C, H, W, OH, OW, kh, kw, sh, sw, ph, pw;
  uint32_t rows, bands;  // output rows per band, bands per plane
  uint32_t nwork;        // planes x bands: what the blocks of the (capped) grid loop over
};

struct PoolBand {
  uint32_t plane, o0, o1, r0, r1;  // output rows [o0, o1) need input rows [r0, r1)
  f4 k;
};

__device__ inline PoolBand pool_band(const PoolGeom& g, uint32_t work, const float* mean, const float* var, const float* scale,
                                     const float* bias, double eps) {
  PoolBand b;
  b.plane = work / g.bands;
  const uint32_t band = work - b.plane * g.bands, c = b.plane % g.C;
  b.k = f4{mean[c], bn_inv_std(var[c], eps), scale[c], bias[c]};
  b.o0 = band * g.rows;
  b.o1 = b.o0 + g.rows < g.OH ? b.o0 + g.rows : g.OH;
  const int top = (int)(b.o0 * g.sh) - (int)g.ph;
  b.r0 = top > 0 ? (uint32_t)top : 0u;
  const uint32_t bottom = (b.o1 - 1) * g.sh + g.kh - g.ph;  // (ph < kh)
  b.r1 = bottom < g.H ? bottom : g.H;
  return b;
}

__device__ inline float pool_take(float m, float v) { return v > m || v != v ? v : m; }

// W % 4 == 0 and OW % 4 == 0: 16-byte loads, LDS accesses and stores.  A lane pools 4 adjacent outputs of one row; their windows
// span 3 * SW + KW <= 9 input columns, which start at float 3 (PW = 1) or 0 (PW = 0) of an aligned 16-byte piece of the staged
// row, so every row of the windows is at most three ds_read_b128 at compile-time offsets.
template <int KW, int SW, int PW, int POL>
__global__ __launch_bounds__(kBlock) void bn_relu_maxpool_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                 const float* __restrict__ mean, const float* __restrict__ var,
                                                                 const float* __restrict__ scale, const float* __restrict__ bias,
                                                                 double eps, const PoolGeom g) {
  extern __shared__ f4 staged[];
  for (uint32_t work = blockIdx.x; work < g.nwork; work += gridDim.x) {
    const PoolBand b = pool_band(g, work, mean, var, scale, bias, eps);
    const uint32_t w4 = g.W / 4, n4 = (b.r1 - b.r0) * w4;
    const f4* src = reinterpret_cast<const f4*>(x + (size_t)b.plane * g.H * g.W) + (size_t)b.r0 * w4;
    for (uint32_t base = 0; base < n4; base += kBlock * kUnroll) {
      f4 v[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t i = base + u * kBlock + threadIdx.x;
        if (i < n4) v[u] = ld4<POL>(src + i);
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const uint32_t i = base + u * kBlock + threadIdx.x;
        if (i < n4) {
          f4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = relu_clamp(bn_value(v[u][j], b.k));
          staged[i] = o;
        }
      }
    }
    __syncthreads();

    constexpr int OFF = PW ? 3 : 0, SPAN = 3 * SW + KW, PIECES = (OFF + SPAN + 3) / 4;
    constexpr float NEG_INF = -__builtin_huge_valf();
    const uint32_t ow4 = g.OW / 4, npieces = (b.o1 - b.o0) * ow4;
    f4* dst = reinterpret_cast<f4*>(y + (size_t)b.plane * g.OH * g.OW);
    for (uint32_t p = threadIdx.x; p < npieces; p += kBlock) {
      const uint32_t orow = p / ow4, q = p - orow * ow4, oh = b.o0 + orow;
      const int col0 = (int)(q * 4 * SW) - (PW ? 4 : 0);  // the first piece's column: a multiple of 4, -4 at the left edge
      f4 m = {NEG_INF, NEG_INF, NEG_INF, NEG_INF};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const int ih = (int)(oh * g.sh) - (int)g.ph + i;
        if (i < (int)g.kh && ih >= 0 && ih < (int)g.H) {
          const f4* row = staged + (size_t)((uint32_t)ih - b.r0) * w4;
          float t[PIECES * 4];
#pragma unroll
          for (int s = 0; s < PIECES; ++s) {
            const int col = col0 + 4 * s;
            const f4 piece = col >= 0 && col < (int)g.W ? row[col >> 2] : f4{NEG_INF, NEG_INF, NEG_INF, NEG_INF};
#pragma unroll
            for (int j = 0; j < 4; ++j) t[4 * s + j] = piece[j];
          }
#pragma unroll
          for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int j = 0; j < KW; ++j) m[o] = pool_take(m[o], t[OFF + o * SW + j]);
          }
        }
      }
      st4<POL>(dst + (size_t)oh * ow4 + q, m);
    }
    __syncthreads();  // the next band overwrites the staged rows
  }
}

// Any W and OW: the same staging and the same scan, element by element.
template <int POL>
__global__ __launch_bounds__(kBlock) void bn_relu_maxpool_scalar_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                                        const float* __restrict__ mean,
                                                                        const float* __restrict__ var,
                                                                        const float* __restrict__ scale,
                                                                        const float* __restrict__ bias, double eps,
                                                                        const PoolGeom g) {
  extern __shared__ f4 staged[];
  float* rows = reinterpret_cast<float*>(staged);
  for (uint32_t work = blockIdx.x; work < g.nwork; work += gridDim.x) {
    const PoolBand b = pool_band(g, work, mean, var, scale, bias, eps);
    const uint32_t n = (b.r1 - b.r0) * g.W;
    const float* src = x + (size_t)b.plane * g.H * g.W + (size_t)b.r0 * g.W;
#pragma unroll 4
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) rows[i] = relu_clamp(bn_value(ld1<POL>(src + i), b.k));
    __syncthreads();

    const uint32_t nout = (b.o1 - b.o0) * g.OW;
    float* dst = y + (size_t)b.plane * g.OH * g.OW;
    for (uint32_t p = threadIdx.x; p < nout; p += kBlock) {
      const uint32_t orow = p / g.OW, ow = p - orow * g.OW, oh = b.o0 + orow;
      float m = -__builtin_huge_valf();
      for (uint32_t i = 0; i < g.kh; ++i) {
        const int ih = (int)(oh * g.sh) - (int)g.ph + (int)i;
        if (ih < 0 || ih >= (int)g.H) continue;
        for (uint32_t j = 0; j < g.kw; ++j) {
          const int iw = (int)(ow * g.sw) - (int)g.pw + (int)j;
          if (iw < 0 || iw >= (int)g.W) continue;
          m = pool_take(m, rows[((uint32_t)ih - b.r0) * g.W + (uint32_t)iw]);
        }
      }
      st1<POL>(dst + (size_t)oh * g.OW + ow, m);
    }
    __syncthreads();
  }
}

template <int KW, int SW, int PW>
void launch_pool_policy(ProfScope& prof, int pol, dim3 grid, size_t lds, hipStream_t st, const float* x, float* y,
                        const float* mean, const float* var, const float* scale, const float* bias, double eps,
                        const PoolGeom& g) {
#define SL_POOL_LAUNCH(P_) \
  SL_LAUNCH(prof, (bn_relu_maxpool_kernel<KW, SW, PW, P_>), grid, dim3(kBlock), lds, st, x, y, mean, var, scale, bias, eps, g)
  switch (pol) {
    case POL_PLAIN: SL_POOL_LAUNCH(POL_PLAIN); break;
    case POL_NT_STORE: SL_POOL_LAUNCH(POL_NT_STORE); break;
    default: SL_POOL_LAUNCH(POL_NT_BOTH); break;
  }
#undef SL_POOL_LAUNCH
}

int launch_bn_relu_maxpool(const float* x, float* y, const float* mean, const float* var, const float* scale, const float* bias,
                           double eps, int64_t B, int64_t C, int64_t H, int64_t W, int kh, int kw, int sh, int sw, int ph,
                           int pw, hipStream_t st, const char* who) {
  SL_REQUIRE(B >= 0 && C >= 0 && H >= 0 && W >= 0, "%s: negative shape", who);
  SL_REQUIRE((kh == 2 || kh == 3) && (kw == 2 || kw == 3), "%s: kernel size %d x %d is not supported (2 or 3 per axis)", who, kh,
             kw);
  SL_REQUIRE((sh == 1 || sh == 2) && (sw == 1 || sw == 2), "%s: stride %d x %d is not supported (1 or 2 per axis)", who, sh, sw);
  SL_REQUIRE(ph >= 0 && pw >= 0 && ph <= kh / 2 && pw <= kw / 2,
             "%s: padding %d x %d is not supported (at most half the kernel size)", who, ph, pw);
  const int64_t total = B * C * H * W;
  if (total == 0) return 0;
  // (before the pointers: such an input has no output, so the caller has no buffer to pass)
  SL_REQUIRE(H + 2 * ph >= kh && W + 2 * pw >= kw, "%s: a %lld x %lld input is smaller than the pooling window", who,
             (long long)H, (long long)W);
  SL_REQUIRE(x && y && mean && var && scale && bias, "%s: null pointer", who);
  SL_REQUIRE(C <= kMaxC, "%s: %lld channels exceed the supported maximum of %lld", who, (long long)C, (long long)kMaxC);
  SL_REQUIRE(total < kMaxTotal, "%s: %lld elements exceed the supported maximum of 2^31 - 1", who, (long long)total);
  SL_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 15) == 0, "%s: tensors must be 16-byte aligned", who);
  SL_REQUIRE(W <= kPoolMaxW, "%s: rows of %lld elements exceed the supported maximum of %lld", who, (long long)W,
             (long long)kPoolMaxW);
  PoolGeom g;
  g.C = (uint32_t)C, g.H = (uint32_t)H, g.W = (uint32_t)W;
  g.kh = kh, g.kw = kw, g.sh = sh, g.sw = sw, g.ph = ph, g.pw = pw;
  g.OH = (uint32_t)((H + 2 * ph - kh) / sh + 1), g.OW = (uint32_t)((W + 2 * pw - kw) / sw + 1);
  const int64_t fit = kPoolLds / (W * 4);  // input rows a block can stage (at least 4)
  int64_t in_rows = H;
  g.rows = g.OH, g.bands = 1;
  if (H > fit) {
    g.rows = (uint32_t)((fit - kh) / sh + 1);
    g.bands = (g.OH + g.rows - 1) / g.rows;
    in_rows = (int64_t)(g.rows - 1) * sh + kh;
  }
  const size_t lds = (size_t)(in_rows * W * 4 + 15) / 16 * 16;
  g.nwork = (uint32_t)(B * C * g.bands);  // (bands <= H: below 2^31 as the element count is)
  // as many blocks as are resident at once (160 KiB of LDS per CU, at most 8 blocks): with more, the last round of a grid
  // whose blocks each take several bands leaves CUs idle
  int64_t per_cu = kLdsPerCu / (int64_t)lds;
  per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
  const int64_t cap = (int64_t)num_cus() * per_cu;
  const dim3 grid((unsigned)(g.nwork < cap ? g.nwork : cap));
  ProfScope prof(SL_PROF_BATCHNORM, st, ((double)total + (double)B * C * g.OH * g.OW) * 4);
  const int pol = bn_policy(total * 4);
  if (W % 4 == 0 && g.OW % 4 == 0) {
#define SL_POOL_CASE(KW_, SW_, PW_)                                                                              \
  case (KW_ - 2) * 4 + (SW_ - 1) * 2 + PW_:                                                                      \
    launch_pool_policy<KW_, SW_, PW_>(prof, pol, grid, lds, st, x, y, mean, var, scale, bias, eps, g);           \
    break
    switch ((kw - 2) * 4 + (sw - 1) * 2 + pw) {
      SL_POOL_CASE(2, 1, 0);
      SL_POOL_CASE(2, 1, 1);
      SL_POOL_CASE(2, 2, 0);
      SL_POOL_CASE(2, 2, 1);
      SL_POOL_CASE(3, 1, 0);
      SL_POOL_CASE(3, 1, 1);
      SL_POOL_CASE(3, 2, 0);
      default: SL_POOL_CASE(3, 2, 1);
    }
#undef SL_POOL_CASE
  } else {
#define SL_POOL_SCALAR(P_) \
  SL_LAUNCH(prof, (bn_relu_maxpool_scalar_kernel<P_>), grid, dim3(kBlock), lds, st, x, y, mean, var, scale, bias, eps, g)
    switch (pol) {
      case POL_PLAIN: SL_POOL_SCALAR(POL_PLAIN); break;
      case POL_NT_STORE: SL_POOL_SCALAR(POL_NT_STORE); break;
      default: SL_POOL_SCALAR(POL_NT_BOTH); break;
    }
#undef SL_POOL_SCALAR
  }
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_batchnorm_infer(const float* d_x, int64_t B, int64_t C, int64_t HW, const float* d_mean, const float* d_var,
                              const float* d_scale, const float* d_bias, double eps, int relu, float* d_y, void* stream) {
  return launch_batchnorm(relu ? EPI_RELU : EPI_PLAIN, d_x, nullptr, d_y, BnParams{d_mean, d_var, d_scale, d_bias, eps}, BnParams{},
                          B, C, HW, (hipStream_t)stream, "sl_batchnorm_infer");
}

SL_API int sl_batchnorm_infer_add_relu(const float* d_x, const float* d_residual, int64_t B, int64_t C, int64_t HW,
                                       const float* d_mean, const float* d_var, const float* d_scale, const float* d_bias,
                                       double eps, float* d_y, void* stream) {
  return launch_batchnorm(EPI_ADD_RELU, d_x, d_residual, d_y, BnParams{d_mean, d_var, d_scale, d_bias, eps}, BnParams{}, B, C, HW,
                          (hipStream_t)stream, "sl_batchnorm_infer_add_relu");
}

SL_API int sl_batchnorm_infer_add_bn_relu(const float* d_xa, const float* d_mean_a, const float* d_var_a, const float* d_scale_a,
                                          const float* d_bias_a, double eps_a, const float* d_xb, const float* d_mean_b,
                                          const float* d_var_b, const float* d_scale_b, const float* d_bias_b, double eps_b,
                                          int64_t B, int64_t C, int64_t HW, float* d_y, void* stream) {
  return launch_batchnorm(EPI_ADD_BN_RELU, d_xa, d_xb, d_y, BnParams{d_mean_a, d_var_a, d_scale_a, d_bias_a, eps_a},
                          BnParams{d_mean_b, d_var_b, d_scale_b, d_bias_b, eps_b}, B, C, HW, (hipStream_t)stream,
                          "sl_batchnorm_infer_add_bn_relu");
}

SL_API int sl_batchnorm_infer_relu_maxpool(const float* d_x, int64_t B, int64_t C, int64_t H, int64_t W, const float* d_mean,
                                           const float* d_var, const float* d_scale, const float* d_bias, double eps, int kh,
                                           int kw, int sh, int sw, int ph, int pw, float* d_y, void* stream) {
  return launch_bn_relu_maxpool(d_x, d_y, d_mean, d_var, d_scale, d_bias, eps, B, C, H, W, kh, kw, sh, sw, ph, pw,
                                (hipStream_t)stream, "sl_batchnorm_infer_relu_maxpool");
}
