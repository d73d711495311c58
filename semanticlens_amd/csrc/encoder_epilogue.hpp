// K11 — the epilogue of the towers' linear layers, shared by the two GEMM units (encoder_linear.hip: fp32-input MFMA,
// encoder_linear3.hip: split-bf16 x3): out = act(x W^T + b) (+ residual), optional row scatter for the patch embedding.
// Everything sits in an anonymous namespace: the kernels' names carry `LinearEpi`'s, and stay what they were in one unit.
#pragma once
#include <type_traits>

#include "gemm_bf16x3.hpp"

namespace sl {
namespace {

using gemm3::split_kp;
using gemm3::store_split;   // (v, row, col, Kp, split matrix): see gemm_bf16x3.hpp for the layout

// erf for the GELU epilogue: Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7) with the hardware exp2 and reciprocal —
// 15 instructions instead of libm erff's ~50.  The epilogue of a 256 x 256 tile evaluates it 128 times per lane, which
// with erff cost 25 K cycles per tile next to a k loop of 52-78 K (K = 512 / 768): fc1 ran 29 % slower per tile than the
// plain GEMM.  max |gelu - exact| over [-8, 8] stays 4.7e-7, the same as with a correctly rounded fp32 erf (the final
// products round at that level).
// Every multiply-add below is written as an explicit fma and contraction is off: left to the compiler, which mul + add pairs
// fuse depends on how the surrounding (unrolled) epilogue code was vectorised, so the SAME value came out 1 ulp apart
// depending on the row's position inside the 256-row tile — and an embedding depended on where its sample sat in the batch
// (found when a batch was cut in two: rows 4800.. of a 9600-row GEMM vs rows 0.. of a 4800-row one).
__device__ inline float erf_as(float z) {
#pragma clang fp contract(off)
  const float a = __builtin_fabsf(z);
  const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(0.3275911f, a, 1.f));
  float p = __builtin_fmaf(t, 1.061405429f, -1.453152027f);
  p = __builtin_fmaf(t, p, 1.421413741f);
  p = __builtin_fmaf(t, p, -0.284496736f);
  p = __builtin_fmaf(t, p, 0.254829592f);
  const float poly = t * p;
  return __builtin_copysignf(__builtin_fmaf(-poly, __expf(-(a * a)), 1.f), z);
}

template <int ACT, bool RES, bool REMAP, bool SPLIT = false>
struct LinearEpi {
  const float* bias;  // (N) or nullptr
  const float* res;   // (M, ldo) or nullptr; may alias out (same element read then written by one lane)
  float* out;
  uint16_t* out_sp;   // SPLIT: the result goes out as a split matrix (M x N, gemm_bf16x3.hpp) instead of fp32
  int64_t out_kp;     // its padded row length split_kp(N)
  int64_t ldo;
  int64_t rpg, gstride, roff;  // REMAP: out row = (r / rpg) * gstride + roff + r % rpg
  const float* rowadd;         // REMAP: (roff + r % rpg, col) of this (T, N) table is added (positional embedding)
  int64_t N;
  uint32_t rpg_inv;            // REMAP: floor(2^32 / rpg) (2^32 - 1 for rpg = 1), for row / rpg without a division
  // row -> (row / rpg, row % rpg), rows and rpg below 2^32: the high product underestimates the quotient by at most one
  __device__ inline void divmod_rpg(int64_t row, uint32_t& q, uint32_t& rem) const {
    const uint32_t r = (uint32_t)row, g = (uint32_t)rpg;
    q = __umulhi(r, rpg_inv);
    rem = r - q * g;
    if (rem >= g) { q += 1; rem -= g; }
    if (rem >= g) { q += 1; rem -= g; }
  }
  __device__ inline float column(int64_t col) const { return bias ? bias[col] : 0.f; }
  // the same epilogue for a GEMM over columns [c0, ...) of the output (c0 a multiple of 32; gemm_bf16x3.hpp: column-strip split)
  LinearEpi shifted(int64_t c0) const {
    LinearEpi e = *this;
    if (e.bias) e.bias += c0;
    if (e.res) e.res += c0;
    if (e.out) e.out += c0;
    if (e.out_sp) e.out_sp += (c0 >> 5) * 64;  // split_pos: 64 elements per 32-column tile of a row
    if (e.rowadd) e.rowadd += c0;
    return e;
  }
  // what `store` adds from memory, fetched ahead of the stores by kernels that batch their epilogue (gemm_8phase.hpp);
  // `store_fetched(..., fetch(row, col))` == `store(...)` bit for bit (same operands, same order of additions)
  static constexpr bool kFetches = RES || REMAP;
  __device__ inline int64_t out_row(int64_t row) const {
    if constexpr (REMAP) {
      // (two 64-bit divisions per element cost the patch-embedding GEMM 10 us of 176)
      uint32_t q, rem;
      divmod_rpg(row, q, rem);
      return (int64_t)q * gstride + roff + (int64_t)rem;
    }
    return row;
  }
  __device__ inline float2 fetch(int64_t row, int64_t col) const {  // (positional-table value, residual value)
    float2 f = make_float2(0.f, 0.f);
    if constexpr (REMAP) {
      if (rowadd) {
        uint32_t q, rem;
        divmod_rpg(row, q, rem);
        f.x = rowadd[(roff + (int64_t)rem) * N + col];
      }
    }
    if constexpr (RES) f.y = res[out_row(row) * ldo + col];
    return f;
  }
  __device__ inline void store_fetched(int64_t row, int64_t col, float acc, float b, float2 f) const {
#pragma clang fp contract(off)  // see erf_as: one rounding sequence per element, whatever code surrounds it
    float v = acc + b;
    if constexpr (ACT == SL_ACT_GELU) {
      const float hv = 0.5f * v;
      v = __builtin_fmaf(hv, erf_as(v * 0.70710678118654752440f), hv);  // 0.5 v (1 + erf(v / sqrt 2))
    }
    if constexpr (ACT == SL_ACT_QUICKGELU) v = v * __builtin_amdgcn_rcpf(1.f + __expf(-1.702f * v));
    if constexpr (ACT == SL_ACT_GELU_TANH) {  // torch gelu(approximate="tanh"): SigLIP's "gelu_pytorch_tanh"
      const float u = 0.79788456080286535588f * __builtin_fmaf(0.044715f * v, v * v, v);
      // 0.5 v (1 + tanh u) = v - v / (1 + exp(2 u)); exp overflow -> v, underflow -> 0.  The overflow case is a select, not
      // v - v * 0: the same bits for every finite v, and +inf stays +inf as in torch (inf * 0 made it NaN)
      const float r = __builtin_amdgcn_rcpf(1.f + __expf(2.f * u));
      v = r == 0.f ? v : __builtin_fmaf(-v, r, v);
    }
    const int64_t orow = out_row(row);
    if constexpr (REMAP) {
      if (rowadd) v += f.x;
    }
    if constexpr (RES) v += f.y;
    if constexpr (SPLIT) store_split(v, orow, col, out_kp, out_sp);
    else out[orow * ldo + col] = v;
  }
  __device__ inline void store(int64_t row, int64_t col, float acc, float b) const { store_fetched(row, col, acc, b, fetch(row, col)); }
};

// `act` as a compile-time constant: f(std::integral_constant<int, SL_ACT_*>), for both linear entry points (which have
// checked the range)
template <class F>
int with_act(int act, F&& f) {
  if (act == SL_ACT_NONE) return f(std::integral_constant<int, SL_ACT_NONE>{});
  if (act == SL_ACT_GELU) return f(std::integral_constant<int, SL_ACT_GELU>{});
  if (act == SL_ACT_GELU_TANH) return f(std::integral_constant<int, SL_ACT_GELU_TANH>{});
  return f(std::integral_constant<int, SL_ACT_QUICKGELU>{});
}

}  // namespace
}  // namespace sl
