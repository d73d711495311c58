// The inference BatchNorm value and the epilogues that follow it, operation by operation as MIOpen and ATen compute them
// (DESIGN.md §K16, §K19).  Shared by batchnorm.hip and conv_tail.hip; both units are compiled with -ffp-contract=off, which
// these forms need: the compiler may neither fuse the subtract/multiply nor split the multiply-add.
#pragma once
#include "common.hpp"

namespace sl {

enum { EPI_PLAIN = 0, EPI_RELU = 1, EPI_ADD_RELU = 2, EPI_ADD_BN_RELU = 3 };

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

// a + b as ATen's add kernel computes it.  Only two NaN operands tell the forms apart: the hardware returns one operand's payload,
// which one depends on the instruction and on the operand's position, and the compiler is free to commute an add or to pair
// two of them into a packed one (it did: v_pk_add_f32 kept the other payload in every such element, whichever tensor was the
// left operand).  So the instruction is written out, with the right-hand operand first: the form that matched on the device.
__device__ inline float add_as_aten(float a, float b) {
  float r;
  asm("v_add_f32_e32 %0, %1, %2" : "=v"(r) : "v"(b), "v"(a));
  return r;
}

// One BatchNorm2d's per-channel tensors, as the module holds them.
struct BnParams {
  const float *mean, *var, *scale, *bias;
  double eps;
};

__device__ inline f4 bn_constants(const BnParams& p, uint32_t c) {
  return f4{p.mean[c], bn_inv_std(p.var[c], p.eps), p.scale[c], p.bias[c]};
}

// r is the residual (EPI_ADD_RELU) or the second tensor's element, kb its constants (EPI_ADD_BN_RELU)
template <int EPI>
__device__ inline float bn_finish(float x, const f4 k, float r, const f4 kb) {
  float y = bn_value(x, k);
  if constexpr (EPI == EPI_ADD_RELU) y = y + r;  // y is an fp32 value here, as when it went through memory
  if constexpr (EPI == EPI_ADD_BN_RELU) y = add_as_aten(y, bn_value(r, kb));  // two fp32 values; x's is the left operand, as in the model
  if constexpr (EPI != EPI_PLAIN) y = relu_clamp(y);
  return y;
}

}  // namespace sl
