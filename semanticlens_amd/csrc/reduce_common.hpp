// K1 / K2 — what the units of the activation reduce share: reduce.hip (dispatch, ABI, generic kernel), reduce_row.hip (fp32
// rows), reduce_row_half.hip (fp16 / bf16 rows) and reduce_col.hip (component axis contiguous).  Device helpers and the host
// grid helper sit in an unnamed namespace (every unit gets its own copy, the kernels keep their names); the functions that
// cross units are declared at the end.
#pragma once
#include <cstdint>
#include <type_traits>

#include "common.hpp"
#include "reduce_policy.hpp"

namespace sl {
namespace {

enum Op : int { OP_MAX = 0, OP_SUM = 1, OP_ABSMAX = 2, OP_ABSSUM = 3 };

// op as a compile-time constant `OP` inside the statement: the switch from a dispatcher's runtime `op` to its template.
// The statement returns; a dispatcher that gets past the switch was handed a bad op and returns bad_reduce_op()
#define SL_SWITCH_OP(op, ...)                                   \
  switch (op) {                                                 \
    case OP_MAX: { constexpr int OP = OP_MAX; __VA_ARGS__; } break;       \
    case OP_SUM: { constexpr int OP = OP_SUM; __VA_ARGS__; } break;       \
    case OP_ABSMAX: { constexpr int OP = OP_ABSMAX; __VA_ARGS__; } break; \
    case OP_ABSSUM: { constexpr int OP = OP_ABSSUM; __VA_ARGS__; } break; \
    default: break;                                             \
  }

// ---- cross-lane helpers ------------------------------------------------------------------
template <int CTRL>
__device__ inline int dpp_i32(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false);
}
// float -> int whose signed order equals the float order with +NaN on top
__device__ inline int f32_sort_key(float f) {
  int b = (int)f32_bits(f);
  return b ^ ((b >> 31) & 0x7FFFFFFF);
}
__device__ inline float sort_key_f32(int k) { return bits_f32((uint32_t)(k ^ ((k >> 31) & 0x7FFFFFFF))); }

template <bool SUM>
__device__ inline float combine(float a, float b) {
  if constexpr (SUM) return a + b;
  return sort_key_f32(max(f32_sort_key(a), f32_sort_key(b)));  // NaN-propagating max
}

// per-lane accumulator: running max ignores NaN (v_max_f32) and remembers it separately
template <int OP>
struct Acc {
  float v;
  bool nan;
  __device__ inline void init() {
    v = (OP == OP_SUM || OP == OP_ABSSUM) ? 0.f : -__builtin_huge_valf();
    nan = false;
  }
  __device__ inline void add(float x, bool valid) {
    if constexpr (OP == OP_ABSMAX || OP == OP_ABSSUM) x = __builtin_fabsf(x);
    if constexpr (OP == OP_SUM || OP == OP_ABSSUM) {
      v += valid ? x : 0.f;
    } else {
      x = valid ? x : -__builtin_huge_valf();
      nan |= (x != x);
      v = __builtin_fmaxf(v, x);
    }
  }
  __device__ inline float lane_value() const {
    if constexpr (OP == OP_SUM || OP == OP_ABSSUM) return v;
    return nan ? bits_f32(0x7FC00000u) : v;
  }
};

template <int OP>
__device__ inline float finish(float v, float count) {
  if constexpr (OP == OP_SUM || OP == OP_ABSSUM) return v / count;  // torch: sum / n
  return v;
}

__device__ inline void store_outputs(float r, int64_t idx, uint16_t* cand, float* outf) {
  if (outf) outf[idx] = r;
  if (cand) cand[idx] = f32_to_bf16_rne(r);
}

// ---- all-reduce over aligned groups of G lanes: three forms, used in different places on purpose ------------------------
//   group_allreduce_f      plain builtins; the round-1 kernels, rowreduce_h and every rare path (the NaN re-scan)
//   group_allreduce_asm    one DPP instruction per level; rowreduce_fast's per-row reduction
//   group_allreduce_bcast  the same within 16 lanes, then row broadcasts + v_readlane; rowreduce_dma (G = 32 / 64 without the
//                          ds_bpermute round trips)
template <bool SUMOP>
__device__ inline float dpp_combine(float v, float o) {
  if constexpr (SUMOP) return v + o;
  return __builtin_fmaxf(v, o);
}
template <int CTRL, bool SUMOP>
__device__ inline float dpp_step(float v) {
  return dpp_combine<SUMOP>(v, bits_f32((uint32_t)dpp_i32<CTRL>((int)f32_bits(v))));
}
// all-reduce (plain float max / add) over aligned groups of G lanes
template <int G, bool SUMOP>
__device__ inline float group_allreduce_f(float v) {
  if constexpr (G >= 2) v = dpp_step<0xB1, SUMOP>(v);
  if constexpr (G >= 4) v = dpp_step<0x4E, SUMOP>(v);
  if constexpr (G >= 8) v = dpp_step<0x141, SUMOP>(v);
  if constexpr (G >= 16) v = dpp_step<0x140, SUMOP>(v);
  if constexpr (G >= 32) v = dpp_combine<SUMOP>(v, __shfl_xor(v, 16, 64));
  if constexpr (G >= 64) v = dpp_combine<SUMOP>(v, __shfl_xor(v, 32, 64));
  return v;
}

// hipcc's own fmaxf lowering (canonicalising v_max pairs, unfused DPP moves) cost ~3x the VALU work of these and capped
// rowreduce_fast near 3.6 TB/s, hence the few single-instruction asm helpers below.
__device__ inline float v_max3(float a, float b, float c) {
  float r;
  asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ inline float v_max2(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// r = op(a, dpp(a)); the s_nop covers the VALU-write -> DPP-read hazard (2 wait states), which the
// compiler does not pad inside an asm statement.
#define SL_DPP_OP(name, insn, ctrl)                                                           \
  __device__ inline float name(float a) {                                                     \
    float r;                                                                                  \
    asm("s_nop 1\n\t" insn " %0, %1, %1 " ctrl " row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(a)); \
    return r;                                                                                 \
  }
SL_DPP_OP(max_qp1, "v_max_f32_dpp", "quad_perm:[1,0,3,2]")
SL_DPP_OP(max_qp2, "v_max_f32_dpp", "quad_perm:[2,3,0,1]")
SL_DPP_OP(max_hmir, "v_max_f32_dpp", "row_half_mirror")
SL_DPP_OP(max_mir, "v_max_f32_dpp", "row_mirror")
SL_DPP_OP(add_qp1, "v_add_f32_dpp", "quad_perm:[1,0,3,2]")
SL_DPP_OP(add_qp2, "v_add_f32_dpp", "quad_perm:[2,3,0,1]")
SL_DPP_OP(add_hmir, "v_add_f32_dpp", "row_half_mirror")
SL_DPP_OP(add_mir, "v_add_f32_dpp", "row_mirror")
#undef SL_DPP_OP

template <int G, bool SUMOP>
__device__ inline float group_allreduce_asm(float v) {
  if constexpr (SUMOP) {
    if constexpr (G >= 2) v = add_qp1(v);
    if constexpr (G >= 4) v = add_qp2(v);
    if constexpr (G >= 8) v = add_hmir(v);
    if constexpr (G >= 16) v = add_mir(v);
    if constexpr (G >= 32) v += __shfl_xor(v, 16, 64);
    if constexpr (G >= 64) v += __shfl_xor(v, 32, 64);
  } else {
    if constexpr (G >= 2) v = max_qp1(v);
    if constexpr (G >= 4) v = max_qp2(v);
    if constexpr (G >= 8) v = max_hmir(v);
    if constexpr (G >= 16) v = max_mir(v);
    if constexpr (G >= 32) v = v_max2(v, __shfl_xor(v, 16, 64));
    if constexpr (G >= 64) v = v_max2(v, __shfl_xor(v, 32, 64));
  }
  return v;
}

// Row-broadcast steps of a wave64 reduction (gfx9 DPP): row_bcast:15 folds the last lane of rows 0 / 2 into rows 1 / 3,
// row_bcast:31 folds lane 31 into rows 2 and 3.  In-place (rows that are masked out keep their value).  After the
// within-16 all-reduce plus these, lane 31 (G = 32: and lane 63) / lane 63 (G = 64) holds the group's result — without
// the two ds_bpermute round trips (~200 dependent cycles per row) that __shfl_xor costs.
#define SL_DPP_BCAST(name, insn, ctrl, mask)                                                              \
  __device__ inline float name(float a) {                                                                 \
    asm("s_nop 1\n\t" insn " %0, %0, %0 " ctrl " row_mask:" mask " bank_mask:0xf" : "+v"(a));            \
    return a;                                                                                             \
  }
SL_DPP_BCAST(max_bc15, "v_max_f32_dpp", "row_bcast:15", "0xa")
SL_DPP_BCAST(max_bc31, "v_max_f32_dpp", "row_bcast:31", "0xc")
SL_DPP_BCAST(add_bc15, "v_add_f32_dpp", "row_bcast:15", "0xa")
SL_DPP_BCAST(add_bc31, "v_add_f32_dpp", "row_bcast:31", "0xc")
#undef SL_DPP_BCAST

// all-reduce over aligned groups of G lanes whose result every lane of the group needs: DPP within 16 lanes, then for
// G = 32 / 64 row broadcasts + v_readlane (the value comes back wave-uniform per group)
template <int G, bool SUMOP>
__device__ inline float group_allreduce_bcast(float v, int lane) {
  if constexpr (G <= 16) return group_allreduce_asm<G, SUMOP>(v);
  v = group_allreduce_asm<16, SUMOP>(v);
  v = SUMOP ? add_bc15(v) : max_bc15(v);
  if constexpr (G == 64) {
    v = SUMOP ? add_bc31(v) : max_bc31(v);
    return bits_f32((uint32_t)__builtin_amdgcn_readlane((int)f32_bits(v), 63));
  } else {
    const float lo = bits_f32((uint32_t)__builtin_amdgcn_readlane((int)f32_bits(v), 31));
    const float hi = bits_f32((uint32_t)__builtin_amdgcn_readlane((int)f32_bits(v), 63));
    return lane < 32 ? lo : hi;
  }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
// cache-policy bits of the streaming loads: 2 = nt (read-once stream; +4..10 % over 0, A/B measured)
constexpr int kLoadAux = 2;

// streaming (read-once) 16-byte load with the nt cache policy, like the buffer loads of rowreduce_fast
__device__ inline float4 nt_load4(const float* p) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}

// ---- 2-byte activations (fp16 / bf16 models): element tags are _Float16 and uint16_t (bf16 bits) ---------------------
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
template <typename T>
__device__ inline void unpack2(uint32_t w, float& lo, float& hi);
template <>
__device__ inline void unpack2<uint16_t>(uint32_t w, float& lo, float& hi) {
  lo = bits_f32(w << 16);
  hi = bits_f32(w & 0xFFFF0000u);
}
template <>
__device__ inline void unpack2<_Float16>(uint32_t w, float& lo, float& hi) {
  const f16x2 h = __builtin_bit_cast(f16x2, w);
  lo = (float)h[0];
  hi = (float)h[1];
}
template <typename T>
__device__ inline float elem_as_f32(T v) {
  if constexpr (sizeof(T) == 4) {
    return v;
  } else {
    float lo, hi;
    unpack2<T>((uint32_t)__builtin_bit_cast(uint16_t, v), lo, hi);
    return lo;
  }
}
// four consecutive elements as floats: one 16-byte (fp32) or 8-byte (fp16 / bf16) load, streaming policy or default
template <typename T, bool NT>
__device__ inline float4 load4_as_f32(const T* p) {
  if constexpr (sizeof(T) == 4) {
    if constexpr (NT) return nt_load4(reinterpret_cast<const float*>(p));
    else return *reinterpret_cast<const float4*>(p);
  } else {
    u32x2 w;
    if constexpr (NT) w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
    else w = *reinterpret_cast<const u32x2*>(p);
    float4 r;
    unpack2<T>(w[0], r.x, r.y);
    unpack2<T>(w[1], r.z, r.w);
    return r;
  }
}
// round to the activation dtype first (the reference aggregates in that dtype), then report
template <typename T>
__device__ inline float round_to_dtype(float v) { return v; }
template <>
__device__ inline float round_to_dtype<_Float16>(float v) { return (float)(_Float16)v; }
template <>
__device__ inline float round_to_dtype<uint16_t>(float v) { return bf16_to_f32(f32_to_bf16_rne(v)); }

// one 16-byte piece -> its EPP elements as floats (4 fp32, or 8 fp16 / bf16), |.| applied when ABS
template <typename T, bool ABS>
__device__ inline void decode_piece(const u32x4& v, float (&e)[16 / (int)sizeof(T)]) {
  constexpr int EPP = 16 / (int)sizeof(T);
  if constexpr (EPP == 4) {
#pragma unroll
    for (int i = 0; i < 4; ++i) e[i] = bits_f32(v[i]);
  } else {
#pragma unroll
    for (int d = 0; d < 4; ++d) unpack2<T>(v[d], e[2 * d], e[2 * d + 1]);
  }
  if constexpr (ABS) {
#pragma unroll
    for (int i = 0; i < EPP; ++i) e[i] = __builtin_fabsf(e[i]);
  }
}

// The exact half of the row kernels' NaN handling.  v_max_f32 drops NaN and torch.amax propagates it, so a running sum rides
// along with every max (NaN in => NaN out); when some row's all-reduced sum `sred` is NaN (a NaN, or +inf and -inf together)
// the whole wave calls this: G lanes re-scan their row (`row` of x, S elements) if it is a suspect (`row_ok`: the row
// exists), and every lane of a group learns whether its row really holds a NaN.
template <typename T, int G>
__device__ inline bool row_has_nan(float sred, bool row_ok, const T* x, int64_t row, int li, int S) {
  bool nan = false;
  if (row_ok && sred != sred) {
    const T* rowp = x + row * (int64_t)S;
    for (int i = li; i < S; i += G) {
      const float ev = elem_as_f32<T>(rowp[i]);
      nan |= (ev != ev);
    }
  }
  return group_allreduce_f<G, false>(nan ? 1.f : 0.f) > 0.f;
}

// colreduce2 reads a TABLE of up to kMaxReduceSources same-shape tensors (see the kernel's header in reduce_col.hip)
constexpr int kMaxReduceSources = 32;
struct MultiSrc {
  const void* ptr[kMaxReduceSources];
  int64_t per;  // batches per tensor
};

// grid size: `want` workgroups, at least one, at most `per_cu` per compute unit (the kernels loop over what is left)
inline unsigned grid_blocks(int64_t want, int per_cu) {
  const int64_t cap = (int64_t)num_cus() * per_cu;
  return (unsigned)(want > cap ? cap : (want < 1 ? 1 : want));
}

}  // namespace

// ---- what every launch function receives -----------------------------------------------------------------------------------
struct ReduceCall {
  ProfScope& prof;
  hipStream_t st;
  float denom;          // sums are divided by it (1: plain sum); the max family ignores it
  uint16_t* cand;       // (B, C) bf16 and / or
  float* outf;          // (B, C) fp32 outputs
  ReducePolicy policy;  // resolved cache policy (reduce_policy.hpp)
};

// ---- the units' dispatchers: `op` is an Op, `dtype` SL_F32 / SL_F16 / SL_BF16; 0 or a negative SL_E_* (message set) ---------
// a U the site's derivation excludes turned up: never pick another kernel silently
int dma_unreachable(const char* site, int u, int64_t R, int S);
// SL_SWITCH_OP fell through: `op` is no Op.  Every dispatcher ends with this instead of launching nothing
int bad_reduce_op(const char* who, int op);
// reduce_row.hip: R contiguous rows of S floats, x 16-byte aligned
int dispatch_rowreduce(int op, const ReduceCall& c, const float* x, int64_t R, int S);
// reduce_row_half.hip: the same for 2-byte elements (dtype SL_F16 / SL_BF16)
int dispatch_rowreduce_h(int op, int dtype, const ReduceCall& c, const void* x, int64_t R, int S);
// reduce_col.hip: out[b][f] = op over t in [t0, t1) of x[b][t][f], f contiguous.  launch_colreduce2 takes a table of
// B / per tensors of `per` batches each and returns 1 = launched, 0 = 16-byte pieces are not legal for the input (nothing
// launched), negative = error
int launch_colreduce2(int op, int dtype, const ReduceCall& c, const void* const* srcs, int64_t per, int64_t B, int T, int64_t F,
                      int64_t sb, int64_t st_, int t0, int t1);
int launch_colreduce(int op, int dtype, const ReduceCall& c, const void* x, int64_t B, int T, int64_t F, int64_t sb, int64_t st_,
                     int t0, int t1);

}  // namespace sl
