// K1 / K2 — activation reduce kernels (HBM-bound).
//
// Replaces the reference's aggregators (component_visualization/aggregators.py:38-244:
// `tensor.clone().flatten(2).amax(-1)` etc. followed by `.cpu()`) and the bf16 cast of
// ActMax.update (activation_caching.py:133).  One pass over the activation, no clone, no
// host round trip; output is the (B,C) candidate matrix the top-k merge consumes.
//
// Roofline: HBM.  Algorithmic bytes per launch = B*C*S*sizeof(act) read (+ B*C*2 written).
//
// Code paths, chosen on the host from the strides and the dtype (reduce_dispatch below), one translation unit each:
//   reduce_row.hip       rows contiguous (NCHW), fp32: the tensor is a flat stream of R = B*C rows of S floats.  G lanes own
//                        one row and read it as 16-byte pieces from the 16-byte-aligned window that covers it (rows such as
//                        7x7 = 196 B are not 16-byte aligned, so head/tail lanes mask by element index); 64/G rows share one
//                        1-KiB wave-load; reduction across the G lanes is DPP.  rowreduce, rowreduce_fast, rowreduce_dma.
//   reduce_row_half.hip  the same for fp16 / bf16: rowreduce_h, rowreduce_dma (the kernel itself: reduce_dma.hpp).
//   reduce_col.hip       reduced axis strided, component axis contiguous (tokens (B,T,F), or channels_last conv): lanes along
//                        F with 16-byte loads, the waves of a workgroup split T and combine through LDS.  colreduce2, colreduce.
//   this file            generic (any strides, any dtype: one lane per output element), the dispatch, the cache policy's process default,
//                        the C entry points, and abs_norm_rows.
// reduce_common.hpp holds what the units share and declares what crosses them.
#include <atomic>
#include <cstdlib>

#include "reduce_common.hpp"

namespace sl {

// ---- process default of the cache policy (reduce_policy.hpp), for calls that pass none: sl_set_reduce_policy, else the
// environment (SL_NT_MIN_BYTES, SL_REDUCE_TAIL_MB in MiB), else 256 MiB / 240 MiB.  A stored -1 = not set by a caller
static std::atomic<int64_t> g_default_nt_min{-1}, g_default_tail{-1};

// a negative field of a call's policy takes the process default
static ReducePolicy resolve_policy(int64_t nt_min_bytes, int64_t tail_bytes) {
  static const ReducePolicy env = [] {  // read once; initialisation of a local static is thread-safe
    const char* n = getenv("SL_NT_MIN_BYTES");
    const char* t = getenv("SL_REDUCE_TAIL_MB");
    return ReducePolicy{n ? (int64_t)atoll(n) : (int64_t)256 << 20, (t ? (int64_t)atoll(t) : (int64_t)240) << 20};
  }();
  if (nt_min_bytes < 0) nt_min_bytes = g_default_nt_min.load(std::memory_order_relaxed);
  if (tail_bytes < 0) tail_bytes = g_default_tail.load(std::memory_order_relaxed);
  return ReducePolicy{nt_min_bytes < 0 ? env.nt_min_bytes : nt_min_bytes, tail_bytes < 0 ? env.tail_bytes : tail_bytes};
}

int bad_reduce_op(const char* who, int op) {
  set_error("reduce: internal error: %s: bad op %d", who, op);
  return SL_E_INVALID;
}

int dma_unreachable(const char* site, int u, int64_t R, int S) {
  set_error("reduce: internal error: rowreduce_dma site (%s) met U = %d, which its guards exclude (R = %lld, S = %d)", site, u,
            (long long)R, S);
  return SL_E_UNSUPPORTED;
}

namespace {

// ---- generic: any strides, fp32 / fp16 / bf16 -------------------------------------------------
template <typename T>
__device__ inline float load_as_f32(const void* p, int64_t i);
template <>
__device__ inline float load_as_f32<float>(const void* p, int64_t i) { return ((const float*)p)[i]; }
template <>
__device__ inline float load_as_f32<_Float16>(const void* p, int64_t i) { return (float)((const _Float16*)p)[i]; }
template <>
__device__ inline float load_as_f32<uint16_t>(const void* p, int64_t i) { return bf16_to_f32(((const uint16_t*)p)[i]); }

template <typename T, int OP>
__global__ __launch_bounds__(256) void generic_reduce_kernel(const void* __restrict__ x, int64_t B, int64_t C,
                                                              int64_t S, int64_t sb, int64_t sc, int64_t ss,
                                                              int64_t s_begin, int64_t s_end, float denom,
                                                              uint16_t* __restrict__ cand, float* __restrict__ outf) {
  const int64_t n = B * C;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / C, c = i % C;
    const int64_t off = b * sb + c * sc;
    Acc<OP> a;
    a.init();
    for (int64_t s = s_begin; s < s_end; ++s) a.add(load_as_f32<T>(x, off + s * ss), true);
    float r = finish<OP>(a.lane_value(), denom);
    r = round_to_dtype<T>(r);
    store_outputs(r, i, cand, outf);
  }
}

template <typename T, int OP>
void launch_generic(const ReduceCall& c, const void* x, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss, int64_t s0,
                    int64_t s1) {
  SL_LAUNCH(c.prof, (generic_reduce_kernel<T, OP>), dim3(grid_blocks((B * C + 255) / 256, 16)), dim3(256), 0, c.st, x, B, C, S, sb, sc,
            ss, s0, s1, c.denom, c.cand, c.outf);
}

int dispatch_generic(int op, const ReduceCall& c, const void* x, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                     int64_t ss, int64_t s0, int64_t s1) {
  if (dtype == SL_F32) {
    SL_SWITCH_OP(op, launch_generic<float, OP>(c, x, B, C, S, sb, sc, ss, s0, s1); return 0);
  } else if (dtype == SL_F16) {
    SL_SWITCH_OP(op, launch_generic<_Float16, OP>(c, x, B, C, S, sb, sc, ss, s0, s1); return 0);
  } else {
    SL_SWITCH_OP(op, launch_generic<uint16_t, OP>(c, x, B, C, S, sb, sc, ss, s0, s1); return 0);
  }
  return bad_reduce_op("dispatch_generic", op);
}

// what the sums over [s0, s1) are divided by.  x / 1 is exact: the same kernels give plain sums
float reduce_denom(int64_t s0, int64_t s1, bool plain_sum) { return plain_sum ? 1.f : (float)(s1 - s0); }

// (B, C, S) with strides -> (B, C): reduce over s in [s0, s1).  Picks the fastest legal path.
int reduce_dispatch(int op, const ReduceCall& c, const void* x, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                    int64_t ss, int64_t s0, int64_t s1) {
  const bool aligned = ((uintptr_t)x & 15) == 0;
  const bool full = (s0 == 0 && s1 == S);
  int rc = 0;
  if (dtype == SL_F32 && aligned && full && ss == 1 && sc == S && sb == C * S && S < (1 << 28)) {
    rc = dispatch_rowreduce(op, c, (const float*)x, B * C, (int)S);
  } else if (dtype == SL_F32 && aligned && sc == 1 && (C % 4) == 0 && (ss % 4) == 0 && (sb % 4) == 0 &&
             S < (1 << 30)) {
    rc = launch_colreduce(op, dtype, c, x, B, (int)S, C, sb, ss, (int)s0, (int)s1);
  } else if (dtype != SL_F32 && aligned && full && ss == 1 && sc == S && sb == C * S && S > 0 && S < (1 << 27)) {
    // fp16 / bf16, NCHW-contiguous rows
    rc = dispatch_rowreduce_h(op, dtype, c, x, B * C, (int)S);
  } else if (dtype != SL_F32 && ((uintptr_t)x & 7) == 0 && sc == 1 && (C % 4) == 0 && (ss % 4) == 0 && (sb % 4) == 0 &&
             S < (1 << 30)) {
    // fp16 / bf16, component axis contiguous (channels_last, tokens): 8-byte loads of four components
    rc = launch_colreduce(op, dtype, c, x, B, (int)S, C, sb, ss, (int)s0, (int)s1);
  } else {
    rc = dispatch_generic(op, c, x, dtype, B, C, S, sb, sc, ss, s0, s1);
  }
  if (rc) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "reduce kernel launch");
  return 0;
}

int dtype_size(int dtype) { return dtype == SL_F32 ? 4 : 2; }

// L same-shape (B, C, S) activations -> (L, B, C) candidates.  ONE launch when the component axis is contiguous (tokens,
// channels_last: colreduce2 over a table of tensors), tensor by tensor otherwise — the same values either way.  Nothing tunes
// these per call: the cache policy is the process default.
int reduce_dispatch_multi(int op, const void* const* xs, int L, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                          int64_t ss, int64_t s0, int64_t s1, uint16_t* cand, hipStream_t st, bool plain_sum = false) {
  const float denom = reduce_denom(s0, s1, plain_sum);
  const ReducePolicy policy = resolve_policy(-1, -1);
  const double work = (double)B * C * (s1 - s0) * dtype_size(dtype);
  for (int l0 = 0; l0 < L; l0 += kMaxReduceSources) {
    const int n = L - l0 < kMaxReduceSources ? L - l0 : kMaxReduceSources;
    uint16_t* out = cand + (int64_t)l0 * B * C;
    bool done = false;
    if (n > 1 && sc == 1 && S < (1 << 30) && (ss % 4) == 0 && (sb % 4) == 0 && (C % 4) == 0) {
      ProfScope prof(SL_PROF_REDUCE, st, work * n);
      const int rc = launch_colreduce2(op, dtype, ReduceCall{prof, st, denom, out, nullptr, policy}, xs + l0, B, n * B, (int)S, C, sb, ss,
                                       (int)s0, (int)s1);
      if (rc < 0) return rc;
      done = rc > 0;
      if (done) {
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return hip_fail(e, "reduce kernel launch");
      }
    }
    if (!done) {
      for (int i = 0; i < n; ++i) {
        ProfScope prof(SL_PROF_REDUCE, st, work);
        const int rc = reduce_dispatch(op, ReduceCall{prof, st, denom, out + (int64_t)i * B * C, nullptr, policy}, xs[l0 + i], dtype, B, C, S,
                                       sb, sc, ss, s0, s1);
        if (rc) return rc;
      }
    }
  }
  return 0;
}

// token aggregator -> op and reduced range [t0, t1) of a (B,T,F) activation, read as (B, C=F, S=T) with sc = sf, ss = st
int token_plan(int agg, int64_t pos, int64_t T, int* op, int64_t* t0, int64_t* t1) {
  *t0 = 0;
  *t1 = T;
  if (agg == SL_TOK_TOKEN) {
    const int64_t p = pos < 0 ? pos + T : pos;
    SL_REQUIRE(p >= 0 && p < T, "sl_reduce_tokens: token position %lld out of range for T=%lld", (long long)pos, (long long)T);
    *t0 = p;
    *t1 = p + 1;
  }
  switch (agg) {
    case SL_TOK_MEAN: *op = OP_SUM; break;
    case SL_TOK_ABSMEAN: *op = OP_ABSSUM; break;
    case SL_TOK_ABSMAX: *op = OP_ABSMAX; break;
    default: *op = OP_MAX; break;  // max, and the single-token pick (max over one element is the element itself)
  }
  return 0;
}

// x (B,C) fp32 in place: x[b][:] /= (sum_c |x[b][c]| + eps)   (crp ChannelConcept.reference_sampling, abs_norm)
__global__ __launch_bounds__(256) void abs_norm_rows_kernel(float* __restrict__ x, int64_t B, int64_t C, float eps) {
  __shared__ float s_part[4];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    float* row = x + b * C;
    float s = 0.f;
    for (int64_t c = threadIdx.x; c < C; c += 256) s += __builtin_fabsf(row[c]);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = s;
    __syncthreads();
    const float tot = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]) + eps;
    for (int64_t c = threadIdx.x; c < C; c += 256) row[c] = row[c] / tot;
  }
}

}  // namespace
}  // namespace sl

using namespace sl;

// ---- C entry points ------------------------------------------------------------------------------------------------------
SL_API int sl_reduce_conv_p(const void* d_act, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss, int agg,
                            uint16_t* d_cand_bf16, float* d_out_f32, void* stream, int64_t nt_min_bytes, int64_t tail_bytes) {
  SL_REQUIRE(d_act || B * C * S == 0, "sl_reduce_conv: null activation");
  SL_REQUIRE(dtype >= SL_F32 && dtype <= SL_BF16, "sl_reduce_conv: bad dtype %d", dtype);
  SL_REQUIRE(B >= 0 && C >= 0 && S >= 0, "sl_reduce_conv: negative shape");
  SL_REQUIRE(agg == SL_CONV_MAX || agg == SL_CONV_MEAN || agg == SL_CONV_SUM, "sl_reduce_conv: bad agg %d", agg);
  SL_REQUIRE(d_cand_bf16 || d_out_f32, "sl_reduce_conv: no output");
  if (B * C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_REDUCE, st, (double)B * C * S * dtype_size(dtype));
  const ReduceCall c{prof, st, reduce_denom(0, S, agg == SL_CONV_SUM), d_cand_bf16, d_out_f32, resolve_policy(nt_min_bytes, tail_bytes)};
  return reduce_dispatch(agg == SL_CONV_MAX ? OP_MAX : OP_SUM, c, d_act, dtype, B, C, S, sb, sc, ss, 0, S);
}

SL_API int sl_reduce_conv(const void* d_act, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                          int64_t ss, int agg, uint16_t* d_cand_bf16, float* d_out_f32, void* stream) {
  return sl_reduce_conv_p(d_act, dtype, B, C, S, sb, sc, ss, agg, d_cand_bf16, d_out_f32, stream, -1, -1);
}

SL_API int sl_reduce_conv_multi(const void* const* h_d_acts, int L, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                                int64_t ss, int agg, uint16_t* d_cand_bf16, void* stream) {
  SL_REQUIRE(L >= 0 && B >= 0 && C >= 0 && S >= 0, "sl_reduce_conv_multi: negative shape");
  SL_REQUIRE(dtype >= SL_F32 && dtype <= SL_BF16, "sl_reduce_conv_multi: bad dtype %d", dtype);
  SL_REQUIRE(agg == SL_CONV_MAX || agg == SL_CONV_MEAN || agg == SL_CONV_SUM, "sl_reduce_conv_multi: bad agg %d", agg);
  if (L == 0 || B * C == 0) return 0;
  SL_REQUIRE(h_d_acts && d_cand_bf16, "sl_reduce_conv_multi: null pointer");
  for (int l = 0; l < L; ++l) SL_REQUIRE(h_d_acts[l] || S == 0, "sl_reduce_conv_multi: null activation");
  return reduce_dispatch_multi(agg == SL_CONV_MAX ? OP_MAX : OP_SUM, h_d_acts, L, dtype, B, C, S, sb, sc, ss, 0, S, d_cand_bf16,
                               (hipStream_t)stream, agg == SL_CONV_SUM);
}

SL_API int sl_reduce_tokens_p(const void* d_act, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st_, int64_t sf, int agg,
                              int64_t pos, uint16_t* d_cand_bf16, float* d_out_f32, void* stream, int64_t nt_min_bytes,
                              int64_t tail_bytes) {
  SL_REQUIRE(d_act || B * T * F == 0, "sl_reduce_tokens: null activation");
  SL_REQUIRE(dtype >= SL_F32 && dtype <= SL_BF16, "sl_reduce_tokens: bad dtype %d", dtype);
  SL_REQUIRE(B >= 0 && T >= 0 && F >= 0, "sl_reduce_tokens: negative shape");
  SL_REQUIRE(agg >= SL_TOK_MEAN && agg <= SL_TOK_TOKEN, "sl_reduce_tokens: bad agg %d", agg);
  SL_REQUIRE(d_cand_bf16 || d_out_f32, "sl_reduce_tokens: no output");
  if (B * F == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  int op;
  int64_t t0, t1;
  if (const int rc = token_plan(agg, pos, T, &op, &t0, &t1)) return rc;
  ProfScope prof(SL_PROF_REDUCE, st, (double)B * (t1 - t0) * F * dtype_size(dtype));
  const ReduceCall c{prof, st, reduce_denom(t0, t1, false), d_cand_bf16, d_out_f32, resolve_policy(nt_min_bytes, tail_bytes)};
  return reduce_dispatch(op, c, d_act, dtype, B, F, T, sb, sf, st_, t0, t1);
}

SL_API int sl_reduce_tokens(const void* d_act, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st_,
                            int64_t sf, int agg, int64_t pos, uint16_t* d_cand_bf16, float* d_out_f32,
                            void* stream) {
  return sl_reduce_tokens_p(d_act, dtype, B, T, F, sb, st_, sf, agg, pos, d_cand_bf16, d_out_f32, stream, -1, -1);
}

SL_API int sl_reduce_tokens_multi(const void* const* h_d_acts, int L, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st_,
                                  int64_t sf, int agg, int64_t pos, uint16_t* d_cand_bf16, void* stream) {
  SL_REQUIRE(L >= 0 && B >= 0 && T >= 0 && F >= 0, "sl_reduce_tokens_multi: negative shape");
  SL_REQUIRE(dtype >= SL_F32 && dtype <= SL_BF16, "sl_reduce_tokens_multi: bad dtype %d", dtype);
  SL_REQUIRE(agg >= SL_TOK_MEAN && agg <= SL_TOK_TOKEN, "sl_reduce_tokens_multi: bad agg %d", agg);
  if (L == 0 || B * F == 0) return 0;
  SL_REQUIRE(h_d_acts && d_cand_bf16, "sl_reduce_tokens_multi: null pointer");
  for (int l = 0; l < L; ++l) SL_REQUIRE(h_d_acts[l] || T == 0, "sl_reduce_tokens_multi: null activation");
  int op;
  int64_t t0, t1;
  if (const int rc = token_plan(agg, pos, T, &op, &t0, &t1)) return rc;
  return reduce_dispatch_multi(op, h_d_acts, L, dtype, B, F, T, sb, sf, st_, t0, t1, d_cand_bf16, (hipStream_t)stream);
}

SL_API int sl_set_reduce_policy(int64_t nt_min_bytes, int64_t tail_bytes) {
  // negative = back to the environment / built-in defaults
  g_default_nt_min.store(nt_min_bytes < 0 ? -1 : nt_min_bytes, std::memory_order_relaxed);
  g_default_tail.store(tail_bytes < 0 ? -1 : tail_bytes, std::memory_order_relaxed);
  return 0;
}

SL_API int sl_abs_norm_rows(float* d_x, int64_t B, int64_t C, float eps, void* stream) {
  SL_REQUIRE(B >= 0 && C >= 0, "sl_abs_norm_rows: negative shape");
  if (B * C == 0) return 0;
  SL_REQUIRE(d_x, "sl_abs_norm_rows: null pointer");
  hipLaunchKernelGGL(abs_norm_rows_kernel, dim3(grid_blocks(B, 8)), dim3(256), 0, (hipStream_t)stream, d_x, B, C, eps);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
