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
//   this file            generic (any strides, any dtype: one lane per output element), the dispatch, the cache-policy state,
//                        the C entry points, and abs_norm_rows.
// reduce_common.hpp holds what the units share and declares what crosses them.
#include <cstdlib>

#include "reduce_common.hpp"

namespace sl {

// ---- cache policy of the reduce streams (sl_set_reduce_policy; environment SL_NT_MIN_BYTES / SL_REDUCE_TAIL_MB) ----
// A COLD input streams best with the nt (read-once) policy: 6.4 vs 5.9 TB/s on 411 MB.  Inside a model the input was
// written by the previous kernel microseconds ago; what still sits (dirty) in the 256 MiB Infinity Cache reads faster
// with the default policy and nt on it LOSES (in-bench average 5.0 TB/s all-nt vs 5.9 mixed).  The kernel cannot know
// its producer, so the default assumes the common case — a forward hook on the layer that just ran: inputs below
// `nt_min_bytes` (default 256 MiB) are read with the default policy; of larger ones the last `tail_bytes` (default
// 240 MiB: what the cache still holds) likewise and the head with nt.  tail_bytes = 0 and nt_min_bytes = 0 = all nt,
// the right setting for inputs known to be cold.  The kernels walk the tail FIRST — the most recently written bytes are
// read while the cache still holds them (in-pipeline 411 MB: 6.07 -> 6.44 TB/s) — and inputs read entirely with the default
// policy front to back.
static int64_t g_nt_min_bytes = -1, g_tail_bytes = -1;
static int64_t nt_min_bytes_() {
  if (g_nt_min_bytes < 0) {
    const char* e = getenv("SL_NT_MIN_BYTES");
    g_nt_min_bytes = e ? (int64_t)atoll(e) : (int64_t)256 << 20;
  }
  return g_nt_min_bytes;
}
static int64_t tail_bytes_() {
  if (g_tail_bytes < 0) {
    const char* e = getenv("SL_REDUCE_TAIL_MB");
    g_tail_bytes = (e ? (int64_t)atoll(e) : (int64_t)240) << 20;
  }
  return g_tail_bytes;
}

bool nt_policy_applies(int64_t bytes) { return bytes >= nt_min_bytes_(); }

int64_t nt_head_units(int64_t bytes, int64_t unit_bytes, int64_t scale, int64_t tail_cap) {
  if (!nt_policy_applies(bytes)) return 0;
  const int64_t tail = tail_bytes_() < tail_cap ? tail_bytes_() : tail_cap;
  if (tail <= 0) return INT64_MAX;
  return bytes > tail ? (bytes - tail) / unit_bytes * scale : 0;
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
void launch_generic(ProfScope& prof, const void* x, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss, int64_t s0,
                    int64_t s1, float denom, uint16_t* cand, float* outf, hipStream_t st) {
  SL_LAUNCH(prof, (generic_reduce_kernel<T, OP>), dim3(grid_blocks((B * C + 255) / 256, 16)), dim3(256), 0, st, x, B, C, S, sb, sc, ss,
            s0, s1, denom, cand, outf);
}

int dispatch_generic(int op, ProfScope& prof, const void* x, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                     int64_t ss, int64_t s0, int64_t s1, float denom, uint16_t* cand, float* outf, hipStream_t st) {
  if (dtype == SL_F32) {
    SL_SWITCH_OP(op, launch_generic<float, OP>(prof, x, B, C, S, sb, sc, ss, s0, s1, denom, cand, outf, st); return 0);
  } else if (dtype == SL_F16) {
    SL_SWITCH_OP(op, launch_generic<_Float16, OP>(prof, x, B, C, S, sb, sc, ss, s0, s1, denom, cand, outf, st); return 0);
  } else {
    SL_SWITCH_OP(op, launch_generic<uint16_t, OP>(prof, x, B, C, S, sb, sc, ss, s0, s1, denom, cand, outf, st); return 0);
  }
  return bad_reduce_op("dispatch_generic", op);
}

// (B, C, S) with strides -> (B, C): reduce over s in [s0, s1).  Picks the fastest legal path.
int reduce_dispatch(int op, ProfScope& prof, const void* x, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                    int64_t ss, int64_t s0, int64_t s1, uint16_t* cand, float* outf, hipStream_t st, bool plain_sum = false) {
  const float denom = plain_sum ? 1.f : (float)(s1 - s0);  // x / 1 is exact: the same kernels give sums
  const bool aligned = ((uintptr_t)x & 15) == 0;
  const bool full = (s0 == 0 && s1 == S);
  int rc = 0;
  if (dtype == SL_F32 && aligned && full && ss == 1 && sc == S && sb == C * S && S < (1 << 28)) {
    rc = dispatch_rowreduce(op, prof, (const float*)x, B * C, (int)S, denom, cand, outf, st);
  } else if (dtype == SL_F32 && aligned && sc == 1 && (C % 4) == 0 && (ss % 4) == 0 && (sb % 4) == 0 &&
             S < (1 << 30)) {
    rc = launch_colreduce(op, dtype, prof, x, B, (int)S, C, sb, ss, (int)s0, (int)s1, denom, cand, outf, st);
  } else if (dtype != SL_F32 && aligned && full && ss == 1 && sc == S && sb == C * S && S > 0 && S < (1 << 27)) {
    // fp16 / bf16, NCHW-contiguous rows
    rc = dispatch_rowreduce_h(op, dtype, prof, x, B * C, (int)S, denom, cand, outf, st);
  } else if (dtype != SL_F32 && ((uintptr_t)x & 7) == 0 && sc == 1 && (C % 4) == 0 && (ss % 4) == 0 && (sb % 4) == 0 &&
             S < (1 << 30)) {
    // fp16 / bf16, component axis contiguous (channels_last, tokens): 8-byte loads of four components
    rc = launch_colreduce(op, dtype, prof, x, B, (int)S, C, sb, ss, (int)s0, (int)s1, denom, cand, outf, st);
  } else {
    rc = dispatch_generic(op, prof, x, dtype, B, C, S, sb, sc, ss, s0, s1, denom, cand, outf, st);
  }
  if (rc) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(e, "reduce kernel launch");
  return 0;
}

int dtype_size(int dtype) { return dtype == SL_F32 ? 4 : 2; }

// L same-shape (B, C, S) activations -> (L, B, C) candidates.  ONE launch when the component axis is contiguous (tokens,
// channels_last: colreduce2 over a table of tensors), tensor by tensor otherwise — the same values either way.
int reduce_dispatch_multi(int op, const void* const* xs, int L, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                          int64_t ss, int64_t s0, int64_t s1, uint16_t* cand, hipStream_t st, bool plain_sum = false) {
  const float denom = plain_sum ? 1.f : (float)(s1 - s0);
  const double work = (double)B * C * (s1 - s0) * dtype_size(dtype);
  for (int l0 = 0; l0 < L; l0 += kMaxReduceSources) {
    const int n = L - l0 < kMaxReduceSources ? L - l0 : kMaxReduceSources;
    uint16_t* out = cand + (int64_t)l0 * B * C;
    bool done = false;
    if (n > 1 && sc == 1 && S < (1 << 30) && (ss % 4) == 0 && (sb % 4) == 0 && (C % 4) == 0) {
      ProfScope prof(SL_PROF_REDUCE, st, work * n);
      const int rc = launch_colreduce2(op, dtype, prof, xs + l0, B, n * B, (int)S, C, sb, ss, (int)s0, (int)s1, denom, out, nullptr, st);
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
        const int rc = reduce_dispatch(op, prof, xs[l0 + i], dtype, B, C, S, sb, sc, ss, s0, s1, out + (int64_t)i * B * C, nullptr, st, plain_sum);
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
SL_API int sl_reduce_conv(const void* d_act, int dtype, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc,
                          int64_t ss, int agg, uint16_t* d_cand_bf16, float* d_out_f32, void* stream) {
  SL_REQUIRE(d_act || B * C * S == 0, "sl_reduce_conv: null activation");
  SL_REQUIRE(dtype >= SL_F32 && dtype <= SL_BF16, "sl_reduce_conv: bad dtype %d", dtype);
  SL_REQUIRE(B >= 0 && C >= 0 && S >= 0, "sl_reduce_conv: negative shape");
  SL_REQUIRE(agg == SL_CONV_MAX || agg == SL_CONV_MEAN || agg == SL_CONV_SUM, "sl_reduce_conv: bad agg %d", agg);
  SL_REQUIRE(d_cand_bf16 || d_out_f32, "sl_reduce_conv: no output");
  if (B * C == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_REDUCE, st, (double)B * C * S * dtype_size(dtype));
  return reduce_dispatch(agg == SL_CONV_MAX ? OP_MAX : OP_SUM, prof, d_act, dtype, B, C, S, sb, sc, ss, 0, S, d_cand_bf16, d_out_f32, st,
                         agg == SL_CONV_SUM);
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

SL_API int sl_reduce_tokens(const void* d_act, int dtype, int64_t B, int64_t T, int64_t F, int64_t sb, int64_t st_,
                            int64_t sf, int agg, int64_t pos, uint16_t* d_cand_bf16, float* d_out_f32,
                            void* stream) {
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
  return reduce_dispatch(op, prof, d_act, dtype, B, F, T, sb, sf, st_, t0, t1, d_cand_bf16, d_out_f32, st);
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
  g_nt_min_bytes = nt_min_bytes < 0 ? -1 : nt_min_bytes;
  g_tail_bytes = tail_bytes < 0 ? -1 : tail_bytes;
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
