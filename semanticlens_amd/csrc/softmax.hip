// K25 — streaming softmax statistics over cosine tiles: the reduction behind label_distribution / probe_softmax (lens.py).
//
// State per row: softmax_state.hpp's (m, a, b, n), four doubles.  One launch folds a row-major candidate tile (R,B), read exactly
// as topk_tile_kernel reads one, into the state: logit = scale * candidate.  The rule that merges two states, and the special
// values, are softmax_state.hpp's; nothing here restates them.
//
// Shape of the work: one wavefront (a 64-thread workgroup) owns a row segment and walks it in chunks of 1024 columns, 16 per
// lane in four guarded 16-byte loads.  It keeps ONE reference for the whole wave, the largest finite candidate M seen so far
// (a cosine, exact in fp32), and every lane keeps its sums against M:
//   t = (c - M) * fl32(scale * log2 e),  e = v_exp_f32(t),  sa += e,  sb += t e       (fp32, 16 terms)
//   A += sa,  B += ln 2 * sb                                                          (fp64, once per chunk)
// One transcendental and six other vector instructions per element (the chunk maximum included); no rescale per element.  A chunk holds a larger
// candidate only rarely (about ln(chunks) times per row for data in random order); one ballot per chunk finds out, and only
// then does the wave reduce the new maximum and rebase its lanes' sums (fp64, softmax_state.hpp: rebase).  At the end of the
// segment the lanes' sums, all on the same M, are added across the wave in a fixed butterfly (sum_same_max) and lane 0 folds
// (scale * M, a, b) into the row's state with combine().  Error: DESIGN.md §K25.
//
// Special candidates: -inf gives e = 0 (and the multiplicand of sb is clamped, so that it adds 0 and not -inf * 0); a NaN
// makes the lane's sa NaN; +inf is kept out of M and makes sa +inf.  make() reads the kind of state off the sums.  Sums that
// are no longer finite are parked in a third accumulator before a rebase, which would turn inf * 0 into NaN.  While M is
// still -inf nothing finite was seen and the chunk is only searched for NaN and +inf.
//
// Few rows of very many columns: the columns are split over S waves per row (the rule K17 uses), each of which writes its
// segment's state to the workspace, and a second launch folds a row's S states into the row's state, one wave per row, in a
// fixed order.  No floating-point atomics anywhere: the same calls give the same bits.
#include "rowseg_tile.hpp"
#include "softmax_state.hpp"

namespace sl {
namespace {

using softmax::State;

constexpr int kMaxK = 1024;  // K17's
constexpr double kLog2e = 1.44269504088896340736;
constexpr double kLn2 = 0.693147180559945309417;

__device__ inline double shfl_xor_f64(double v, int d) { return __shfl_xor(v, d, kWave); }
__device__ inline double shfl_down_f64(double v, int d) { return __shfl_down(v, d, kWave); }

__device__ inline State shfl_down_state(const State& s, int d) {
  return State{shfl_down_f64(s.m, d), shfl_down_f64(s.a, d), shfl_down_f64(s.b, d), shfl_down_f64(s.n, d)};
}

// One wave per (row, split).  S == 1: fold columns [0,B) of the row into the state in place.  S > 1: write the state of
// columns [s*seg, (s+1)*seg) to entry (row, s) of the workspace.
__global__ __launch_bounds__(64) void softmax_tile_kernel(State* __restrict__ state, int64_t R, const float* __restrict__ cand,
                                                            int64_t ld, int64_t B, double scale, float s2, int S, int64_t seg,
                                                            State* __restrict__ ws) {
  const int lane = threadIdx.x;
  for (int64_t w = blockIdx.x; w < R * S; w += gridDim.x) {
    const auto [row, s, lo, hi] = rowseg::item(w, S, seg, B);
    const float* rowp = cand + row * ld;
    float M = -INFINITY;                // wave-uniform: the largest finite candidate so far
    double A = 0.0, Bn = 0.0, Sp = 0.0;  // the lane's sums against M (Bn in nats); Sp: parked non-finite sums
    for (int64_t base = rowseg::chunk_start((uintptr_t)(rowp + lo), lo); base < hi; base += rowseg::kChunk) {
      f4 x[4];
      rowseg::load_chunk(rowp, base, lo, hi, lane, -INFINITY, x);  // -inf adds nothing
      float bm = -INFINITY;  // fmaxf drops a NaN: those reach the sums below
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) bm = fmaxf(bm, x[u][j]);
      if (__ballot(bm > M) != 0) {  // rare: a candidate above the reference, or a +inf
        float fm = -INFINITY;
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) fm = fmaxf(fm, x[u][j] < INFINITY ? x[u][j] : -INFINITY);
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) fm = fmaxf(fm, __shfl_xor(fm, d, kWave));
        if (fm > M) {
          if (!(A < softmax::pos_inf())) Sp += A, A = 0.0, Bn = 0.0;
          const State t = softmax::rebase(State{scale * (double)M, A, Bn, 0.0}, scale * (double)fm);
          A = t.a, Bn = t.b, M = fm;
        }
      }
      if (M == -INFINITY) {  // nothing finite yet: these 1024 columns hold only -inf, NaN and +inf
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (!(x[u][j] < INFINITY)) Sp += (double)x[u][j];
        continue;
      }
      float sa = 0.f, sb = 0.f;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float t = (x[u][j] - M) * s2;
          const float e = __builtin_amdgcn_exp2f(t);
          sa += e;
          sb = fmaf(fmaxf(t, -1e30f), e, sb);
        }
      }
      A += (double)sa;
      Bn += kLn2 * (double)sb;
    }
    State part{scale * (double)M, A + Sp, Bn, 0.0};
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1)
      part = softmax::sum_same_max(part, State{part.m, shfl_xor_f64(part.a, d), shfl_xor_f64(part.b, d), 0.0});
    if (lane == 0) {
      part = softmax::make(part.m, part.a, part.b, hi > lo ? (double)(hi - lo) : 0.0);  // a split's last segment can be empty
      if (S == 1)
        state[row] = softmax::combine(state[row], part);
      else
        ws[row * S + s] = part;
    }
  }
}

// One wave per row: fold the row's S workspace states into its state.  Lane l folds entries l, l + 64, ... in ascending
// order, then the lanes are folded pairwise at distances 32, 16, ..., 1: a fixed order.
__global__ __launch_bounds__(64) void softmax_fold_kernel(State* __restrict__ state, int64_t R, const State* __restrict__ ws, int S) {
  const int lane = threadIdx.x;
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    State acc = softmax::empty_state();
    for (int s = lane; s < S; s += kWave) acc = softmax::combine(acc, ws[row * S + s]);
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) acc = softmax::combine(acc, shfl_down_state(acc, d));
    if (lane == 0) state[row] = softmax::combine(state[row], acc);
  }
}

__global__ __launch_bounds__(256) void softmax_init_kernel(State* __restrict__ state, int64_t R) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += (int64_t)gridDim.x * blockDim.x)
    state[i] = softmax::empty_state();
}

__global__ __launch_bounds__(256) void softmax_finish_kernel(const State* __restrict__ state, int64_t R, double scale,
                                                               const float* __restrict__ vals, int64_t k, float* __restrict__ probs,
                                                               double* __restrict__ log_z, double* __restrict__ entropy) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = t0; r < R; r += step) {
    const State s = state[r];
    log_z[r] = softmax::log_z(s);
    entropy[r] = softmax::entropy(s);
  }
  if (!vals) return;
  for (int64_t i = t0; i < R * k; i += step) {
    const int64_t r = i / k;
    probs[i] = (float)softmax::prob(state[r], scale * (double)vals[i], (double)(i - r * k));
  }
}

int64_t wave_grid(int64_t items) { return rowseg::wave_grid(items, num_cus(), 32); }

int check_state(const char* fn, int64_t R, const void* state) {
  SL_REQUIRE(R >= 0, "%s: negative row count", fn);
  if (R == 0) return 0;
  SL_REQUIRE(state, "%s: null state", fn);
  SL_REQUIRE(((uintptr_t)state & 7) == 0, "%s: the state is not 8-byte aligned", fn);
  return 0;
}

int check_scale(const char* fn, double scale) {
  SL_REQUIRE(scale > 0.0 && scale < softmax::pos_inf(), "%s: logit scale %g is not finite and > 0", fn, scale);
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_softmax_init(double* d_state, int64_t R, void* stream) {
  if (int rc = check_state("sl_softmax_init", R, d_state)) return rc;
  if (R == 0) return 0;
  hipLaunchKernelGGL(softmax_init_kernel, dim3(stride_grid_256(R)), dim3(256), 0, (hipStream_t)stream, (State*)d_state, R);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API size_t sl_softmax_merge_ws_bytes(int64_t R, int64_t B) {
  if (R <= 0 || B < 1) return 0;
  const int64_t S = rowseg::splits(R, B, num_cus());
  return S > 1 ? (size_t)R * (size_t)S * sizeof(State) + 256 : 0;
}

SL_API int sl_softmax_merge(double* d_state, int64_t R, const float* d_cand, int64_t ld, int64_t B, double scale, void* d_ws,
                            size_t ws_bytes, void* stream) {
  if (int rc = check_state("sl_softmax_merge", R, d_state)) return rc;
  if (int rc = rowseg::check_tile_shape("sl_softmax_merge", B, ld)) return rc;
  if (int rc = check_scale("sl_softmax_merge", scale)) return rc;
  if (R == 0) return 0;
  if (int rc = rowseg::check_tile_ptr("sl_softmax_merge", d_cand)) return rc;
  const int64_t S = rowseg::splits(R, B, num_cus());
  if (int rc = rowseg::check_items("sl_softmax_merge", R, S)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const float s2 = (float)(scale * kLog2e);  // one rounding
  SL_REQUIRE(s2 >= 1.17549435e-38f && s2 < INFINITY, "sl_softmax_merge: logit scale %g leaves fp32's normal range", scale);
  ProfScope prof(SL_PROF_SOFTMAX, st, (double)R * (double)B * 4);
  if (S == 1) {
    SL_LAUNCH(prof, softmax_tile_kernel, dim3((unsigned)wave_grid(R)), dim3(64), 0, st, (State*)d_state, R, d_cand, ld, B, scale, s2, 1,
              B, (State*)nullptr);
    SL_CHECK_HIP(hipGetLastError());
    return 0;
  }
  SL_REQUIRE(d_ws && ws_bytes >= sl_softmax_merge_ws_bytes(R, B), "sl_softmax_merge: workspace too small");
  State* ws = (State*)rowseg::align_ws(d_ws);
  const int64_t seg = rowseg::segment(B, S);
  SL_LAUNCH(prof, softmax_tile_kernel, dim3((unsigned)wave_grid(R * S)), dim3(64), 0, st, (State*)d_state, R, d_cand, ld, B, scale, s2,
            (int)S, seg, ws);
  ProfScope fold(SL_PROF_SOFTMAX, st, (double)R * (double)S * sizeof(State));
  SL_LAUNCH(fold, softmax_fold_kernel, dim3((unsigned)wave_grid(R)), dim3(64), 0, st, (State*)d_state, R, (const State*)ws, (int)S);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_softmax_finish(const double* d_state, int64_t R, double scale, const float* d_vals, int64_t k, float* d_probs,
                             double* d_log_z, double* d_entropy, void* stream) {
  if (int rc = check_state("sl_softmax_finish", R, d_state)) return rc;
  if (int rc = check_scale("sl_softmax_finish", scale)) return rc;
  if (d_vals) SL_REQUIRE(k >= 1 && k <= kMaxK, "sl_softmax_finish: k = %lld not in [1, %d]", (long long)k, kMaxK);
  if (R == 0) return 0;
  SL_REQUIRE(d_log_z && d_entropy, "sl_softmax_finish: null log_z or entropy");
  SL_REQUIRE(!d_vals || d_probs, "sl_softmax_finish: values without a place for their probabilities");
  hipStream_t st = (hipStream_t)stream;
  const int64_t items = d_vals ? R * k : R;
  ProfScope prof(SL_PROF_SOFTMAX, st, (double)R * 48 + (d_vals ? (double)R * (double)k * 8 : 0.0));
  SL_LAUNCH(prof, softmax_finish_kernel, dim3(stride_grid_256(items)), dim3(256), 0, st, (const State*)d_state, R, scale, d_vals,
            d_vals ? k : 1, d_probs, d_log_z, d_entropy);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
