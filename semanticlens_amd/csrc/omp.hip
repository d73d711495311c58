// K28 — the step between two vocabulary passes of an orthogonal matching pursuit: the kernel behind decompose_components /
// probe_decompose (lens.py).  The pass itself is K6 + K17 (`topk_probe` of the residuals with k = t + 1); this file takes the
// candidates it found and, per component, appends one word to a small least-squares problem, solves it and writes the new residual.
// The rules (which candidate, when a component stops, the Cholesky append and solve) are omp_state.hpp's; nothing here restates them.
//
// Shape of the work: one wavefront per component, four per 256-thread workgroup, grid-stride over the components.  A frozen
// component costs one flag read.  Otherwise, lane-uniform scalar code picks the candidate; then
//   pass 1  the lanes walk D once, 16 bytes per lane and row where every row starts on a 16-byte boundary (D % 4 == 0 and aligned
//           bases; else 4 bytes per lane), over the new word's row, the t chosen rows and x, all loads of a chunk issued before the
//           first product, and form in float64 the squared norms of every row, the t cosines' numerators and w.x: 2 t + 3 sums, added
//           across the wave by a butterfly, so every lane holds the same bits;
//           lane 0 brings the component's packed factor and right-hand side into LDS, appends and solves (omp_state.hpp) and
//           writes the new factor row, the weights and the id back: a serial float64 chain of about t^2 operations;
//   pass 2  the lanes walk D again: r = x / |x| - sum_i (a_i / |w_i|) w_i in float64 over the t + 1 rows, which come from L2, the
//           fp32 residual stored with the same width as the loads, |r|^2 summed as in pass 1.
// The residual is recomputed from x every step, never updated from the previous one: its error does not grow with t.
// The norms of the chosen rows are summed again in every step's pass 1 (the rows are streamed for the cosines anyway) instead of being
// kept as state.  No floating-point atomics, no state shared between waves: the same inputs give the same bits.
#include <initializer_list>

#include "omp_state.hpp"
#include "rowseg_tile.hpp"

namespace sl {
namespace {

constexpr int kWaves = 4;        // per workgroup
constexpr int kPerCuWaves = 4;   // rowseg::wave_grid: at most 16 x CUs components in flight, 16 waves per CU
constexpr int kMaxTerms = omp::kMaxTerms;
static_assert(kMaxTerms == SL_OMP_MAX_TERMS && omp::kMinPivot == SL_OMP_MIN_PIVOT && omp::kResidualDone == SL_OMP_RESIDUAL_DONE,
              "the header's constants are omp_state.hpp's");

struct StepArgs {
  const float* x;
  int64_t C, D;
  const float* w;
  int64_t V;
  const float* cand_vals;
  const int64_t* cand_ids;
  int k_cand, t, s;
  double min_correlation;
  int64_t* ids;
  double* chol;
  double* rhs;
  double* coefs;
  float* corr;
  double* explained;
  int32_t* n_terms;
  int32_t* finished;
  float* residual;
  float* last;
};

__device__ inline double wave_sum(double v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// P floats of a row at p: one 16-byte access (P = 4) or one float (P = 1)
template <int P>
__device__ inline void load_piece(const float* p, float (&v)[P]) {
  if constexpr (P == 4) {
    const f4 q = *reinterpret_cast<const f4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = q[e];
  } else {
    v[0] = *p;
  }
}
template <int P>
__device__ inline void store_piece(float* p, const float (&v)[P]) {
  if constexpr (P == 4) {
    *reinterpret_cast<f4*>(p) = f4{v[0], v[1], v[2], v[3]};
  } else {
    *p = v[0];
  }
}

// A component stops with n terms: its true residual (the working row) goes to `last` unless it is there already, the working
// row becomes zeros (cosine 0 to every word in K6: later passes choose nothing), and the unused slots of `explained` repeat the
// last value.
template <int P>
__device__ inline void freeze(float* work, float* last, int64_t D, int lane, bool copy, int32_t* finished, double* explained, int n,
                              int s, double last_explained) {
  for (int64_t col = (int64_t)lane * P; col < D; col += kWave * P) {
    float v[P];
    if (copy) {
      load_piece<P>(work + col, v);
      store_piece<P>(last + col, v);
    }
#pragma unroll
    for (int e = 0; e < P; ++e) v[e] = 0.f;
    store_piece<P>(work + col, v);
  }
  if (lane == 0) {
    *finished = 1;
    for (int i = n; i < s; ++i) explained[i] = last_explained;
  }
}

// TP: the rows a step reads, t + 1, rounded up to 1, 4, 8 or 16 (registers per lane grow with it).
template <int TP, int P>
__global__ __launch_bounds__(kWaves* kWave) void omp_step_kernel(StepArgs a) {
  constexpr int NP = TP > 1 ? TP - 1 : 1;  // chosen rows at most
  __shared__ double lds_L[kWaves][omp::packed_size(kMaxTerms)];
  __shared__ double lds_b[kWaves][kMaxTerms], lds_a[kWaves][kMaxTerms], lds_g[kWaves][kMaxTerms];
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double* L = lds_L[wid];
  double* b = lds_b[wid];
  double* av = lds_a[wid];
  double* g = lds_g[wid];
  const int t = a.t, s = a.s;
  const int64_t D = a.D;
  for (int64_t c = (int64_t)blockIdx.x * kWaves + wid; c < a.C; c += (int64_t)gridDim.x * kWaves) {
    if (a.finished[c]) continue;
    int64_t* ids = a.ids + c * s;
    double* explained = a.explained + c * s;
    float* work = a.residual + c * D;
    float* last = a.last + c * D;
    const float* cand_vals = a.cand_vals + c * a.k_cand;
    const int64_t* cand_ids = a.cand_ids + c * a.k_cand;
    const double explained_so_far = t > 0 ? explained[t - 1] : 0.0;
    const omp::Choice ch = omp::choose(cand_vals, cand_ids, a.k_cand, ids, t, a.V, a.min_correlation);
    if (ch.slot < 0) {
      freeze<P>(work, last, D, lane, true, a.finished + c, explained, t, s, explained_so_far);
      continue;
    }
    const int64_t id = cand_ids[ch.slot];
    const float* x = a.x + c * D;
    const float* wn = a.w + id * D;
    const float* prev[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) prev[i] = a.w + (i < t ? ids[i] : 0) * D;

    // ---- pass 1: 2 t + 3 sums over D
    double sg[NP], sn[NP], sw = 0.0, sx = 0.0, sb = 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) sg[i] = sn[i] = 0.0;
    for (int64_t col = (int64_t)lane * P; col < D; col += kWave * P) {
      float xv[P], wv[P], pv[NP][P];
      load_piece<P>(x + col, xv);
      load_piece<P>(wn + col, wv);
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (i < t) load_piece<P>(prev[i] + col, pv[i]);
#pragma unroll
      for (int e = 0; e < P; ++e) {
        const double xe = xv[e], we = wv[e];
        sx = fma(xe, xe, sx);
        sw = fma(we, we, sw);
        sb = fma(we, xe, sb);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (i < t) {
#pragma unroll
          for (int e = 0; e < P; ++e) {
            const double pe = pv[i][e];
            sg[i] = fma(pe, (double)wv[e], sg[i]);
            sn[i] = fma(pe, pe, sn[i]);
          }
        }
    }
    sx = wave_sum(sx);
    sw = wave_sum(sw);
    sb = wave_sum(sb);
#pragma unroll
    for (int i = 0; i < NP; ++i)
      if (i < t) {
        sg[i] = wave_sum(sg[i]);
        sn[i] = wave_sum(sn[i]);
      }
    const double nx = sqrt(sx), nw = sqrt(sw);

    // ---- append and solve: lane 0, on the wave's LDS
    int ok = 0;
    if (lane == 0) {
      double* Lg = a.chol + c * omp::packed_size(s);
      double* rhs = a.rhs + c * s;
      for (int i = 0; i < omp::packed_size(t); ++i) L[i] = Lg[i];
      for (int i = 0; i < t; ++i) b[i] = rhs[i];
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (i < t) g[i] = sg[i] / (nw * sqrt(sn[i]));
      double pivot;
      ok = omp::word_usable(sw) && omp::chol_append(L, t, g, &pivot);
      if (ok) {
        b[t] = sb / (nw * nx);
        omp::chol_solve(L, t + 1, b, av);
        for (int j = 0; j <= t; ++j) Lg[omp::packed_at(t, j)] = L[omp::packed_at(t, j)];
        rhs[t] = b[t];
        double* coefs = a.coefs + c * s;
        for (int i = 0; i <= t; ++i) coefs[i] = av[i];
        ids[t] = id;
        a.corr[c * s + t] = cand_vals[ch.slot];
        a.n_terms[c] = t + 1;
      }
    }
    ok = __shfl(ok, 0, kWave);
    if (!ok) {
      freeze<P>(work, last, D, lane, true, a.finished + c, explained, t, s, explained_so_far);
      continue;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // lane 0's weights, read by every lane
    __builtin_amdgcn_wave_barrier();
    double cf[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) cf[i] = i < t ? av[i] / sqrt(sn[i]) : 0.0;
    const double cfn = av[t] / nw;

    // ---- pass 2: the residual, from x
    float* dst = t == s - 1 ? last : work;
    double r2 = 0.0;
    for (int64_t col = (int64_t)lane * P; col < D; col += kWave * P) {
      float xv[P], wv[P], pv[NP][P], out[P];
      load_piece<P>(x + col, xv);
      load_piece<P>(wn + col, wv);
#pragma unroll
      for (int i = 0; i < NP; ++i)
        if (i < t) load_piece<P>(prev[i] + col, pv[i]);
#pragma unroll
      for (int e = 0; e < P; ++e) {
        double r = (double)xv[e] / nx;
#pragma unroll
        for (int i = 0; i < NP; ++i)
          if (i < t) r = fma(-cf[i], (double)pv[i][e], r);
        r = fma(-cfn, (double)wv[e], r);
        r2 = fma(r, r, r2);
        out[e] = (float)r;
      }
      store_piece<P>(dst + col, out);
    }
    r2 = wave_sum(r2);
    const double now = 1.0 - r2;
    if (lane == 0) explained[t] = now;
    // (the last step wrote `last` itself; the working row then still holds the residual before it)
    if (omp::residual_done(r2)) freeze<P>(work, last, D, lane, dst == work, a.finished + c, explained, t + 1, s, now);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  // the LDS is lane 0's again in the next trip
    __builtin_amdgcn_wave_barrier();
  }
}

template <int P>
__global__ __launch_bounds__(kWaves* kWave) void omp_init_kernel(const float* __restrict__ x, int64_t C, int64_t D, int s,
                                                                  int64_t* __restrict__ ids, double* __restrict__ coefs,
                                                                  float* __restrict__ corr, double* __restrict__ explained,
                                                                  int32_t* __restrict__ n_terms, int32_t* __restrict__ finished,
                                                                  float* __restrict__ residual, float* __restrict__ last) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const float nan = __builtin_nanf("");
  for (int64_t c = (int64_t)blockIdx.x * kWaves + wid; c < C; c += (int64_t)gridDim.x * kWaves) {
    const float* xr = x + c * D;
    double sx = 0.0;
    for (int64_t col = (int64_t)lane * P; col < D; col += kWave * P) {
      float xv[P];
      load_piece<P>(xr + col, xv);
#pragma unroll
      for (int e = 0; e < P; ++e) sx = fma((double)xv[e], (double)xv[e], sx);
    }
    sx = wave_sum(sx);
    const bool valid = omp::word_usable(sx);  // a zero row, an infinite or a NaN coordinate: nothing to decompose
    const double nx = sqrt(sx);
    for (int64_t col = (int64_t)lane * P; col < D; col += kWave * P) {
      float xv[P], out[P];
      load_piece<P>(xr + col, xv);
#pragma unroll
      for (int e = 0; e < P; ++e) out[e] = valid ? (float)((double)xv[e] / nx) : 0.f;
      store_piece<P>(residual + c * D + col, out);
      if (!valid) {
#pragma unroll
        for (int e = 0; e < P; ++e) out[e] = nan;
        store_piece<P>(last + c * D + col, out);
      }
    }
    if (lane < s) {
      ids[c * s + lane] = -1;
      coefs[c * s + lane] = 0.0;
      corr[c * s + lane] = nan;
      explained[c * s + lane] = valid ? 0.0 : (double)nan;
    }
    if (lane == 0) {
      n_terms[c] = 0;
      finished[c] = valid ? 0 : 1;
    }
  }
}

unsigned grid_for_components(int64_t C) {
  const int64_t waves = rowseg::wave_grid(C, num_cus(), kPerCuWaves);
  return (unsigned)((waves + kWaves - 1) / kWaves);
}

// 16-byte accesses need every row of x, w and the residuals on a 16-byte boundary
bool rows_are_16_byte_aligned(int64_t D, std::initializer_list<const void*> bases) {
  if (D % 4 != 0) return false;
  for (const void* p : bases)
    if ((uintptr_t)p & 15) return false;
  return true;
}

template <int TP>
void launch_step(ProfScope& prof, hipStream_t st, bool vec, const StepArgs& a) {
  const dim3 grid(grid_for_components(a.C)), block(kWaves * kWave);
  if (vec)
    SL_LAUNCH(prof, (omp_step_kernel<TP, 4>), grid, block, 0, st, a);
  else
    SL_LAUNCH(prof, (omp_step_kernel<TP, 1>), grid, block, 0, st, a);
}

bool aligned_to(const void* p, uintptr_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_omp_init(const float* d_x, int64_t C, int64_t D, int64_t s, int64_t* d_ids, double* d_coefs, float* d_corr,
                       double* d_explained, int32_t* d_n_terms, int32_t* d_finished, float* d_residual, float* d_last, void* stream) {
  SL_REQUIRE(C >= 0, "sl_omp_init: negative component count");
  SL_REQUIRE(s >= 1 && s <= kMaxTerms, "sl_omp_init: s = %lld not in [1, %d]", (long long)s, kMaxTerms);
  SL_REQUIRE(D >= 1, "sl_omp_init: D = %lld, a component has at least one coordinate", (long long)D);
  if (C == 0) return 0;
  SL_REQUIRE(d_x && d_ids && d_coefs && d_corr && d_explained && d_n_terms && d_finished && d_residual && d_last,
             "sl_omp_init: null components, state or residuals");
  SL_REQUIRE(aligned_to(d_ids, 8) && aligned_to(d_coefs, 8) && aligned_to(d_explained, 8),
             "sl_omp_init: ids, coefs or explained are not 8-byte aligned");
  SL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_corr, 4) && aligned_to(d_n_terms, 4) && aligned_to(d_finished, 4) &&
                 aligned_to(d_residual, 4) && aligned_to(d_last, 4),
             "sl_omp_init: components, correlations, counts, flags or residuals are not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)C * (double)D * 12);
  const dim3 grid(grid_for_components(C)), block(kWaves * kWave);
  if (rows_are_16_byte_aligned(D, {d_x, d_residual, d_last}))
    SL_LAUNCH(prof, omp_init_kernel<4>, grid, block, 0, st, d_x, C, D, (int)s, d_ids, d_coefs, d_corr, d_explained, d_n_terms, d_finished,
              d_residual, d_last);
  else
    SL_LAUNCH(prof, omp_init_kernel<1>, grid, block, 0, st, d_x, C, D, (int)s, d_ids, d_coefs, d_corr, d_explained, d_n_terms, d_finished,
              d_residual, d_last);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_omp_step(const float* d_x, int64_t C, int64_t D, const float* d_w, int64_t V, const float* d_cand_vals,
                       const int64_t* d_cand_ids, int64_t k_cand, int64_t t, int64_t s, double min_correlation, int64_t* d_ids,
                       double* d_chol, double* d_rhs, double* d_coefs, float* d_corr, double* d_explained, int32_t* d_n_terms,
                       int32_t* d_finished, float* d_residual, float* d_last, void* stream) {
  SL_REQUIRE(C >= 0, "sl_omp_step: negative component count");
  SL_REQUIRE(s >= 1 && s <= kMaxTerms, "sl_omp_step: s = %lld not in [1, %d]", (long long)s, kMaxTerms);
  SL_REQUIRE(t >= 0 && t < s, "sl_omp_step: t = %lld not in [0, s = %lld)", (long long)t, (long long)s);
  SL_REQUIRE(k_cand >= t + 1 && k_cand <= 0x7FFFFFFF, "sl_omp_step: k_cand = %lld, step t = %lld needs at least t + 1 candidates",
             (long long)k_cand, (long long)t);
  SL_REQUIRE(D >= 1, "sl_omp_step: D = %lld, a component has at least one coordinate", (long long)D);
  SL_REQUIRE(min_correlation >= 0.0 && min_correlation < 1.0, "sl_omp_step: min_correlation = %g not in [0, 1)", min_correlation);
  if (C == 0) return 0;
  SL_REQUIRE(V >= 1, "sl_omp_step: V = %lld, an empty vocabulary", (long long)V);
  SL_REQUIRE(d_x && d_w && d_cand_vals && d_cand_ids, "sl_omp_step: null components, vocabulary or candidates");
  SL_REQUIRE(d_ids && d_chol && d_rhs && d_coefs && d_corr && d_explained && d_n_terms && d_finished && d_residual && d_last,
             "sl_omp_step: null state or residuals");
  SL_REQUIRE(aligned_to(d_cand_ids, 8) && aligned_to(d_ids, 8) && aligned_to(d_chol, 8) && aligned_to(d_rhs, 8) &&
                 aligned_to(d_coefs, 8) && aligned_to(d_explained, 8),
             "sl_omp_step: candidate ids, ids, factor, right-hand side, coefs or explained are not 8-byte aligned");
  SL_REQUIRE(aligned_to(d_x, 4) && aligned_to(d_w, 4) && aligned_to(d_cand_vals, 4) && aligned_to(d_corr, 4) &&
                 aligned_to(d_n_terms, 4) && aligned_to(d_finished, 4) && aligned_to(d_residual, 4) && aligned_to(d_last, 4),
             "sl_omp_step: components, vocabulary, candidate values, correlations, counts, flags or residuals are not 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const StepArgs a{d_x,   C,     D,      d_w,     V,      d_cand_vals, d_cand_ids,  (int)k_cand, (int)t,     (int)s,
                   min_correlation, d_ids, d_chol, d_rhs, d_coefs, d_corr, d_explained, d_n_terms, d_finished, d_residual, d_last};
  const bool vec = rows_are_16_byte_aligned(D, {d_x, d_w, d_residual, d_last});
  ProfScope prof(SL_PROF_TOPK, st, (double)C * (double)(t + 2) * (double)D * 8);  // t + 1 rows and x, twice
  const int rows = (int)t + 1;
  if (rows == 1)
    launch_step<1>(prof, st, vec, a);
  else if (rows <= 4)
    launch_step<4>(prof, st, vec, a);
  else if (rows <= 8)
    launch_step<8>(prof, st, vec, a);
  else
    launch_step<16>(prof, st, vec, a);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
