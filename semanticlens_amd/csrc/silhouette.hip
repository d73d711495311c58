// K23 — silhouette of a clustered concept DB: scikit-learn's `silhouette_samples` / `silhouette_score`
// (sklearn/metrics/cluster/_unsupervised.py, 1.7.2) per component and per label set, the model-selection criterion behind
// `polysemanticity_facets(n_clusters="auto")`.
//
//   V (C,n,D) fp32, labels (m,C,n) int32 -> samples (m,C,n) fp64 (optional), mean (m,C) fp64
//
//   cnt_j = #{l : label_l = j},  S_i(j) = sum_{l != i, label_l = j} d(i,l)
//   a_i = S_i(A) / (cnt_A - 1) for i in A,  b_i = min_{j != A, cnt_j > 0} S_i(j) / cnt_j,  s_i = (b_i - a_i) / max(a_i, b_i)
//   s_i = 0 when cnt_A == 1 or max(a_i, b_i) == 0 (scikit-learn's nan_to_num).  A label outside [0, n_clusters) takes the
//   sample out (sl_facet_stats' masking): it enters no sum, its s_i is NaN and the mean skips it.  With fewer than two
//   non-empty clusters the silhouette is not defined (scikit-learn raises): every s_i and the mean are NaN.
//
// Launch 1 (gram.hpp) writes every component's Gram matrix H = V_c V_c^T once, in fp64, into the workspace: V is read once
// per call however many label sets there are.  n <= 128 takes K9's LDS-staged kernel, larger n the one-thread-per-pair kernel.
// Launch 2 (silhouette_kernel<T>) walks H once per (component, label set) and derives the distances from it:
//   euclidean  d(i,l) = sqrt(max(H_ii + H_ll - 2 H_il, 0)),   cosine  d(i,l) = 1 - H_il / (max(sqrt H_ii, 1e-12) max(sqrt H_ll, 1e-12))
// Thread t of a group of T owns rows i = t, t + T, ...; it walks COLUMN i of the symmetric H (H[l][i], l ascending), so that
// the T threads of a group read consecutive doubles of one row of H, and adds d(i,l) to its private accumulator of
// label_l (a column of an LDS pad: label_l is the same for the whole group, so there are no bank conflicts and no dynamic
// register indexing).  l == i is skipped by index.  Labels and the diagonal terms sit in LDS.
//   T = 64  (n <= 128): one wavefront per (component, label set), four of them in a workgroup; H[c] (<= 128 KiB, usually
//            3-80 KiB) is read once from L2 / HBM by that wave.
//   T = 256 (n > 128): one workgroup per (component, label set); H[c] (up to 8 MiB) streams from L2.
// Every sum is fp64 in a fixed order (l ascending per row; rows ascending per thread; an xor-shuffle tree; the four waves
// in order): the results depend neither on the grid nor on m.  There are no float atomics.
#include "common.hpp"
#include "gram.hpp"

namespace sl {
namespace {

constexpr int kSilMaxN = 1024, kSilMaxClusters = 16, kSilMaxSets = 15;
constexpr int kSilWaveN = kGramStagedMaxN;  // up to here: one wavefront per (component, label set)

__device__ inline double sil_wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int T>  // threads per (component, label set): 64 (four groups per workgroup) or 256
__global__ __launch_bounds__(256) void silhouette_kernel(const double* __restrict__ Hall, int64_t C, int n,
                                                          const int32_t* __restrict__ labels, int m, int k, int metric,
                                                          double* __restrict__ samples, double* __restrict__ mean) {
  constexpr int G = 256 / T;                          // groups per workgroup
  constexpr int NL = T == 64 ? kSilWaveN : kSilMaxN;  // rows a group stages
  __shared__ double s_acc[kSilMaxClusters * 256];     // [cluster][thread]: S_i(j) of the row the thread is on
  __shared__ double s_diag[G * NL];                   // euclidean: H_ll; cosine: max(sqrt(H_ll), 1e-12)
  __shared__ int s_lab[G * NL];                       // label_l, -1 when out of range
  __shared__ int s_cnt[G * kSilMaxClusters];
  __shared__ double s_red[4];
  const int g = threadIdx.x / T, t = threadIdx.x % T;
  const int64_t pair = (int64_t)blockIdx.x * G + g;  // = set * C + component: the index of labels, samples and mean rows
  const bool valid = pair < C * (int64_t)m;          // the last workgroup of the T = 64 grid may hold idle groups
  const int64_t c = valid ? pair % C : 0;
  const double* H = Hall + c * (int64_t)n * n;
  double* sd = s_diag + g * NL;
  int* sl_ = s_lab + g * NL;
  int* sc = s_cnt + g * kSilMaxClusters;

  if (t < kSilMaxClusters) sc[t] = 0;
  __syncthreads();
  for (int l = t; l < n; l += T) {
    int lab = valid ? labels[pair * n + l] : -1;
    if (lab < 0 || lab >= k) lab = -1;
    sl_[l] = lab;
    if (lab >= 0) atomicAdd(&sc[lab], 1);  // integer adds in LDS: the order does not matter
    const double hll = H[(size_t)l * n + l];
    const double nrm = sqrt(hll > 0.0 ? hll : 0.0);
    sd[l] = metric == 0 ? hll : (nrm > 1e-12 ? nrm : 1e-12);
  }
  __syncthreads();
  int nonempty = 0, n_in = 0;
  for (int j = 0; j < k; ++j) {
    nonempty += sc[j] > 0;
    n_in += sc[j];
  }
  const double nan = __builtin_nan("");

  double tot = 0.0;  // sum of s_i over this thread's rows
  for (int i = t; i < n; i += T) {
    const int A = sl_[i];
    double s = nan;
    if (valid && A >= 0 && nonempty >= 2) {
      double* acc = s_acc + threadIdx.x;
      for (int j = 0; j < k; ++j) acc[j * 256] = 0.0;
      const double di = sd[i];
      for (int l = 0; l < n; ++l) {
        const int lab = sl_[l];
        if (lab < 0 || l == i) continue;
        const double h = H[(size_t)l * n + i];
        double d;
        if (metric == 0) {
          d = di + sd[l] - 2.0 * h;
          d = sqrt(d > 0.0 ? d : 0.0);
        } else {
          d = 1.0 - h / (di * sd[l]);
        }
        acc[lab * 256] += d;
      }
      const int cntA = sc[A];
      if (cntA == 1) {
        s = 0.0;
      } else {
        const double a = acc[A * 256] / (double)(cntA - 1);
        double b = __builtin_huge_val();
        for (int j = 0; j < k; ++j) {
          if (j == A || sc[j] == 0) continue;
          const double bj = acc[j * 256] / (double)sc[j];
          b = bj < b ? bj : b;
        }
        const double mx = a > b ? a : b;
        s = mx == 0.0 ? 0.0 : (b - a) / mx;
      }
      tot += s;
    }
    if (valid && samples) samples[pair * n + i] = s;
  }

  tot = sil_wave_sum(tot);
  if (T == 64) {
    if (valid && t == 0) mean[pair] = nonempty >= 2 ? tot / (double)n_in : nan;
  } else {
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = tot;
    __syncthreads();
    if (valid && threadIdx.x == 0) mean[pair] = nonempty >= 2 ? (((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)n_in : nan;
  }
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API size_t sl_silhouette_ws_bytes(int64_t C, int64_t n, int64_t D) {
  (void)D;
  if (C < 0 || n < 0) return 0;
  return (size_t)C * (size_t)n * (size_t)n * 8 + 256;
}

SL_API int sl_silhouette(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* d_labels, int m, int n_clusters, int metric,
                         double* d_samples, double* d_mean, void* d_ws, size_t ws_bytes, void* stream) {
  SL_REQUIRE(C >= 0 && n >= 0 && D >= 0, "sl_silhouette: negative shape");
  SL_REQUIRE(m >= 1 && m <= kSilMaxSets, "sl_silhouette: m=%d label sets not in [1, %d]", m, kSilMaxSets);
  SL_REQUIRE(n_clusters >= 2 && n_clusters <= kSilMaxClusters, "sl_silhouette: n_clusters=%d not in [2, %d]", n_clusters, kSilMaxClusters);
  SL_REQUIRE(metric == 0 || metric == 1, "sl_silhouette: metric=%d is neither 0 (euclidean) nor 1 (cosine)", metric);
  SL_REQUIRE(n <= kSilMaxN, "sl_silhouette: n_samples=%lld exceeds the supported maximum %d", (long long)n, kSilMaxN);
  if (C == 0) return 0;
  SL_REQUIRE(n >= 2 && D >= 1, "sl_silhouette: n_samples=%lld, D=%lld: at least 2 samples of at least 1 feature", (long long)n, (long long)D);
  SL_REQUIRE(C <= 65535, "sl_silhouette: %lld components in one call (the Gram kernel's grid holds 65535: split the call)", (long long)C);
  SL_REQUIRE(d_V && d_labels && d_mean, "sl_silhouette: null pointer");
  SL_REQUIRE(d_ws && ws_bytes >= sl_silhouette_ws_bytes(C, n, D), "sl_silhouette: workspace of %zu bytes too small (%zu needed)", ws_bytes,
             sl_silhouette_ws_bytes(C, n, D));
  hipStream_t st = (hipStream_t)stream;
  double* H = reinterpret_cast<double*>(((uintptr_t)d_ws + 255) & ~(uintptr_t)255);
  {
    ProfScope prof(SL_PROF_SCORES, st, (double)C * n * D * 4);
    if (n <= kGramStagedMaxN) {
      int Dc = (int)(48 * 1024 / (4 * n)) - 1;
      if (Dc > D) Dc = (int)D;
      int64_t blocks = C;
      const int64_t cap = (int64_t)num_cus() * 8;
      if (blocks > cap) blocks = cap;
      SL_LAUNCH(prof, gram_kernel, dim3((unsigned)blocks), dim3(256), (size_t)n * (Dc + 1) * 4, st, d_V, C, (int)n, D, Dc, H);
    } else {
      int64_t bx = (n * n + 255) / 256;
      if (bx > 64) bx = 64;
      SL_LAUNCH(prof, gram_general_kernel, dim3((unsigned)bx, (unsigned)C), dim3(256), 0, st, d_V, C, (int)n, D, H);
    }
    SL_CHECK_HIP(hipGetLastError());
  }
  const int64_t pairs = C * (int64_t)m;
  if (n <= kSilWaveN)
    hipLaunchKernelGGL(silhouette_kernel<64>, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, st, (const double*)H, C, (int)n, d_labels, m,
                       n_clusters, metric, d_samples, d_mean);
  else
    hipLaunchKernelGGL(silhouette_kernel<256>, dim3((unsigned)pairs), dim3(256), 0, st, (const double*)H, C, (int)n, d_labels, m,
                       n_clusters, metric, d_samples, d_mean);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
