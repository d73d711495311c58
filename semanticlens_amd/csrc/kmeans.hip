// K9 — polysemanticity_score (semanticlens/scores.py:131-185).
//
// The reference loops over components on the host and runs scikit-learn
// `KMeans(n_clusters, n_init=10, random_state=123).fit(e)` on each (n_samples, D) block
// (scores.py:167; 6.3 ms per component), then `1 - clarity_score(centres)`.
// Because it hands sklearn a torch tensor, sklearn clusters in float64.
//
// Here one launch computes every component's n x n Gram matrix H = V V^T in fp64 (HBM-bound:
// C*n*D*4 bytes read once), and a second launch runs the whole KMeans procedure per component on
// the *centred* Gram matrix G, one wavefront per component:
//   * k-means centres are always means of point subsets S_k, so every quantity sklearn computes
//     from coordinates follows from G:  ||x_i - c_k||^2 = G_ii - 2/|S_k| sum_{j in S_k} G_ij + W_k,
//     W_k = 1/|S_k|^2 sum_{j,l in S_k} G_jl;  ||c_k - c'_k||^2 likewise.
//   * the random draws of k-means++ (first centre, the candidate thresholds per further centre) do not depend
//     on the data: the host replays numpy's RandomState for them (semanticlens_amd/scores.py
//     kmeans_draws) and passes them in.
// The procedure, restated from sklearn/cluster/_kmeans.py (1.7.2), is written ONCE (`kmeans_component` and the steps above it):
//   * _kmeans_plusplus: n_local_trials = 2 + int(ln k) candidates per further centre, np.searchsorted on the cumulative
//     closest distances, np.argmin (first minimum) over the candidates' potentials;
//   * _kmeans_single_lloyd: E-step = first minimum of ||c_j||^2 - 2 x_i.c_j (strict '<'); empty clusters take, in ascending
//     cluster id, the points farthest from their own centre (np.argmax from -inf, descending distance) and those points leave
//     their old cluster (_relocate_empty_clusters_dense); nothing moves when the largest distance is 0 (its early return): the
//     cluster then stays empty, is never a point's nearest, and _average_centers parks it on the biggest cluster's centre.
//     Caveats: with two or more empty clusters sklearn hands out the far points in np.argpartition's order, which is not
//     sorted among the n_empty farthest — the SET of relocated points is the same, which cluster id gets which may differ
//     (the score is symmetric in the ids); and "distance == 0" is tested in Gram space here, in feature space there (a centre
//     of >= 3 duplicates may round off it);
//   * strict convergence (labels unchanged) / tol = mean(var) * 1e-4 on the summed squared centre shifts / 300 iterations,
//     a final E-step when not strictly converged, best of n_init by inertia unless `_is_same_clustering`;
//   * scores.py:168-185: 1 - clarity(centres) of the chosen run, or the fallback score when a cluster has < 2 labels.
// It is instantiated twice, for the two places a component's state (kmeans_layout.hpp) can live:
//   * LDS variant (`kmeans2_kernel`): k = 2 fixed at compile time, n <= 128, state in dynamic LDS, the draws a kernel argument
//     (no copy, no synchronise), r_i = mean_j H_ij resident, two register accumulators in `subset_stats`, and the closing
//     score of the two centres from raw H (`score_two_from_H`);
//   * workspace variant (`kmeansk_kernel`): k <= 16 at run time, n <= 1024, state in a per-component slice of the workspace
//     (L2-resident: one wavefront walks it), the draws copied to the device, r_i re-summed from H where the fallback needs it,
//     a (k x 64) LDS pad of per-lane accumulators, and the closing score from the centred sums (`score_centres`).
// Everything else — every decision rule — is the same code.  The per-cluster scalars are lane-uniform: registers in the LDS
// variant, static LDS in the workspace variant.
// Checked against scikit-learn on the host first (a numpy transcription of this procedure: 460 components, k = 2..6, with
// duplicated points that force relocations — every clustering identical) and on the device by tests/test_gpu_parity.py.
// fp64 Gram-space arithmetic is not bit-identical to sklearn's coordinate arithmetic; decisions can
// differ only on numerical near-ties.  One kind is structural, not a coincidence: two mutually nearest outliers j1, j2
// (nobody else closer to them than the centres chosen so far) have k-means++ potentials S + d(j1, j2) EACH, so which of
// the two scikit-learn takes hangs on the rounding of its BLAS distances (tools/k9_postmortem.py; ~1 in 1 500 components
// of tiny random inputs ends in another clustering for it: profiles/r05_k9_near_tie.txt).
#include "common.hpp"
#include "gram.hpp"
#include "kmeans_layout.hpp"

namespace sl {
namespace {

using namespace k9;
static_assert(kLdsMaxN == kGramStagedMaxN, "the LDS variant takes what the staged Gram kernel takes");

// ---- launch 1: H[c] = V_c V_c^T (fp64 accumulation of exact fp32 products): gram_kernel / gram_general_kernel, gram.hpp ----

// ---- launch 2: KMeans per component, one wave per component ---------------------------------------
__device__ inline double wave_sum(double v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ inline double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}

// The data-independent draws.  LDS variant: by value in the kernel arguments.  Workspace variant: up to 32 x 15 x 4 doubles
// do not fit there, so device pointers.  u(init, cc, t): the t-th threshold for centre cc >= 1 of run `init`.
struct DrawsArg {
  int n_init;
  int first[32];
  double rand[32][2];
  __device__ int first_centre(int init) const { return first[init]; }
  __device__ double u(int init, int, int t) const { return rand[init][t]; }
};
struct DrawsPtr {
  int n_init, k, trials;
  const int32_t* first;
  const double* rnd;
  __device__ int first_centre(int init) const { return first[init]; }
  __device__ double u(int init, int cc, int t) const { return rnd[((size_t)init * (k - 1) + (cc - 1)) * trials + t]; }
};

// Per-cluster scalars of the current / next member sets.  Every lane computes and writes the same value, so the record can sit
// in registers (LDS variant: nothing of the k = 2 decision chain waits for an LDS round trip) or in static LDS (workspace variant).
template <int KMAX>
struct Clusters {
  double cnt[KMAX], W[KMAX], ncnt[KMAX], nW[KMAX], x[KMAX];
  int seed[KMAX], count[KMAX], map[KMAX];
};
// a[j] and a[j] = v under a run-time j; at two clusters a select, so that a record in registers is never indexed through memory
template <class T, int K>
__device__ inline T at(const T (&a)[K], int j) {
  if constexpr (K == 2) return j == 0 ? a[0] : a[1];
  else return a[j];
}
template <class T, int K>
__device__ inline void put(T (&a)[K], int j, T v) {
  if constexpr (K == 2) (j == 0 ? a[0] : a[1]) = v;
  else a[j] = v;
}

// One component's state: the arrays of kmeans_layout.hpp over `base`.  KFIX = 2: the LDS variant; 0: k and trials at run time.
template <int KFIX>
struct State {
  static constexpr int kFix = KFIX;
  static constexpr int kMaxK = KFIX ? KFIX : kMaxClusters;
  static constexpr int kMaxT = KFIX ? 2 : kMaxTrials;  // 2 + int(ln 2) = 2
  int n, k_, trials_;
  double *G, *r, *s, *sn, *closest, *cand;
  int *label, *label_old, *member, *best_label, *best_member;
  Clusters<kMaxK>* cl;

  __device__ State(unsigned char* base, const Layout& L, int n, int k, int trials, Clusters<kMaxK>* cl)
      : n(n), k_(k), trials_(trials), cl(cl) {
    auto d = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
    auto q = [&](size_t off) { return reinterpret_cast<int*>(base + off); };
    G = d(L.G); r = d(KFIX ? L.r : L.closest); s = d(L.s); sn = d(L.sn); closest = d(L.closest); cand = d(L.cand);
    label = q(L.label); label_old = q(L.label_old); member = q(L.member); best_label = q(L.best_label); best_member = q(L.best_member);
  }
  __device__ int k() const {
    if constexpr (KFIX != 0) return KFIX;
    else return k_;
  }
  __device__ int trials() const {
    if constexpr (KFIX != 0) return kMaxT;
    else return trials_;
  }
  __device__ double Gd(int i) const { return G[(size_t)i * n + i]; }
  __device__ double dist_to(int i, int cc) const {
    const double d = Gd(i) + Gd(cc) - 2.0 * G[(size_t)i * n + cc];
    return d > 0.0 ? d : 0.0;
  }
  // squared distance of point i to centre j (sums `sarr`, the current cnt / W) without the G_ii term: what the E-step compares.
  // A cluster left empty (relocation's early return) is never the first minimum.
  __device__ double dpart(const double* sarr, int i, int j) const {
    const double c = at(cl->cnt, j);
    return c > 0 ? at(cl->W, j) - 2.0 * sarr[(size_t)j * n + i] / c : __builtin_huge_val();
  }
  // r_i = mean_j H_ij after G is built: resident, or re-summed in the same order
  __device__ double row_mean(const double* H, int i) const {
    if constexpr (KFIX != 0) {
      return r[i];
    } else {
      double t = 0.0;
      for (int b = 0; b < n; ++b) t += H[(size_t)i * n + b];
      return t / n;
    }
  }
};

// H -> centred G:  G_ij = H_ij - r_i - r_j + mu   (KMeans.fit subtracts X.mean(axis=0)).  Returns mu; sets tol.
template <class St>
__device__ inline double centre_gram(St& w, const double* H, int64_t D, double& tol, int lane) {
  const int n = w.n;
  double musum = 0.0;
  for (int i = lane; i < n; i += kWave) {
    double t = 0.0;
    for (int j = 0; j < n; ++j) t += H[(size_t)i * n + j];
    w.r[i] = t / n;  // workspace variant: parked in `closest` until G is built
    musum += t / n;
  }
  const double mu = wave_sum(musum) / n;
  __syncthreads();
  double tr = 0.0;
  for (int i = lane; i < n; i += kWave) {
    const double ri = w.r[i];
    for (int j = 0; j < n; ++j) w.G[(size_t)i * n + j] = H[(size_t)i * n + j] - ri - w.r[j] + mu;
    tr += H[(size_t)i * n + i] - 2.0 * ri + mu;
  }
  __syncthreads();
  tol = wave_sum(tr) / ((double)n * (double)D) * 1e-4;  // _tolerance: mean(var(X, axis=0)) * tol
  return mu;
}

// cl->count[j] = how many of m[0..n) equal j (lane-uniform)
template <class St>
__device__ inline void count_members(St& w, const int* m, int lane) {
  const int k = w.k();
  for (int j = 0; j < k; ++j) {
    int c = 0;
    for (int i0 = 0; i0 < w.n; i0 += kWave) c += __popcll(__ballot(i0 + lane < w.n && m[i0 + lane] == j));
    w.cl->count[j] = c;
  }
  __syncthreads();
}

// _kmeans_plusplus, one further centre cc >= 1: its id; `closest` and `pot` move on while more centres follow
template <class St, class Dr>
__device__ inline int seed_next_centre(St& w, const Dr& dr, int init, int cc, double& pot, int lane) {
  const int n = w.n, trials = w.trials();
  const bool more = cc + 1 < w.k();
  int cand[St::kMaxT];
  double v[St::kMaxT];
#pragma unroll
  for (int t = 0; t < St::kMaxT; ++t) {
    cand[t] = n;
    v[t] = t < trials ? dr.u(init, cc, t) * pot : 0.0;
  }
  double cs = 0.0;
  for (int i = 0; i < n; ++i) {  // lane-uniform: searchsorted(cumsum(closest), rand * pot), side='left'
    cs += w.closest[i];
#pragma unroll
    for (int t = 0; t < St::kMaxT; ++t)
      if (cand[t] == n && cs >= v[t]) cand[t] = i;
  }
  int b = 0, chosen = 0;
  double best_pot = 0.0;
#pragma unroll
  for (int t = 0; t < St::kMaxT; ++t) {
    if (t >= trials) break;
    if (cand[t] >= n) cand[t] = n - 1;
    double sum = 0.0;
    for (int i = lane; i < n; i += kWave) {
      const double d = w.dist_to(i, cand[t]);
      const double mn = d < w.closest[i] ? d : w.closest[i];
      if (more) w.cand[(size_t)t * n + i] = mn;
      sum += mn;
    }
    sum = wave_sum(sum);
    if (t == 0 || sum < best_pot) {  // np.argmin: first minimum
      best_pot = sum;
      chosen = cand[t];
      b = t;
    }
  }
  pot = best_pot;
  if (more) {
    __syncthreads();
    for (int i = lane; i < n; i += kWave) w.closest[i] = w.cand[(size_t)b * n + i];
    __syncthreads();
  }
  return chosen;
}

// E-step: nearest centre, first on ties; `mem` (may be null): the member sets start as the labels
template <class St>
__device__ inline void estep(St& w, int* lab, int* mem, int lane) {
  const int k = w.k();
  for (int i = lane; i < w.n; i += kWave) {
    int bj = 0;
    double bd = w.dpart(w.s, i, 0);
    for (int j = 1; j < k; ++j) {
      const double d = w.dpart(w.s, i, j);
      if (d < bd) {
        bd = d;
        bj = j;
      }
    }
    lab[i] = bj;
    if (mem) mem[i] = bj;
  }
  __syncthreads();
}

// _relocate_empty_clusters_dense on `member` (cl->count: the E-step's label counts); lane-uniform and sequential (rare)
template <class St>
__device__ inline void relocate_empty(St& w, int lane) {
  const int n = w.n, k = w.k();
  double* dist = w.sn;  // free until subset_stats refills it
  double far = 0.0;
  for (int i = lane; i < n; i += kWave) {
    const double d = w.Gd(i) + w.dpart(w.s, i, w.label[i]);
    dist[i] = d;
    far = d > far ? d : far;
  }
  far = wave_max(far);
  __syncthreads();
  // early return when max(distances) == 0 (every point on its centre: fewer distinct points than clusters)
  for (int j = 0; j < k && far > 0.0; ++j) {
    if (w.cl->count[j] != 0) continue;
    double bestd = -__builtin_huge_val();
    int besti = 0;
    for (int i = 0; i < n; ++i) {  // np.argmax: first maximum
      const double d = dist[i];
      if (d > bestd) {
        bestd = d;
        besti = i;
      }
    }
    __syncthreads();
    if (lane == 0) {
      w.member[besti] = j;
      dist[besti] = -__builtin_huge_val();  // taken
    }
    __syncthreads();
  }
}

// member sets m[] -> sums so[j][i] = sum_{l in S_j} G_il, counts and W_j (into cl->ncnt / cl->nW); `counted`: cl->count holds m's
template <class St>
__device__ inline void subset_stats(St& w, const int* m, double* so, bool counted, int lane) {
  const int n = w.n, k = w.k();
  if (!counted) count_members(w, m, lane);
  auto finish = [&](int j, double t) {  // t: this lane's part of sum_{i in S_j} so[j][i];  W_j = the sum / |S_j|^2
    t = wave_sum(t);
    const int c = w.cl->count[j];
    w.cl->ncnt[j] = (double)c;
    w.cl->nW[j] = c ? t / ((double)c * (double)c) : 0.0;
  };
  if constexpr (St::kFix == 2) {
    // two register accumulators and W's partial sums in the same pass: the same additions in the same order as below, without
    // the LDS pad and the second walk (faster at k = 2)
    double wa = 0.0, wb = 0.0;
    for (int i = lane; i < n; i += kWave) {
      double a = 0.0, b = 0.0;
      const double* Gi = w.G + (size_t)i * n;
      for (int l = 0; l < n; ++l) {
        const double g = Gi[l];
        if (m[l] == 0) a += g;
        else b += g;
      }
      so[i] = a;
      so[n + i] = b;
      if (m[i] == 0) wa += a;
      else wb += b;
    }
    finish(0, wa);
    finish(1, wb);
  } else {
    __shared__ double acc[kMaxClusters * kWave];  // per-lane accumulators, one column per lane
    for (int i0 = 0; i0 < n; i0 += kWave) {
      const int i = i0 + lane;
      for (int j = 0; j < k; ++j) acc[j * kWave + lane] = 0.0;
      if (i < n) {
        const double* Gi = w.G + (size_t)i * n;
        for (int l = 0; l < n; ++l) acc[m[l] * kWave + lane] += Gi[l];
        for (int j = 0; j < k; ++j) so[(size_t)j * n + i] = acc[j * kWave + lane];
      }
    }
    __syncthreads();
    for (int j = 0; j < k; ++j) {
      double t = 0.0;
      for (int i = lane; i < n; i += kWave)
        if (m[i] == j) t += so[(size_t)j * n + i];
      finish(j, t);
    }
  }
  __syncthreads();
}

// _kmeans_single_lloyd from the seeds in cl->seed: labels in `label`, member sets of the final centres in `member`; the inertia
template <class St>
__device__ inline double lloyd(St& w, double tol, int lane) {
  const int n = w.n, k = w.k();
  auto& cl = *w.cl;
  for (int j = 0; j < k; ++j) {  // initial centres are the seed points: S_j = {seed_j}
    cl.cnt[j] = 1.0;
    cl.W[j] = w.Gd(cl.seed[j]);
  }
  for (int i = lane; i < n; i += kWave) {
    for (int j = 0; j < k; ++j) w.s[(size_t)j * n + i] = w.G[(size_t)i * n + cl.seed[j]];
    w.label_old[i] = -1;
  }
  __syncthreads();
  bool strict = false;
  for (int it = 0; it < 300; ++it) {
    estep(w, w.label, w.member, lane);
    count_members(w, w.label, lane);
    bool any_empty = false;
    for (int j = 0; j < k; ++j) any_empty |= (cl.count[j] == 0);
    if (any_empty) relocate_empty(w, lane);
    subset_stats(w, w.member, w.sn, !any_empty, lane);  // without a relocation the member sets are the labels just counted
    // centre shift^2 = sum_j W_old + W_new - 2 <c_old, c_new>
    for (int j = 0; j < k; ++j) {
      double x = 0.0;
      for (int i = lane; i < n; i += kWave)
        if (w.member[i] == j) x += w.s[(size_t)j * n + i];
      cl.x[j] = wave_sum(x);
    }
    __syncthreads();
    double shift = 0.0;
    for (int j = 0; j < k; ++j)  // a cluster empty on either side sits on another cluster's centre: no shift of its own
      if (cl.cnt[j] > 0 && cl.ncnt[j] > 0) shift += cl.W[j] + cl.nW[j] - 2.0 * cl.x[j] / (cl.cnt[j] * cl.ncnt[j]);
    __syncthreads();
    {
      double* t = w.s;
      w.s = w.sn;
      w.sn = t;
    }
    for (int j = 0; j < k; ++j) {
      cl.cnt[j] = cl.ncnt[j];
      cl.W[j] = cl.nW[j];
    }
    int same = 1;
    for (int i = lane; i < n; i += kWave) same &= (w.label[i] == w.label_old[i]);
    same = __all(same);
    __syncthreads();
    if (same) {
      strict = true;
      break;
    }
    if (shift <= tol) break;
    for (int i = lane; i < n; i += kWave) w.label_old[i] = w.label[i];
    __syncthreads();
  }
  if (!strict) estep(w, w.label, nullptr, lane);  // rerun the E-step so labels match the final centres
  double inertia = 0.0;
  for (int i = lane; i < n; i += kWave) inertia += w.Gd(i) + w.dpart(w.s, i, w.label[i]);
  return wave_sum(inertia);
}

// _is_same_clustering(label, best_label): every label of one run maps to a single label of the other (lane-uniform, sequential)
template <class St>
__device__ inline bool same_clustering(St& w, int lane) {
  for (int j = 0; j < w.k(); ++j) w.cl->map[j] = -1;
  __syncthreads();
  bool same = true;
  for (int i = 0; i < w.n && same; ++i) {
    const int a = w.label[i], b = w.best_label[i];
    const int m = at(w.cl->map, a);
    if (m == -1) put(w.cl->map, a, b);
    else if (m != b) same = false;
  }
  __syncthreads();
  return same;
}

// ---- the closing score of the chosen clustering, 1 - clarity(centres): one per variant, the arithmetic differs ----
// LDS variant: two centres c_k = mean_{j in S_k} x_j from raw H (x_i . x_j = H_ij);
// clarity_score (n = 2):  2 * sum(((c1^ + c2^) / 2)^2) - 1 with c^ = c / max(||c||, 1e-12)
template <class St>
__device__ inline double score_two_from_H(const St& w, const double* H, int lane) {
  const int n = w.n;
  double cA = 0.0, cB = 0.0, dAA = 0.0, dBB = 0.0, dAB = 0.0;
  for (int i = lane; i < n; i += kWave) {
    const int mi = w.best_member[i];
    (mi == 0 ? cA : cB) += 1.0;
    double a = 0.0, b = 0.0;
    for (int j = 0; j < n; ++j) {
      const double h = H[(size_t)i * n + j];
      if (w.best_member[j] == 0) a += h;
      else b += h;
    }
    if (mi == 0) {
      dAA += a;
      dAB += b;
    } else {
      dBB += b;
    }
  }
  cA = wave_sum(cA); cB = wave_sum(cB);
  dAA = wave_sum(dAA); dBB = wave_sum(dBB); dAB = wave_sum(dAB);
  double nA2 = cA > 0 ? dAA / (cA * cA) : 0.0, nB2 = cB > 0 ? dBB / (cB * cB) : 0.0;
  double dot = (cA > 0 && cB > 0) ? dAB / (cA * cB) : 0.0;
  if (cA == 0) nA2 = dot = nB2;  // _average_centers: a cluster without members takes the other one's centre
  if (cB == 0) nB2 = dot = nA2;
  const double na = sqrt(nA2 > 0 ? nA2 : 0.0), nb = sqrt(nB2 > 0 ? nB2 : 0.0);
  const double ia = 1.0 / (na > 1e-12 ? na : 1e-12), ib = 1.0 / (nb > 1e-12 ? nb : 1e-12);
  const double msq = (nA2 * ia * ia + nB2 * ib * ib + 2.0 * dot * ia * ib) / 4.0;
  return 1.0 - ((msq - 0.5) / 1.0 * 2.0);
}

// Workspace variant: k centres.  Original-space centres c_j = centred centre + mean:  c_j.c_l = g_jl + (R_j - mu) + (R_l - mu) + mu,
// g_jl = sum_{a in S_j} s_l[a] / (n_j n_l) (centred) and R_j = mean_{a in S_j} r_a, r_a = mean_b H_ab;
// clarity_score:  ((mean_j c_j^)^2.sum() - 1/k) / (k - 1) * k,  c^ = c / max(||c||, 1e-12)
template <class St>
__device__ inline double score_centres(St& w, const double* H, double mu, int lane) {
  __shared__ double s_dot[kMaxClusters * kMaxClusters];
  const int n = w.n, k = w.k();
  auto& cl = *w.cl;
  subset_stats(w, w.best_member, w.s, false, lane);
  for (int j = 0; j < k; ++j) {
    double rj = 0.0;
    for (int i = lane; i < n; i += kWave)
      if (w.best_member[i] == j) rj += w.row_mean(H, i);
    rj = wave_sum(rj);
    cl.x[j] = cl.ncnt[j] > 0 ? rj / cl.ncnt[j] : 0.0;
  }
  __syncthreads();
  for (int j = 0; j < k; ++j)
    for (int l = 0; l < k; ++l) {
      double t = 0.0;
      for (int i = lane; i < n; i += kWave)
        if (w.best_member[i] == j) t += w.s[(size_t)l * n + i];
      t = wave_sum(t);
      const bool both = cl.ncnt[j] > 0 && cl.ncnt[l] > 0;
      const double g = both ? t / (cl.ncnt[j] * cl.ncnt[l]) : 0.0;
      s_dot[j * k + l] = both ? g + (cl.x[j] - mu) + (cl.x[l] - mu) + mu : 0.0;
    }
  __syncthreads();
  if (lane == 0) {  // _average_centers: a cluster without members takes the centre of the biggest one (np.argmax: the first)
    int big = 0;
    for (int j = 1; j < k; ++j)
      if (cl.ncnt[j] > cl.ncnt[big]) big = j;
    for (int j = 0; j < k; ++j) {
      if (cl.ncnt[j] > 0) continue;
      for (int l = 0; l < k; ++l) s_dot[j * k + l] = s_dot[big * k + l];
      for (int l = 0; l < k; ++l) s_dot[l * k + j] = s_dot[l * k + big];
    }
  }
  __syncthreads();
  for (int j = 0; j < k; ++j) {  // cl.x: 1 / max(||c_j||, 1e-12) from here on
    const double nn = sqrt(s_dot[j * k + j] > 0 ? s_dot[j * k + j] : 0.0);
    cl.x[j] = 1.0 / (nn > 1e-12 ? nn : 1e-12);
  }
  __syncthreads();
  double msq = 0.0;
  for (int j = 0; j < k; ++j)
    for (int l = 0; l < k; ++l) msq += s_dot[j * k + l] * cl.x[j] * cl.x[l];
  msq /= (double)k * (double)k;
  return 1.0 - (msq - 1.0 / k) / (double)(k - 1) * (double)k;
}

// fallback (scores.py:173-184): 1 - mean_{i < min(10,n)} clarity([mean_j v_j, v_i]), clarity in fp32 there (lane-uniform)
template <class St>
__device__ inline double fallback_score(const St& w, const double* H, double mu) {
  const int n = w.n, ns = n < 10 ? n : 10;
  const double nm = sqrt(mu > 0 ? mu : 0.0);
  const double im = 1.0 / (nm > 1e-12 ? nm : 1e-12);
  double acc = 0.0;
  for (int i = 0; i < ns; ++i) {
    const double hii = H[(size_t)i * n + i];
    const double ri = w.row_mean(H, i);
    const double ni = sqrt(hii > 0 ? hii : 0.0);
    const double ii = 1.0 / (ni > 1e-12 ? ni : 1e-12);
    const double m2 = (mu * im * im + hii * ii * ii + 2.0 * ri * im * ii) / 4.0;
    acc += (m2 - 0.5) * 2.0;
  }
  return 1.0 - acc / ns;
}

// KMeans(k, n_init).fit on one component's Gram matrix H, then its polysemanticity: the whole procedure
template <class St, class Dr>
__device__ inline void kmeans_component(St& w, const Dr& dr, const double* __restrict__ H, int64_t D, int replace_empty,
                                        double* __restrict__ out, int32_t* __restrict__ min_count, int32_t* __restrict__ labels,
                                        int lane) {
  const int n = w.n, k = w.k();
  double tol;
  const double mu = centre_gram(w, H, D, tol, lane);
  double best_inertia = 0.0;
  bool have_best = false;
  for (int init = 0; init < dr.n_init; ++init) {
    const int c0 = dr.first_centre(init);
    w.cl->seed[0] = c0;
    double pot = 0.0;
    for (int i = lane; i < n; i += kWave) {
      const double d = w.dist_to(i, c0);
      w.closest[i] = d;
      pot += d;
    }
    pot = wave_sum(pot);
    __syncthreads();
    for (int cc = 1; cc < k; ++cc) w.cl->seed[cc] = seed_next_centre(w, dr, init, cc, pot, lane);
    __syncthreads();
    const double inertia = lloyd(w, tol, lane);
    // best of n_init (KMeans.fit): better inertia AND not the same clustering
    bool take = !have_best;
    if (have_best && inertia < best_inertia) take = !same_clustering(w, lane);
    if (take) {
      best_inertia = inertia;
      have_best = true;
      for (int i = lane; i < n; i += kWave) {
        w.best_label[i] = w.label[i];
        w.best_member[i] = w.member[i];
      }
    }
    __syncthreads();
  }
  // K21: scikit-learn's `labels_` of the chosen run (scores.py:167), cluster j = the j-th seeded centre
  if (labels)
    for (int i = lane; i < n; i += kWave) labels[i] = w.best_label[i];
  double poly;
  if constexpr (St::kFix == 2) poly = score_two_from_H(w, H, lane);
  else poly = score_centres(w, H, mu, lane);
  count_members(w, w.best_label, lane);
  int mc = n;  // a missing label makes it 0, as the reference's zero-filled counts do (scores.py:177)
  for (int j = 0; j < k; ++j) mc = w.cl->count[j] < mc ? w.cl->count[j] : mc;
  if (replace_empty && mc < 2) poly = fallback_score(w, H, mu);
  if (lane == 0) {
    *out = poly;
    if (min_count) *min_count = mc;
  }
}

__global__ __launch_bounds__(64) void kmeans2_kernel(const double* __restrict__ Hall, int64_t C, int n, int64_t D, DrawsArg dr,
                                                      int replace_empty, double* __restrict__ out, int32_t* __restrict__ min_count,
                                                      int32_t* __restrict__ labels) {
  extern __shared__ __align__(16) unsigned char smem[];
  Clusters<2> cl;
  const int64_t c = blockIdx.x;
  if (c >= C) return;
  State<2> w(smem, lds_layout(n), n, 2, 2, &cl);
  kmeans_component(w, dr, Hall + c * (int64_t)n * n, D, replace_empty, out + c, min_count ? min_count + c : nullptr,
                   labels ? labels + c * n : nullptr, (int)threadIdx.x);
}

__global__ __launch_bounds__(64) void kmeansk_kernel(const double* __restrict__ Hall, int64_t C, int n, int64_t D, DrawsPtr dr,
                                                      int replace_empty, unsigned char* __restrict__ ws_all, size_t ws_stride,
                                                      double* __restrict__ out, int32_t* __restrict__ min_count,
                                                      int32_t* __restrict__ labels) {
  __shared__ Clusters<kMaxClusters> cl;
  const int64_t c = blockIdx.x;
  if (c >= C) return;
  State<0> w(ws_all + c * ws_stride, ws_layout(n, dr.k), n, dr.k, dr.trials, &cl);
  kmeans_component(w, dr, Hall + c * (int64_t)n * n, D, replace_empty, out + c, min_count ? min_count + c : nullptr,
                   labels ? labels + c * n : nullptr, (int)threadIdx.x);
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API size_t sl_poly2means_ws_bytes(int64_t C, int64_t n, int64_t D) {
  (void)D;
  return poly2means_ws_bytes(C, n);
}

SL_API int sl_kmeans_trials(int n_clusters) { return n_clusters >= 1 ? 2 + (int)log((double)n_clusters) : 0; }

SL_API size_t sl_polykmeans_ws_bytes(int64_t C, int64_t n, int64_t D, int n_clusters, int n_init) {
  (void)D;
  if (C < 0 || n < 0 || n_clusters < 1 || n_init < 1) return 0;
  return polykmeans_ws_bytes(C, n, n_clusters, n_init);
}

// The one implementation behind the four entry points.  `general`: the workspace variant (sl_polykmeans*), which also checks
// n_clusters and the Gram kernel's grid; `name`: the entry point family, for the messages.
static int kmeans_impl(const char* name, bool general, bool want_labels, const float* d_V, int64_t C, int64_t n, int64_t D,
                       int n_clusters, const int32_t* h_first_center, int n_init, const double* h_rand, int replace_empty_clusters,
                       double* d_out, int32_t* d_min_count, int32_t* d_labels, void* d_ws, size_t ws_bytes, void* stream) {
  SL_REQUIRE(!want_labels || d_labels || C <= 0 || n <= 0, "%s_labels: null label pointer", name);
  SL_REQUIRE(C >= 0 && n >= 0 && D >= 0, "%s: negative shape", name);
  if (C == 0) return 0;
  const int max_n = general ? kMaxNGeneral : kLdsMaxN;
  SL_REQUIRE(!general || (n_clusters >= 2 && n_clusters <= kMaxClusters), "%s: n_clusters=%d not in [2, %d]", name, n_clusters,
             kMaxClusters);
  SL_REQUIRE(n >= n_clusters, "%s: n_samples=%lld should be >= n_clusters=%d.", name, (long long)n, n_clusters);  // sklearn's ValueError
  SL_REQUIRE(n <= max_n, "%s: n_samples=%lld exceeds the supported maximum %d", name, (long long)n, max_n);
  SL_REQUIRE(n_init >= 1 && n_init <= 32, "%s: n_init=%d not in [1, 32]", name, n_init);
  SL_REQUIRE(!general || C <= 65535, "%s: %lld components in one call (the Gram kernel's grid holds 65535: split the call)", name,
             (long long)C);
  SL_REQUIRE(d_V && d_out && h_first_center && h_rand, "%s: null pointer", name);
  const size_t need = general ? sl_polykmeans_ws_bytes(C, n, D, n_clusters, n_init) : sl_poly2means_ws_bytes(C, n, D);
  SL_REQUIRE(d_ws && ws_bytes >= need, "%s: workspace too small", name);
  for (int i = 0; i < n_init; ++i)
    SL_REQUIRE(h_first_center[i] >= 0 && h_first_center[i] < n, "%s: first centre %d out of range", name, h_first_center[i]);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* p = reinterpret_cast<unsigned char*>(((uintptr_t)d_ws + 255) & ~(uintptr_t)255);
  double* H = reinterpret_cast<double*>(p);
  p += (size_t)C * n * n * 8;
  if (!general) {
    DrawsArg dr;
    dr.n_init = n_init;
    for (int i = 0; i < n_init; ++i) {
      dr.first[i] = h_first_center[i];
      dr.rand[i][0] = h_rand[2 * i];
      dr.rand[i][1] = h_rand[2 * i + 1];
    }
    {
      ProfScope prof(SL_PROF_SCORES, st, (double)C * n * D * 4);
      int Dc = (int)(48 * 1024 / (4 * n)) - 1;
      if (Dc > D) Dc = (int)D;
      if (Dc < 1) Dc = 1;
      int64_t blocks = C;
      const int64_t cap = (int64_t)num_cus() * 8;
      if (blocks > cap) blocks = cap;
      SL_LAUNCH(prof, gram_kernel, dim3((unsigned)blocks), dim3(256), (size_t)n * (Dc + 1) * 4, st, d_V, C, (int)n, D, Dc, H);
    }
    const size_t smem = lds_bytes(n);
    if (smem > 64 * 1024)
      SL_CHECK_HIP(hipFuncSetAttribute((const void*)kmeans2_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    hipLaunchKernelGGL(kmeans2_kernel, dim3((unsigned)C), dim3(64), smem, st, (const double*)H, C, (int)n, D, dr,
                       replace_empty_clusters, d_out, d_min_count, d_labels);
  } else {
    unsigned char* slices = p;
    const size_t stride = ws_slice_bytes(n, n_clusters);
    p += (size_t)C * stride;
    DrawsPtr dr;
    dr.n_init = n_init;
    dr.k = n_clusters;
    dr.trials = sl_kmeans_trials(n_clusters);
    const size_t rand_bytes = (size_t)n_init * (n_clusters - 1) * dr.trials * 8;
    dr.rnd = reinterpret_cast<const double*>(p);
    dr.first = reinterpret_cast<const int32_t*>(p + align256(rand_bytes));
    // the data-independent draws of numpy's RandomState (host) -> device; pageable source: the copy is staged by the runtime
    SL_CHECK_HIP(hipMemcpyAsync(const_cast<double*>(dr.rnd), h_rand, rand_bytes, hipMemcpyHostToDevice, st));
    SL_CHECK_HIP(hipMemcpyAsync(const_cast<int32_t*>(dr.first), h_first_center, (size_t)n_init * 4, hipMemcpyHostToDevice, st));
    {
      ProfScope prof(SL_PROF_SCORES, st, (double)C * n * D * 4);
      int64_t bx = ((int64_t)n * n + 255) / 256;
      if (bx > 64) bx = 64;
      SL_LAUNCH(prof, gram_general_kernel, dim3((unsigned)bx, (unsigned)C), dim3(256), 0, st, d_V, C, (int)n, D, H);
    }
    hipLaunchKernelGGL(kmeansk_kernel, dim3((unsigned)C), dim3(64), 0, st, (const double*)H, C, (int)n, D, dr,
                       replace_empty_clusters, slices, stride, d_out, d_min_count, d_labels);
  }
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_poly2means(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* h_first_center, int n_init,
                         const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                         void* d_ws, size_t ws_bytes, void* stream) {
  return kmeans_impl("sl_poly2means", false, false, d_V, C, n, D, 2, h_first_center, n_init, h_rand, replace_empty_clusters, d_out,
                     d_min_count, nullptr, d_ws, ws_bytes, stream);
}

SL_API int sl_poly2means_labels(const float* d_V, int64_t C, int64_t n, int64_t D, const int32_t* h_first_center, int n_init,
                                const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                                int32_t* d_labels, void* d_ws, size_t ws_bytes, void* stream) {
  return kmeans_impl("sl_poly2means", false, true, d_V, C, n, D, 2, h_first_center, n_init, h_rand, replace_empty_clusters, d_out,
                     d_min_count, d_labels, d_ws, ws_bytes, stream);
}

SL_API int sl_polykmeans(const float* d_V, int64_t C, int64_t n, int64_t D, int n_clusters, const int32_t* h_first_center,
                         int n_init, const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                         void* d_ws, size_t ws_bytes, void* stream) {
  return kmeans_impl("sl_polykmeans", true, false, d_V, C, n, D, n_clusters, h_first_center, n_init, h_rand, replace_empty_clusters,
                     d_out, d_min_count, nullptr, d_ws, ws_bytes, stream);
}

SL_API int sl_polykmeans_labels(const float* d_V, int64_t C, int64_t n, int64_t D, int n_clusters, const int32_t* h_first_center,
                                int n_init, const double* h_rand, int replace_empty_clusters, double* d_out, int32_t* d_min_count,
                                int32_t* d_labels, void* d_ws, size_t ws_bytes, void* stream) {
  return kmeans_impl("sl_polykmeans", true, true, d_V, C, n, D, n_clusters, h_first_center, n_init, h_rand, replace_empty_clusters,
                     d_out, d_min_count, d_labels, d_ws, ws_bytes, stream);
}
