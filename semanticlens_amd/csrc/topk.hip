// K17 — streaming fp32 row top-k: the selection behind label_components / search_components (lens.py).
//
// State per row: vals (R,k) fp32 + ids (R,k) int64, sorted best-first.  One launch folds a row-major candidate tile
// (R,B) — column j has the id id_base + j — into the state; a second entry point folds explicit (value, id) lists.
//
// Order (a total order; nothing upstream defines one): NaN first, then the larger value, -0.0 == +0.0, equal keys by the
// smaller id.  An empty slot is (-inf, -1) and ranks below every real candidate, a real -inf included.  The top k of a set
// under a total order is unique, so the state does not depend on how the candidates were cut into tiles; a (value, id) pair
// travels with its own bits (the sign of a zero and a NaN's payload come back as they went in).
//
// Shape of the work: rows are independent and after the first tiles nearly every candidate falls below the row's k-th
// entry, so the hot loop is a 16-byte read per lane against ONE threshold and insertion is the rare path.  One wavefront
// (a 64-thread workgroup: its barriers are free) owns a row segment.  Its LDS holds n = pow2 >= k + 128 entries: the sorted
// state in [0,k) and, behind it, the candidates that beat the threshold since the last sort.  When that buffer cannot take
// another 64 the wave sorts all n entries (bitonic, in LDS), which leaves the new top k in front and a new threshold.
// Memory-bound: R*B*4 bytes read once; the state is read and written only by rows that saw a passing candidate.
//
// Few rows (search: a handful of queries against tens of thousands of components): the columns are split over S waves per
// row, each of which selects its segment's top k into a workspace (filtered by the state's k-th entry: what that rejects
// cannot reach the result), and a second launch folds the S lists into the state with the explicit-id kernel.
//
// K29 (sl_topk_merge_biased) is the same fold of the same tile under another score: column j of row r ranks by
// biased_score(cand[r][j], row_bias[r], col_bias[j]) (biased_score.hpp), computed in registers from the chunk the wave holds and
// the chunk's 16 column biases per lane, so no adjusted tile is ever written.  The state then holds scores; the threshold test,
// the LDS selection, the split rows and the list fold do not know the difference.
#include "biased_score.hpp"
#include "packed_best.hpp"  // f32_order_key
#include "rowseg_tile.hpp"

namespace sl {
namespace {

constexpr int kMaxK = 1024;
constexpr int64_t kMaxId = (int64_t)1 << 62;
constexpr int kMinBuf = 128;  // room behind the state: at least two appends of 64

// f32_order_key (packed_best.hpp) of a slot; the empty slot's key is 0, below every real value's
__device__ inline uint32_t entry_key(float v, int64_t id) { return id < 0 ? 0u : f32_order_key(v); }

// One wavefront's selection state in LDS.  Every member function is called by all 64 lanes together.
struct WaveTopK {
  float* v;      // n values
  int64_t* id;   // n ids
  int n, k;
  int count;     // entries in the buffer [k, k + count), wave-uniform
  uint32_t tk;   // threshold: key and id of the k-th entry; a candidate must be strictly better
  int64_t tid;

  __device__ inline bool passes(uint32_t key, int64_t cid) const { return better(key, cid, tk, tid); }

  // start from a state in global memory (or from empty slots when gv is NULL)
  __device__ inline void load(const float* gv, const int64_t* gid, int lane) {
    for (int i = lane; i < k; i += kWave) {
      v[i] = gv ? gv[i] : -INFINITY;
      id[i] = gv ? gid[i] : (int64_t)-1;
    }
    count = 0;
    __syncthreads();
    tk = entry_key(v[k - 1], id[k - 1]);
    tid = id[k - 1];
  }

  // a threshold from elsewhere (the state a partial selection will later be folded into)
  __device__ inline void raise_threshold(float ov, int64_t oid) {
    const uint32_t ok = entry_key(ov, oid);
    if (better(ok, oid, tk, tid)) tk = ok, tid = oid;
  }

  // bitonic sort of all n entries, best first; afterwards [0,k) is the top k of state + buffer
  __device__ inline void flush(int lane) {
    for (int i = k + count + lane; i < n; i += kWave) v[i] = -INFINITY, id[i] = -1;
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int t = lane; t < (n >> 1); t += kWave) {
          const int i = 2 * t - (t & (stride - 1)), j = i + stride;
          const float vi = v[i], vj = v[j];
          const int64_t ii = id[i], ij = id[j];
          const uint32_t ki = entry_key(vi, ii), kj = entry_key(vj, ij);
          const bool desc = (i & size) == 0;
          if (desc ? better(kj, ij, ki, ii) : better(ki, ii, kj, ij)) {
            v[i] = vj, id[i] = ij;
            v[j] = vi, id[j] = ii;
          }
        }
        __syncthreads();
      }
    }
    count = 0;
    const float nv = v[k - 1];
    const int64_t nid = id[k - 1];
    raise_threshold(nv, nid);
  }

  // append the lanes' candidates that pass (`pass` is false on lanes that hold none)
  __device__ inline void push(bool pass, float cv, int64_t cid, int lane) {
    unsigned long long mask = __ballot(pass);
    if (mask == 0) return;
    if (k + count + kWave > n) {  // no room for 64 more: sort, which empties the buffer (n - k >= 128) and moves the threshold
      flush(lane);
      pass = pass && passes(f32_order_key(cv), cid);
      mask = __ballot(pass);
      if (mask == 0) return;
    }
    if (pass) {
      const int pos = k + count + (int)__popcll(mask & ((1ull << lane) - 1ull));
      v[pos] = cv, id[pos] = cid;
    }
    count += (int)__popcll(mask);
  }

  __device__ inline void store(float* gv, int64_t* gid, int lane) {
    __syncthreads();
    for (int i = lane; i < k; i += kWave) gv[i] = v[i], gid[i] = id[i];
  }
};

// LDS entries of a wave: the state and at least kMinBuf behind it (k <= kMaxK on both sides)
__host__ __device__ inline int pow2_entries(int k) {
  int n = 256;
  while (n < k + kMinBuf) n <<= 1;
  return n;
}

// The column biases of piece u of the chunk at column `base`, laid out as rowseg::load_chunk lays out the tile's: columns
// [base + (u * 64 + lane) * 4, + 4), 0 where a column is outside [lo, hi) (nothing outside the segment is read).  colb + base lies
// on a 16-byte boundary only when the caller's slice of the bias vector happens to start where the row does, so a whole piece is
// copied as 16 bytes of 4-byte alignment (gfx950 runs with unaligned global access enabled; preprocess.hip: load12): one
// global_load_dwordx4 either way.
__device__ inline f4 load_bias_piece(const float* __restrict__ colb, int64_t base, int u, int64_t lo, int64_t hi, int lane) {
  const int64_t c = base + (int64_t)(u * kWave + lane) * 4;
  f4 q;
  if (c >= lo && c + 4 <= hi) {
    __builtin_memcpy(&q, colb + c, 16);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = (c + j >= lo && c + j < hi) ? colb[c + j] : 0.f;
  }
  return q;
}

// One wave per (row, split).  S == 1: fold columns [0,B) of the row into the state in place.  S > 1: select the top k of
// columns [s*seg, (s+1)*seg) into list s of the row in the workspace (wv / wid: (R, S, k)).
// kBiased (K29): the candidates are biased_score(cand, rowb[row], colb[column]); rowb and colb are not looked at otherwise.
template <bool kBiased>
__global__ __launch_bounds__(64) void topk_tile_kernel(float* __restrict__ vals, int64_t* __restrict__ ids, int64_t R, int k,
                                                         const float* __restrict__ cand, int64_t ld, int64_t B, int64_t id_base,
                                                         int S, int64_t seg, float* __restrict__ wv, int64_t* __restrict__ wid,
                                                         const float* __restrict__ rowb, const float* __restrict__ colb) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  WaveTopK st;
  st.k = k;
  st.n = pow2_entries(k);
  st.id = reinterpret_cast<int64_t*>(smem);
  st.v = reinterpret_cast<float*>(smem + (size_t)st.n * 8);
  for (int64_t w = blockIdx.x; w < R * S; w += gridDim.x) {
    const auto [row, s, lo, hi] = rowseg::item(w, S, seg, B);
    float* gv = vals + row * k;
    int64_t* gid = ids + row * k;
    __syncthreads();  // the previous item's stores have read the LDS
    if (S == 1) {
      st.load(gv, gid, lane);
    } else {
      st.load(nullptr, nullptr, lane);
      st.raise_threshold(gv[k - 1], gid[k - 1]);
    }
    bool touched = false;
    const float* rowp = cand + row * ld;
    float rb = 0.f;
    if constexpr (kBiased) rb = rowb[row];
    for (int64_t base = rowseg::chunk_start((uintptr_t)(rowp + lo), lo); base < hi; base += rowseg::kChunk) {
      f4 x[4];
      rowseg::load_chunk(rowp, base, lo, hi, lane, 0.f, x);
      if constexpr (kBiased) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const f4 q = load_bias_piece(colb, base, u, lo, hi, lane);
#pragma unroll
          for (int j = 0; j < 4; ++j) x[u][j] = biased_score(x[u][j], rb, q[j]);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        // the common case: no key in these 256 columns reaches the k-th entry's (columns outside [lo,hi) read as 0.0, or as the
        // score of a zero cosine under a zero column bias, and are sorted out below whatever that is)
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) any = any || f32_order_key(x[u][j]) >= st.tk;
        if (__ballot(any) == 0) continue;
        const int64_t c = base + (int64_t)(u * kWave + lane) * 4;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool pass = c + j >= lo && c + j < hi && st.passes(f32_order_key(x[u][j]), id_base + c + j);
          if (__ballot(pass) == 0) continue;
          touched = true;
          st.push(pass, x[u][j], id_base + c + j, lane);
        }
      }
    }
    if (S > 1) {
      if (st.count) st.flush(lane);
      st.store(wv + (row * S + s) * k, wid + (row * S + s) * k, lane);
    } else if (touched) {  // wave-uniform: set from a ballot
      if (st.count) st.flush(lane);
      st.store(gv, gid, lane);
    }
  }
}

// One wave per row: fold M explicit (value, id) entries per row into the state.  Entries with a negative id are empty slots.
__global__ __launch_bounds__(64) void topk_lists_kernel(float* __restrict__ vals, int64_t* __restrict__ ids, int64_t R, int k,
                                                          const float* __restrict__ ov, const int64_t* __restrict__ oid, int64_t M) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int lane = threadIdx.x;
  WaveTopK st;
  st.k = k;
  st.n = pow2_entries(k);
  st.id = reinterpret_cast<int64_t*>(smem);
  st.v = reinterpret_cast<float*>(smem + (size_t)st.n * 8);
  for (int64_t row = blockIdx.x; row < R; row += gridDim.x) {
    float* gv = vals + row * k;
    int64_t* gid = ids + row * k;
    __syncthreads();
    st.load(gv, gid, lane);
    bool touched = false;
    for (int64_t b = 0; b < M; b += kWave) {
      const int64_t i = b + lane;
      float cv = 0.f;
      int64_t cid = -1;
      if (i < M) cv = ov[row * M + i], cid = oid[row * M + i];
      const bool pass = cid >= 0 && st.passes(f32_order_key(cv), cid);
      if (__ballot(pass) == 0) continue;
      touched = true;
      st.push(pass, cv, cid, lane);
    }
    if (touched) {
      if (st.count) st.flush(lane);
      st.store(gv, gid, lane);
    }
  }
}

__global__ __launch_bounds__(256) void topk_init_kernel(float* __restrict__ vals, int64_t* __restrict__ ids, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    vals[i] = -INFINITY;
    ids[i] = -1;
  }
}

size_t lds_bytes(int64_t k) { return (size_t)pow2_entries((int)k) * 12; }

int64_t wave_grid(int64_t items, int64_t k) {
  int64_t per_cu = (int64_t)(160 * 1024 / lds_bytes(k));  // resident one-wave workgroups per CU
  if (per_cu > 32) per_cu = 32;
  if (per_cu < 1) per_cu = 1;
  return rowseg::wave_grid(items, num_cus(), per_cu);
}

int check_state(const char* fn, int64_t R, int64_t k) {
  SL_REQUIRE(R >= 0, "%s: negative row count", fn);
  SL_REQUIRE(k >= 1 && k <= kMaxK, "%s: k = %lld not in [1, %d]", fn, (long long)k, kMaxK);
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_topk_init(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, void* stream) {
  if (int rc = check_state("sl_topk_init", R, k)) return rc;
  if (R == 0) return 0;
  SL_REQUIRE(d_vals && d_ids, "sl_topk_init: null state");
  const int64_t n = R * k;
  hipLaunchKernelGGL(topk_init_kernel, dim3(stride_grid_256(n)), dim3(256), 0, (hipStream_t)stream, d_vals, d_ids, n);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API size_t sl_topk_merge_ws_bytes(int64_t R, int64_t k, int64_t B) {
  if (R <= 0 || k < 1 || k > kMaxK || B < 1) return 0;
  const int64_t S = rowseg::splits(R, B, num_cus());
  return S > 1 ? (size_t)R * (size_t)S * (size_t)k * 12 + 256 : 0;
}

namespace {

// sl_topk_merge (kBiased false, no bias vectors) and sl_topk_merge_biased: one order of refusals, one launch
template <bool kBiased>
int merge_tile(const char* fn, float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand, int64_t ld, int64_t B,
               int64_t id_base, const float* d_row_bias, const float* d_col_bias, void* d_ws, size_t ws_bytes, void* stream) {
  if (int rc = check_state(fn, R, k)) return rc;
  if (int rc = rowseg::check_tile_shape(fn, B, ld)) return rc;
  SL_REQUIRE(id_base >= 0 && id_base <= kMaxId - B, "%s: ids from id_base = %lld leave [0, 2^62]", fn, (long long)id_base);
  if (R == 0) return 0;
  SL_REQUIRE(d_vals && d_ids, "%s: null state", fn);
  if (int rc = rowseg::check_tile_ptr(fn, d_cand)) return rc;
  if constexpr (kBiased) {
    SL_REQUIRE(d_row_bias && d_col_bias, "%s: null bias vector", fn);
    SL_REQUIRE((((uintptr_t)d_row_bias | (uintptr_t)d_col_bias) & 3) == 0, "%s: a bias vector is not 4-byte aligned", fn);
  }
  const int64_t S = rowseg::splits(R, B, num_cus());
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  if (S == 1) {
    SL_LAUNCH(prof, topk_tile_kernel<kBiased>, dim3((unsigned)wave_grid(R, k)), dim3(64), lds_bytes(k), st, d_vals, d_ids, R, (int)k,
              d_cand, ld, B, id_base, 1, B, (float*)nullptr, (int64_t*)nullptr, d_row_bias, d_col_bias);
    SL_CHECK_HIP(hipGetLastError());
    return 0;
  }
  SL_REQUIRE(d_ws && ws_bytes >= sl_topk_merge_ws_bytes(R, k, B), "%s: workspace too small", fn);
  int64_t* wid = (int64_t*)rowseg::align_ws(d_ws);
  float* wv = (float*)(wid + R * S * k);
  const int64_t seg = rowseg::segment(B, S);
  SL_LAUNCH(prof, topk_tile_kernel<kBiased>, dim3((unsigned)wave_grid(R * S, k)), dim3(64), lds_bytes(k), st, d_vals, d_ids, R,
            (int)k, d_cand, ld, B, id_base, (int)S, seg, wv, wid, d_row_bias, d_col_bias);
  ProfScope fold(SL_PROF_TOPK, st, (double)R * (double)S * (double)k * 12);
  SL_LAUNCH(fold, topk_lists_kernel, dim3((unsigned)wave_grid(R, k)), dim3(64), lds_bytes(k), st, d_vals, d_ids, R, (int)k, wv, wid,
            S * k);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

SL_API int sl_topk_merge(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand, int64_t ld, int64_t B,
                         int64_t id_base, void* d_ws, size_t ws_bytes, void* stream) {
  return merge_tile<false>("sl_topk_merge", d_vals, d_ids, R, k, d_cand, ld, B, id_base, nullptr, nullptr, d_ws, ws_bytes, stream);
}

SL_API int sl_topk_merge_biased(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_cand, int64_t ld, int64_t B,
                                int64_t id_base, const float* d_row_bias, const float* d_col_bias, void* d_ws, size_t ws_bytes,
                                void* stream) {
  return merge_tile<true>("sl_topk_merge_biased", d_vals, d_ids, R, k, d_cand, ld, B, id_base, d_row_bias, d_col_bias, d_ws, ws_bytes,
                          stream);
}

SL_API int sl_topk_merge_states(float* d_vals, int64_t* d_ids, int64_t R, int64_t k, const float* d_other_vals,
                                const int64_t* d_other_ids, int64_t M, void* stream) {
  if (int rc = check_state("sl_topk_merge_states", R, k)) return rc;
  SL_REQUIRE(M >= 0, "sl_topk_merge_states: negative entry count");
  if (R == 0 || M == 0) return 0;
  SL_REQUIRE(d_vals && d_ids, "sl_topk_merge_states: null state");
  SL_REQUIRE(d_other_vals && d_other_ids, "sl_topk_merge_states: null other state");
  hipStream_t st = (hipStream_t)stream;
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)M * 12);
  SL_LAUNCH(prof, topk_lists_kernel, dim3((unsigned)wave_grid(R, k)), dim3(64), lds_bytes(k), st, d_vals, d_ids, R, (int)k,
            d_other_vals, d_other_ids, M);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
