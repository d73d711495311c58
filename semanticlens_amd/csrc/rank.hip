// K26 — where given (value, id) keys stand in a row of cosine tiles: the count behind label_rank / probe_rank (lens.py).
//
// State per row: T int64 counts, one per key slot.  One launch adds, for every slot with a key id >= 0, the number of columns of a
// row-major candidate tile (R,B), read exactly as topk_tile_kernel reads one, that order before the slot's key.  The order, the
// exclusion of the key's own column and their 32-bit column form are rank_order.hpp's; nothing here restates them.
//
// Shape of the work: one wavefront (a 64-thread workgroup) owns a row segment and walks it in chunks of 1024 columns, 16 per
// lane in four 16-byte loads.  A chunk that lies wholly inside the segment (a wave-uniform test) issues its four loads together
// and converts afterwards; a segment's first and last chunk guard every piece.  A row's keys are wave-uniform: the order key
// of each value and its id live in scalar registers.  Per chunk and slot, scalar code places the key's column relative to the
// chunk (before / inside / after).  Outside
// the one chunk that holds the key's column the rule collapses to one unsigned threshold for the whole chunk, so an element costs
// one order-key conversion plus, per slot, one compare and one add into the lane's 32-bit chunk counter; that counter (at most
// 16) is added to the lane's 64-bit total once per chunk.  A column outside the tile gets the key 0, which is above no threshold.
// At the end of the segment the lanes' totals are added across the wave and lane 0 adds them to the row's counts.
//
// Few rows of very many columns: the columns are split over S waves per row (the rule K17 uses), and the S partial counts go into
// the row's counts with 64-bit integer atomic adds.  Integer addition is associative and commutative: the counts after a sequence
// of merges do not depend on the cut into tiles, their order or the scheduling.  No workspace, no second launch.
#include "rank_order.hpp"
#include "rowseg_tile.hpp"

namespace sl {
namespace {

using rowseg::kChunk;
constexpr int kMaxTargets = SL_RANK_MAX_TARGETS;

// One wave per (row, split): columns [s*seg, (s+1)*seg) of the row.  TP: the slots the kernel is built for (1, 4 or 16: more
// slots are more registers and fewer waves per SIMD), T <= TP the slots a row has; the slots from T on are treated as unused, and
// an unused slot is skipped by a wave-uniform branch.
template <int TP>
__global__ __launch_bounds__(64) void rank_tile_kernel(int64_t* __restrict__ counts, int64_t R, int T, const float* __restrict__ cand,
                                                         int64_t ld, int64_t B, int64_t id_base, const float* __restrict__ key_vals,
                                                         const int64_t* __restrict__ key_ids, int S, int64_t seg) {
  const int lane = threadIdx.x;
  for (int64_t w = blockIdx.x; w < R * S; w += gridDim.x) {
    const auto [row, s, lo, hi] = rowseg::item(w, S, seg, B);
    const float* rowp = cand + row * ld;
    uint32_t key[TP];
    int64_t kid[TP];
    uint64_t total[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      kid[t] = t < T ? key_ids[row * T + t] : -1;
      key[t] = t < T ? f32_order_key(key_vals[row * T + t]) : 0u;
      total[t] = 0;
    }
    for (int64_t base = rowseg::chunk_start((uintptr_t)(rowp + lo), lo); base < hi; base += kChunk) {
      uint32_t ck[4][4];
      if (base >= lo && base + kChunk <= hi) {  // wave-uniform: the whole chunk lies inside, four loads in flight at once
        f4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = *reinterpret_cast<const f4*>(rowp + base + (u * kWave + lane) * 4);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int j = 0; j < 4; ++j) ck[u][j] = f32_order_key(x[u][j]);
      } else {  // a segment's first or last chunk: rowseg::load_chunk's guards, spelled out (rowseg_tile.hpp says why)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int64_t c = base + (int64_t)(u * kWave + lane) * 4;
          if (c >= lo && c + 4 <= hi) {
            const f4 x = *reinterpret_cast<const f4*>(rowp + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) ck[u][j] = f32_order_key(x[j]);
          } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) ck[u][j] = (c + j >= lo && c + j < hi) ? f32_order_key(rowp[c + j]) : 0u;  // counts nowhere
          }
        }
      }
#pragma unroll
      for (int t = 0; t < TP; ++t) {
        if (kid[t] < 0) continue;  // wave-uniform
        const int32_t kc = rank_order::key_column(kid[t], id_base + base, kChunk);
        uint32_t n = 0;
        if (kc < 0 || kc >= kChunk) {  // the key's column is not in this chunk: one threshold for all of it
          const uint32_t thr = rank_order::threshold(key[t], kc >= kChunk);
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j) n += ck[u][j] > thr ? 1u : 0u;
        } else {
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              n += rank_order::column_orders_before(ck[u][j], (u * kWave + lane) * 4 + j, key[t], kc) ? 1u : 0u;
        }
        total[t] += n;
      }
    }
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      if (kid[t] < 0) continue;
      uint64_t v = total[t];
#pragma unroll
      for (int d = kWave / 2; d > 0; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d, kWave);
      if (lane == 0 && v != 0) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(counts + row * T + t);
        if (S == 1)
          *dst += v;  // the row's only wave in this launch
        else
          atomicAdd(dst, (unsigned long long)v);
      }
    }
  }
}

template <int TP>
void launch(ProfScope& prof, hipStream_t st, int64_t items, int64_t* counts, int64_t R, int T, const float* cand, int64_t ld, int64_t B,
            int64_t id_base, const float* key_vals, const int64_t* key_ids, int S, int64_t seg) {
  SL_LAUNCH(prof, rank_tile_kernel<TP>, dim3((unsigned)rowseg::wave_grid(items, num_cus(), 32)), dim3(64), 0, st, counts, R, T, cand, ld, B, id_base, key_vals,
            key_ids, S, seg);
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int64_t sl_rank_merge_splits(int64_t R, int64_t B) { return R <= 0 || B < 1 ? 1 : rowseg::splits(R, B, num_cus()); }

SL_API int sl_rank_merge(int64_t* d_counts, int64_t R, int64_t T, const float* d_cand, int64_t ld, int64_t B, int64_t id_base,
                         const float* d_key_vals, const int64_t* d_key_ids, void* stream) {
  SL_REQUIRE(R >= 0, "sl_rank_merge: negative row count");
  SL_REQUIRE(T >= 1 && T <= kMaxTargets, "sl_rank_merge: T = %lld not in [1, %d]", (long long)T, kMaxTargets);
  if (int rc = rowseg::check_tile_shape("sl_rank_merge", B, ld)) return rc;
  SL_REQUIRE(id_base >= 0 && id_base <= (1ll << 62), "sl_rank_merge: id_base %lld outside [0, 2^62]", (long long)id_base);
  if (R == 0) return 0;
  SL_REQUIRE(d_counts && d_cand && d_key_vals && d_key_ids, "sl_rank_merge: null counts, candidate tile or keys");
  SL_REQUIRE(((uintptr_t)d_counts & 7) == 0 && ((uintptr_t)d_key_ids & 7) == 0, "sl_rank_merge: counts or key ids are not 8-byte aligned");
  SL_REQUIRE(((uintptr_t)d_cand & 3) == 0 && ((uintptr_t)d_key_vals & 3) == 0, "sl_rank_merge: candidate tile or key values are not 4-byte aligned");
  const int64_t S = rowseg::splits(R, B, num_cus());
  if (int rc = rowseg::check_items("sl_rank_merge", R, S)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t seg = rowseg::segment(B, S);
  ProfScope prof(SL_PROF_TOPK, st, (double)R * (double)B * 4);
  const int t = (int)T;
  if (t == 1)
    launch<1>(prof, st, R * S, d_counts, R, t, d_cand, ld, B, id_base, d_key_vals, d_key_ids, (int)S, seg);
  else if (t <= 4)
    launch<4>(prof, st, R * S, d_counts, R, t, d_cand, ld, B, id_base, d_key_vals, d_key_ids, (int)S, seg);
  else
    launch<16>(prof, st, R * S, d_counts, R, t, d_cand, ld, B, id_base, d_key_vals, d_key_ids, (int)S, seg);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
