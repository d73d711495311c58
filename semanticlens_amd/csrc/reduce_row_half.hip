// K1 — fp16 / bf16 activations with contiguous rows (NCHW activations of half-precision models): rowreduce_h (VGPR loads)
// and rowreduce_dma<_Float16 / uint16_t> (reduce_dma.hpp: inputs of >= 8 MiB), and the ladder that picks between them.
// Element tags are _Float16 and uint16_t (bf16 bits).  Overview of the kernel families: reduce.hip.
#include "reduce_dma.hpp"

namespace sl {
namespace {

// ---- rowreduce_h: contiguous rows of 2-byte elements (NCHW activations of fp16 / bf16 models) -------------------------
// x 16-byte aligned, R rows of S elements back to back.  G lanes per row (64 / G rows = one *set* per wave pass); a lane
// loads 16-byte pieces (8 elements) of its row's window, converts to fp32 and masks the elements that belong to the
// neighbouring rows (rows start on 2-byte boundaries).  An aligned 16-byte piece that holds at least one valid byte never
// crosses a page, so the window's first and last piece are safe to read whole.  U sets x J pieces per lane are in flight
// before any is reduced (short rows would otherwise keep < 1 KB per wave in flight).  max: v_max_f32 drops NaN, so a
// running sum rides along as the NaN detector and a row whose sum is NaN is re-scanned exactly (as in the fp32 kernels).
// Same cache policy and tail-first walk as the fp32 kernels; sums accumulate in fp32 and are rounded to the activation
// dtype once, like torch's.
template <typename T, int G, int U, int J, int OP, bool ALIGNED>
__global__ __launch_bounds__(256) void rowreduce_h_kernel(const T* __restrict__ x, int64_t R, int S, float denom, int64_t tail_from,
                                                           uint16_t* __restrict__ cand, float* __restrict__ outf) {
  constexpr int RPW = kWave / G;
  constexpr bool SUMOP = (OP == OP_SUM || OP == OP_ABSSUM);
  constexpr bool ABS = (OP == OP_ABSMAX || OP == OP_ABSSUM);
  const float fill = SUMOP ? 0.f : -__builtin_huge_valf();
  // the same value as a pair of raw elements (-inf is 0xFF80 in bf16, 0xFC00 in fp16).  The aligned path takes |.| of
  // whole pieces, fill included, so absmax fills with +0 (|x| >= 0 makes it neutral; |-inf| would be +inf).
  const uint32_t fillw = (SUMOP || ABS) ? 0u : (std::is_same<T, uint16_t>::value ? 0xFF80FF80u : 0xFC00FC00u);
  const int lane = threadIdx.x & 63;
  const int li = lane & (G - 1);
  const int g = lane / G;
  const int64_t nsets = (R + RPW - 1) / RPW;
  const int64_t nbatch = (nsets + U - 1) / U;  // a batch = U consecutive sets
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int64_t rot = (tail_from > 0 && tail_from < nbatch) ? tail_from : 0;
  const int np_max = ALIGNED ? S / 8 : (S + 14) / 8;  // pieces a row's window can touch
  const u32x4* xp = reinterpret_cast<const u32x4*>(x);
  for (int64_t bi = wave0; bi < nbatch; bi += nwaves) {
    int64_t batch = bi + rot;
    if (batch >= nbatch) batch -= nbatch;
    int64_t row[U];
    int h[U], np[U];
    const u32x4* rp[U];
    float m[U], sum[U];
    f32x2 sum2[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      row[u] = (batch * U + u) * RPW + g;
      const bool ok = row[u] < R;
      const int64_t e0 = (ok ? row[u] : 0) * (int64_t)S;
      h[u] = ALIGNED ? 0 : (int)(e0 & 7);
      np[u] = ok ? (h[u] + S + 7) >> 3 : 0;
      rp[u] = xp + (e0 >> 3);
      m[u] = fill;
      sum[u] = 0.f;
      sum2[u] = f32x2{0.f, 0.f};
    }
    auto walk = [&](auto NT) __attribute__((always_inline)) {
      constexpr bool nt = decltype(NT)::value;
      for (int q0 = 0; q0 < np_max; q0 += J * G) {
        u32x4 w[U][J];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const int q = q0 + j * G + li;
            w[u][j] = u32x4{fillw, fillw, fillw, fillw};  // lanes without a piece contribute the fill value
            if (q < np[u]) {
              if constexpr (nt) w[u][j] = __builtin_nontemporal_load(rp[u] + q);
              else w[u][j] = rp[u][q];
            }
          }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int j = 0; j < J; ++j) {
            const int q = q0 + j * G + li;
            const bool in = q < np[u];
            const int idx0 = q * 8 - h[u];  // row-relative index of the piece's first element
#pragma unroll
            for (int d = 0; d < 4; ++d) {
              // word by word on purpose, not decode_piece: decoding the whole piece first costs this kernel 2-7 VGPRs
              float e[2];
              unpack2<T>(w[u][j][d], e[0], e[1]);
              if constexpr (ALIGNED) {  // whole pieces: two elements per v_max3 / v_pk_add
                if constexpr (ABS) {
                  e[0] = __builtin_fabsf(e[0]);
                  e[1] = __builtin_fabsf(e[1]);
                }
                if constexpr (!SUMOP) m[u] = v_max3(m[u], e[0], e[1]);
                sum2[u] += f32x2{e[0], e[1]};  // the sum, or the NaN detector of the max
              } else {
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                  float v = ABS ? __builtin_fabsf(e[k]) : e[k];
                  const bool valid = in && (unsigned)(idx0 + 2 * d + k) < (unsigned)S;
                  v = valid ? v : fill;
                  if constexpr (!SUMOP) m[u] = __builtin_fmaxf(m[u], v);
                  sum[u] += v;  // the sum, or the NaN detector of the max
                }
              }
            }
          }
      }
    };
    if (batch < tail_from) walk(std::true_type());
    else walk(std::false_type());
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool ok = row[u] < R;
      if constexpr (ALIGNED) sum[u] = sum2[u][0] + sum2[u][1];
      float r;
      if constexpr (SUMOP) {
        r = group_allreduce_f<G, true>(sum[u]);
      } else {
        r = group_allreduce_f<G, false>(m[u]);
        if (__builtin_expect(__any(ok && sum[u] != sum[u]), 0)) {  // a NaN, or +inf and -inf (or fill) together: look again
          if (row_has_nan<T, G>(group_allreduce_f<G, true>(sum[u]), ok, x, row[u], li, S)) r = bits_f32(0x7FC00000u);
        }
      }
      r = round_to_dtype<T>(finish<OP>(r, denom));
      if (li == 0 && ok) store_outputs(r, row[u], cand, outf);
    }
  }
}

template <typename T, int G, int U, int J, int OP, bool ALIGNED>
void launch_rowreduce_h(const ReduceCall& c, const T* x, int64_t R, int S) {
  constexpr int RPW = kWave / G;
  const int64_t nsets = (R + RPW - 1) / RPW;
  const int64_t nbatch = (nsets + U - 1) / U;
  const unsigned blocks = grid_blocks((nbatch + 3) / 4, 8);
  const int64_t tail_from = nt_head_units(c.policy, R * (int64_t)S * 2, (int64_t)U * RPW * S * 2);  // in batches
  SL_LAUNCH(c.prof, (rowreduce_h_kernel<T, G, U, J, OP, ALIGNED>), dim3(blocks), dim3(256), 0, c.st, x, R, S, c.denom, tail_from,
            c.cand, c.outf);
}

// G = lanes per row: the smallest power of two that covers the pieces of a row's window (at most 64: longer rows loop)
template <typename T, int OP>
int dispatch_rowreduce_h_t(const ReduceCall& c, const T* x, int64_t R, int S) {
  const bool al = S % 8 == 0;
  const int np = al ? S / 8 : (S + 14) / 8;
  // LDS-DMA ring kernel first (rowreduce_dma_kernel<T>: the fp32 kernel's feed with 8-element pieces); it takes inputs of
  // >= 8 MB whose tasks (64 / G rows) are whole 16-byte pieces
  // Each site's U set follows from its guards (a task of 64 / G rows is 128 S / G bytes).  The size conditions of
  // try_rowreduce_dma do not depend on G, so a site reached because an earlier one failed on them fails on them too.
#define SL_TRY_DMA(G_, AL_, MULTI_, UMASK_)                                                                                  \
  do {                                                                                                                       \
    const int t_ = try_rowreduce_dma<G_, OP, AL_, T, MULTI_, UMASK_>("half G=" #G_ " aligned=" #AL_ " multi=" #MULTI_, c, x, R, S); \
    if (t_) return t_ < 0 ? t_ : 0;                                                                                          \
  } while (0)
  if (al) {
    // task = 64 np bytes, np in 5..64: 320 B .. 4 KiB, so U = min(4, 64 / np) takes every value 1..4
    if (np > 4 && np <= 64) SL_TRY_DMA(16, true, false, kDmaUAll);
    // task = 256 np bytes, np in 1..4: 256 B .. 1 KiB, U = 4
    if (np <= 4) SL_TRY_DMA(4, true, false, kDmaU4);
    // task = one row = 16 np bytes, np in 65..256: more than 1 KiB up to 4 KiB, U = 256 / np is 3, 2 or 1
    if (np > 64) SL_TRY_DMA(64, true, false, kDmaU1 | kDmaU2 | kDmaU3);
  } else {
    // one piece per lane: np <= 4: S <= 25, task = 32 S <= 800 B; np <= 8: S <= 57, 16 S <= 912 B; np <= 16: S <= 121,
    // 8 S <= 968 B; np <= 32: S <= 249, 4 S <= 996 B — every task below 1 KiB, U = 4
    if (np <= 4) SL_TRY_DMA(4, false, false, kDmaU4);
    if (np <= 8) SL_TRY_DMA(8, false, false, kDmaU4);
    if (np <= 16) SL_TRY_DMA(16, false, false, kDmaU4);
    if (np <= 32) SL_TRY_DMA(32, false, false, kDmaU4);
    // windows longer than a task's lanes, or rows whose short tasks are not whole pieces: walk the window in steps with the
    // fewest rows per task that make it whole (2 rows when S % 4 == 0: S <= 1024; 4 when S is even: S <= 512; else 8: S <= 256)
    // Each is reached with windows longer than the single-step sites cover (S >= 252 / 122 / 59): tasks of 4 S / 8 S / 16 S
    // bytes run from ~1 KiB to the 16 KiB limit, so U = 2, U = 1 and the sixteen-instruction form all occur
    if (S % 4 == 0) SL_TRY_DMA(32, false, true, kDmaU1 | kDmaU2 | kDmaU16K);
    if (S % 2 == 0) SL_TRY_DMA(16, false, true, kDmaU1 | kDmaU2 | kDmaU16K);
    SL_TRY_DMA(8, false, true, kDmaU1 | kDmaU2 | kDmaU16K);
  }
#undef SL_TRY_DMA
  // every rung below is reachable, aligned or not (small inputs; np = 1 is S = 8, or S = 1 unaligned)
#define SL_ROWH(G, U, J)                                                                          \
  do {                                                                                            \
    if (al) launch_rowreduce_h<T, G, U, J, OP, true>(c, x, R, S);                                \
    else launch_rowreduce_h<T, G, U, J, OP, false>(c, x, R, S);                                  \
    return 0;                                                                                     \
  } while (0)
  if (np <= 1) SL_ROWH(1, 4, 1);
  if (np <= 2) SL_ROWH(2, 4, 1);
  if (np <= 4) SL_ROWH(4, 4, 1);
  if (np <= 8) SL_ROWH(8, 4, 1);
  if (np <= 16) SL_ROWH(16, 4, 1);
  if (np <= 32) SL_ROWH(32, 4, 1);
  if (np <= 64) SL_ROWH(64, 4, 1);
  SL_ROWH(64, 2, 2);
#undef SL_ROWH
}

}  // namespace

int dispatch_rowreduce_h(int op, int dtype, const ReduceCall& c, const void* x, int64_t R, int S) {
  if (dtype == SL_F16) {
    SL_SWITCH_OP(op, return (dispatch_rowreduce_h_t<_Float16, OP>(c, (const _Float16*)x, R, S)));
  } else {
    SL_SWITCH_OP(op, return (dispatch_rowreduce_h_t<uint16_t, OP>(c, (const uint16_t*)x, R, S)));
  }
  return bad_reduce_op("dispatch_rowreduce_h", op);
}

}  // namespace sl
