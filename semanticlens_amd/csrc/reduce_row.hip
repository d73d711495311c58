// K1 — fp32 activations with contiguous rows (NCHW): rowreduce (round 1, any row length and alignment), rowreduce_fast (the
// streaming path for the common shapes) and rowreduce_dma<float> (reduce_dma.hpp: inputs of >= 8 MiB), and the ladder that
// picks among them.  Overview of the kernel families: reduce.hip.
#include "reduce_dma.hpp"

namespace sl {
namespace {

// ---- rowreduce: contiguous rows -------------------------------------------------------------
// x: 16-byte aligned, R rows of S floats back to back.  A wave works on a batch of U tasks; a task
// is 64/G consecutive rows covered by one 1-KiB wave-load per step (G lanes per row).
//
// Cost model (HBM-bound: ~13 B/clk/CU at 8 TB/s => one 1-KiB wave-load per ~78 clk per CU):
//  * max: v_max_f32 ignores NaN, torch.amax propagates it.  Instead of testing every element, a
//    running SUM rides along (NaN in => NaN out); only when a row's sum is NaN (a NaN, or +inf and
//    -inf together) the row is re-scanned exactly.  4 max + 4 add per 16-byte piece.
//  * element masks for rows that are not 16-byte aligned (e.g. 7x7 = 49 floats) depend only on the
//    lane when 64/G is a multiple of 4, so they are computed once per kernel.
//  * addressing: wave-uniform 64-bit batch base + 32-bit lane offsets.
// TAIL: total = R*S is not a multiple of 4, so the tensor ends inside a 16-byte piece; the last
// (total & 3) floats are masked out of the vector loads and added by scalar loads to the rows that
// own them (up to three rows when S < 4).
template <int G, int U, int OP, bool TAIL>
__global__ __launch_bounds__(256) void rowreduce_kernel(const float* __restrict__ x, int64_t R, int S, float denom,
                                                         uint16_t* __restrict__ cand, float* __restrict__ outf) {
  constexpr int RPT = kWave / G;
  constexpr bool SUMOP = (OP == OP_SUM || OP == OP_ABSSUM);
  constexpr bool ABS = (OP == OP_ABSMAX || OP == OP_ABSSUM);
  constexpr bool HOIST_H = (RPT % 4 == 0);  // row phase h = (row * S) & 3 depends on the lane only
  const float fill = SUMOP ? 0.f : -__builtin_huge_valf();
  const int lane = threadIdx.x & 63;
  const int li = lane & (G - 1);
  const int g = lane / G;
  const int64_t total = R * (int64_t)S;
  const int64_t total4 = total & ~3ll;  // floats readable as whole 16-byte pieces
  const int64_t nbatch = (R + U * RPT - 1) / (U * RPT);
  // wave-uniform by construction; readfirstlane lets the compiler keep the batch base in SGPRs
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int nsteps = ((S + 6) / 4 + G - 1) / G;  // 16-byte pieces of a row window, per lane
  const int h_lane = (g * S) & 3;

  for (int64_t tb = wave0; tb < nbatch; tb += nwaves) {
    const int64_t row0 = tb * (int64_t)(U * RPT);  // wave-uniform
    const int64_t e_batch = row0 * (int64_t)S;
    const int delta = (int)(e_batch & 3);
    const int64_t a0 = e_batch - delta;
    const float4* __restrict__ A = reinterpret_cast<const float4*>(x + a0);  // wave-uniform, 16-byte aligned
    // last whole piece of the tensor, relative to A: lanes whose piece would start beyond it are
    // clamped onto it; every element they then hold is masked by its row position anyway
    // (a batch that starts at or beyond the last whole piece — always the case for a tensor of fewer than four floats —
    // clamps onto its own first piece: aligned, holds at least one float of the tensor, hence readable; index -1 would
    // be the 16 bytes in front of the tensor)
    const int64_t lim = (total4 - a0) / 4 - 1;
    const int idx_max = lim > 0x7FFFFFFF ? 0x7FFFFFFF : (lim < 0 ? 0 : (int)lim);
    const int64_t rel = total4 - a0;  // floats of whole pieces left from A on
    const int rel_lim = rel > 0x7FFFFFFF ? 0x7FFFFFFF : (int)rel;

    float m[U], sum[U];
    int rs[U];  // row start in elements relative to A
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = fill;
      sum[u] = 0.f;
      rs[u] = delta + (u * RPT + g) * S;
    }

    for (int step = 0; step < nsteps; ++step) {
      const int q = step * G + li;
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = A[min((rs[u] >> 2) + q, idx_max)];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int h = HOIST_H ? h_lane : (rs[u] & 3);
        const int pos0 = q * 4 - h;  // row-local index of v.x (negative in the head piece)
        int lim_s = S;
        if constexpr (TAIL) {  // also drop elements at or beyond the last whole piece of the tensor
          const int left = rel_lim - rs[u];  // row-local index of the first float not covered by whole pieces
          lim_s = left < S ? (left > 0 ? left : 0) : S;
        }
        float e0 = v[u].x, e1 = v[u].y, e2 = v[u].z, e3 = v[u].w;
        if constexpr (ABS) {
          e0 = __builtin_fabsf(e0); e1 = __builtin_fabsf(e1); e2 = __builtin_fabsf(e2); e3 = __builtin_fabsf(e3);
        }
        e0 = (unsigned)(pos0 + 0) < (unsigned)lim_s ? e0 : fill;
        e1 = (unsigned)(pos0 + 1) < (unsigned)lim_s ? e1 : fill;
        e2 = (unsigned)(pos0 + 2) < (unsigned)lim_s ? e2 : fill;
        e3 = (unsigned)(pos0 + 3) < (unsigned)lim_s ? e3 : fill;
        if constexpr (!SUMOP)
          m[u] = __builtin_fmaxf(__builtin_fmaxf(m[u], __builtin_fmaxf(e0, e1)), __builtin_fmaxf(e2, e3));
        sum[u] += (e0 + e1) + (e2 + e3);
      }
    }

#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = row0 + (u * RPT + g);
      const bool row_ok = row < R;
      if constexpr (TAIL) {
        if (row_ok && li == 0 && (row + 1) * (int64_t)S > total4) {  // this row owns floats behind the last whole piece
          const int64_t lo = row * (int64_t)S > total4 ? row * (int64_t)S : total4;
          for (int64_t i = lo; i < (row + 1) * (int64_t)S; ++i) {
            float e = x[i];
            if constexpr (ABS) e = __builtin_fabsf(e);
            if constexpr (!SUMOP) m[u] = __builtin_fmaxf(m[u], e);
            sum[u] += e;
          }
        }
      }
      float r;
      if constexpr (SUMOP) {
        r = group_allreduce_f<G, true>(sum[u]) / denom;  // torch: sum / n (denom = 1: plain sum)
      } else {
        r = group_allreduce_f<G, false>(m[u]);
        const float sred = group_allreduce_f<G, true>(sum[u]);
        if (__builtin_expect(__any(row_ok && sred != sred), 0)) {  // exact re-scan of this lane-group's row
          if (row_has_nan<float, G>(sred, row_ok, x, row, li, S)) r = bits_f32(0x7FC00000u);
        }
      }
      if (li == 0 && row_ok) store_outputs(r, row, cand, outf);
    }
  }
}

// ---- rowreduce_fast: the streaming path for the common shapes -----------------------------------
// Preconditions (checked by the launcher): the row phase h = (row*S)&3 is the same for every row a
// lane ever touches, i.e. S % 4 == 0 (ALIGNED: h = 0, a row is a whole number of 16-byte pieces) or
// 64/G % 4 == 0 with one piece per lane (h = (g*S)&3).  Then
//   * the lane's byte offset inside a task and its four element masks are loop invariant,
//   * the task base is wave-uniform, so every load is `global_load_dwordx4 v, v_off, s[base]`,
//   * ALIGNED rows need no element masks at all: lanes past the row's last piece re-read that piece
//     (max is idempotent; for sums the piece is masked as a whole).
// VALU per 16-byte piece: 2 v_max3 + 4 v_add (+ 4 v_cndmask when rows are unaligned); per row one DPP
// max-reduction (group_allreduce_asm).
template <int G, int U, int OP, bool ALIGNED, int AUX>
__global__ __launch_bounds__(256) void rowreduce_fast_kernel(const float* __restrict__ x, int64_t R, int S, float denom,
                                                              uint16_t* __restrict__ cand,
                                                              float* __restrict__ outf, int64_t tail_from) {
  constexpr int RPT = kWave / G;
  constexpr bool SUMOP = (OP == OP_SUM || OP == OP_ABSSUM);
  constexpr bool ABS = (OP == OP_ABSMAX || OP == OP_ABSSUM);
  const float fill = SUMOP ? 0.f : -__builtin_huge_valf();
  const int lane = threadIdx.x & 63;
  const int li = lane & (G - 1);
  const int g = lane / G;
  const int64_t ntask = R / RPT;  // launcher guarantees R % RPT == 0 and total % 4 == 0
  const int64_t nbatch = (ntask + U - 1) / U;
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t wave0 = (int64_t)blockIdx.x * (blockDim.x >> 6) + wave_in_block;
  const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
  const int npieces = ALIGNED ? S / 4 : (S + 6) / 4;     // pieces of one row window
  const int nsteps = ALIGNED ? (npieces + G - 1) / G : 1;  // unaligned rows: one piece per lane
  const int h = ALIGNED ? 0 : ((g * S) & 3);
  const uint32_t row_byte0 = (uint32_t)(((g * S) >> 2) * 16);  // lane-group's row start inside the task
  const uint32_t task_bytes = (uint32_t)(RPT * S) * 4u;        // multiple of 16
  // element masks of this lane's piece (unaligned rows only; loop invariant)
  const int pos0 = li * 4 - h;
  const bool k0 = (unsigned)(pos0 + 0) < (unsigned)S, k1 = (unsigned)(pos0 + 1) < (unsigned)S;
  const bool k2 = (unsigned)(pos0 + 2) < (unsigned)S, k3 = (unsigned)(pos0 + 3) < (unsigned)S;

  for (int64_t tb = wave0; tb < nbatch; tb += nwaves) {
    const int64_t task0 = tb * U;
    int nu = U;  // tasks that exist in this batch (wave-uniform)
    if (task0 + U > ntask) nu = (int)(ntask - task0);
    // Buffer descriptor over this batch's bytes, built from provably wave-uniform halves of the base
    // pointer so every load is `buffer_load_dwordx4 v, v_off, s[rsrc], s_off offen` (no 64-bit VALU
    // address math, no waterfall loop); the hardware range check makes out-of-batch reads return 0.
    const uint64_t bptr = (uint64_t)(reinterpret_cast<const char*>(x) + task0 * (int64_t)task_bytes);
    const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bptr);
    const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bptr >> 32));
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(((uint64_t)bhi << 32) | blo), 0, (int)((uint32_t)nu * task_bytes), 0x00020000);
    float m[U], sum[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = fill;
      sum[u] = 0.f;
    }
    for (int step = 0; step < nsteps; ++step) {
      const int q = step * G + li;
      uint32_t off;
      bool piece_ok = true;
      if constexpr (ALIGNED) {
        piece_ok = q < npieces;
        off = row_byte0 + (uint32_t)(piece_ok ? q : npieces - 1) * 16u;  // past the row: re-read its last piece
      } else {
        // past the row's window (li >= npieces): clamp onto the window's last piece; all masks are false there
        off = row_byte0 + (uint32_t)(li < npieces ? li : npieces - 1) * 16u;
      }
      float4 v[U];
      // batches from `tail_from` on (the part of a just-produced input that is still in the Infinity Cache) are read
      // with the default policy, the rest (already evicted to HBM) with the streaming one; wave-uniform choice
      if (AUX != 0 && __builtin_amdgcn_readfirstlane((int)(tb >= tail_from))) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, (int)((uint32_t)u * task_bytes), 0);
          v[u] = make_float4(bits_f32(w[0]), bits_f32(w[1]), bits_f32(w[2]), bits_f32(w[3]));
        }
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)off, (int)((uint32_t)u * task_bytes), AUX);
          v[u] = make_float4(bits_f32(w[0]), bits_f32(w[1]), bits_f32(w[2]), bits_f32(w[3]));
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float e0 = v[u].x, e1 = v[u].y, e2 = v[u].z, e3 = v[u].w;
        if constexpr (ABS) {
          e0 = __builtin_fabsf(e0); e1 = __builtin_fabsf(e1); e2 = __builtin_fabsf(e2); e3 = __builtin_fabsf(e3);
        }
        if constexpr (!ALIGNED) {
          e0 = k0 ? e0 : fill; e1 = k1 ? e1 : fill; e2 = k2 ? e2 : fill; e3 = k3 ? e3 : fill;
        }
        if constexpr (SUMOP) {
          float ps = (e0 + e1) + (e2 + e3);
          if constexpr (ALIGNED) ps = piece_ok ? ps : 0.f;
          sum[u] += ps;
        } else {
          m[u] = v_max3(v_max3(m[u], e0, e1), e2, e3);
          sum[u] += (e0 + e1) + (e2 + e3);  // NaN detector only
        }
      }
    }
    float r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (SUMOP) {
        r[u] = group_allreduce_asm<G, true>(sum[u]) / denom;  // torch: sum / n (denom = 1: plain sum)
      } else {
        r[u] = group_allreduce_asm<G, false>(m[u]);
        // any lane of the wave saw a NaN sum (a NaN, or +inf and -inf)?  Rare: re-scan those rows exactly.
        const bool row_ok = u < nu;
        if (__builtin_expect(__any(row_ok && sum[u] != sum[u]), 0)) {
          const int64_t row = (task0 + u) * RPT + g;
          if (row_has_nan<float, G>(group_allreduce_f<G, true>(sum[u]), row_ok, x, row, li, S)) r[u] = bits_f32(0x7FC00000u);
        }
      }
    }
    // After the all-reduce every lane of a group holds its row's result for each u.  Lane li of group g
    // keeps r[p + li] and stores it: one masked store instruction per G tasks instead of one per task.
#pragma unroll
    for (int p = 0; p < U; p += G) {
      float sel = r[p];
#pragma unroll
      for (int u = p + 1; u < U && u < p + G; ++u) sel = (li == u - p) ? r[u] : sel;
      const int uu = p + li;
      if (li < G && uu < nu) store_outputs(sel, (task0 + uu) * RPT + g, cand, outf);
    }
  }
}

template <int G, int U, int OP>
void launch_rowreduce(const ReduceCall& c, const float* x, int64_t R, int S) {
  constexpr int RPT = kWave / G;
  const int64_t ntasks = (R + RPT - 1) / RPT;
  const int64_t nbatch = (ntasks + U - 1) / U;
  const unsigned blocks = grid_blocks((nbatch + 3) / 4, 8);
  if ((R * (int64_t)S) % 4 == 0)
    SL_LAUNCH(c.prof, (rowreduce_kernel<G, U, OP, false>), dim3(blocks), dim3(256), 0, c.st, x, R, S, c.denom, c.cand, c.outf);
  else
    SL_LAUNCH(c.prof, (rowreduce_kernel<G, U, OP, true>), dim3(blocks), dim3(256), 0, c.st, x, R, S, c.denom, c.cand, c.outf);
}

template <int G, int U, int OP, bool ALIGNED>
void launch_rowreduce_fast(const ReduceCall& c, const float* x, int64_t R, int S) {
  constexpr int RPT = kWave / G;
  const int64_t nbatch = (R / RPT + U - 1) / U;
  const unsigned blocks = grid_blocks((nbatch + 3) / 4, 8);
  const int64_t bytes = R * (int64_t)S * 4;
  // cache policy in batches; inputs below nt_min_bytes take the instance whose every load has the default policy
  if (nt_policy_applies(c.policy, bytes)) {
    const int64_t tail_from = nt_head_units(c.policy, bytes, (int64_t)U * RPT * S * 4);
    SL_LAUNCH(c.prof, (rowreduce_fast_kernel<G, U, OP, ALIGNED, kLoadAux>), dim3(blocks), dim3(256), 0, c.st, x, R, S, c.denom, c.cand, c.outf,
              tail_from);
  } else {
    SL_LAUNCH(c.prof, (rowreduce_fast_kernel<G, U, OP, ALIGNED, 0>), dim3(blocks), dim3(256), 0, c.st, x, R, S, c.denom, c.cand, c.outf,
              (int64_t)INT64_MAX);
  }
}

// Every site's U set follows from the guards that lead to it; with S % 4 == 0 a row is np = S / 4 pieces and a task of
// 64 / G rows is 1024 * np / G bytes.  The size conditions of try_rowreduce_dma (>= 8 MiB, R < 2^31) do not depend on G: a
// site reached because an earlier site failed on them fails on them too.
template <int OP>
int dispatch_rowreduce_t(const ReduceCall& c, const float* x, int64_t R, int S) {
  // pieces needed for a row window: up to (S + 6) / 4
  const int need = (S + 6) / 4;
#define SL_TRY_DMA(G_, AL_, MULTI_, UMASK_)                                                                                     \
  do {                                                                                                                          \
    const int t_ = try_rowreduce_dma<G_, OP, AL_, float, MULTI_, UMASK_>("fp32 G=" #G_ " aligned=" #AL_ " multi=" #MULTI_, c, x, R, S); \
    if (t_) return t_ < 0 ? t_ : 0;                                                                                             \
  } while (0)
#define SL_ROWREDUCE(G_, U_, AL_, UMASK_)                                            \
  do {                                                                               \
    SL_TRY_DMA(G_, AL_, false, UMASK_);                                              \
    launch_rowreduce_fast<G_, U_, OP, AL_>(c, x, R, S);                              \
    return 0;                                                                        \
  } while (0)
  // fast path A: rows are whole 16-byte pieces
  if (S % 4 == 0 && S >= 16 && (int64_t)S * 64 * 4 * 8 < (1ll << 31)) {
    const int np = S / 4;  // >= 4
    // Rows longer than an LDS-DMA batch (> 4 KiB: 56 x 56 maps and larger) stay on rowreduce_fast<64, 4>: 6.5 TB/s cold AND behind
    // a producer on (256, 192, 56, 56) (617 MB, 0.82 of spec).  Round 4 built a ping-pong stream kernel for them (a wave walks
    // (row, block-of-4-loads) items, the next item issued before the current one is reduced): 6.1 cold / 4.6 behind a producer in
    // fp32, 5.4 against rowreduce_h's 6.1-6.3 in fp16 — removed (tools/k1_long_rows.py, profiles/r04_k1_long_rows.txt).
    // LDS-DMA path: lanes read from LDS, where clamped lanes are free, so four rows share a task (G = 16, up to four
    // steps per row) and their DPP reductions run in the same instructions
    // task = 64 np bytes, np in 5..64: 320 B .. 4 KiB, so U = min(4, 64 / np) takes every value 1..4
    if (np > 4 && np <= 64 && R % 4 == 0) SL_TRY_DMA(16, true, false, kDmaUAll);
    // np = 4 only (S >= 16): a task is exactly 1 KiB, U = 4
    if (np <= 4 && R % 16 == 0) SL_ROWREDUCE(4, 8, true, kDmaU4);
    // np in 5..8 with R % 8 == 0 was offered to G = 16 above and failed on size; what is left is np = 4: 512 B, U = 4
    if (np <= 8 && R % 8 == 0) SL_ROWREDUCE(8, 8, true, kDmaU4);
    // the same G as the first site, which np > 4 already failed: np = 4 is left, 256 B, U = 4 (np 5..16 would give U = 4 too)
    if (np <= 16 && R % 4 == 0) SL_ROWREDUCE(16, 8, true, kDmaU4);
    // R % 4 == 2 (multiples of four went above): task = 32 np bytes, np in 4..32: 128 B .. 1 KiB, U = 4
    if (np <= 32 && R % 2 == 0) SL_ROWREDUCE(32, 8, true, kDmaU4);
    // task = one row = 16 np bytes, np in 4..64: 64 B .. 1 KiB, U = 4
    if (np <= 64) SL_ROWREDUCE(64, 8, true, kDmaU4);
    // np > 64: a row of more than 1 KiB, U = 256 / np is 3, 2 or 1 (np > 256: too long for a batch, rowreduce_fast)
    SL_ROWREDUCE(64, 4, true, kDmaU1 | kDmaU2 | kDmaU3);
  }
  // fast path B: short unaligned rows (e.g. 7x7 = 49 floats), >= 4 rows per wave-load
  if (S % 4 != 0 && need <= 16) {
    // need <= 4: S <= 13, task = 64 S <= 832 B, U = 4
    if (need <= 4 && R % 16 == 0) SL_ROWREDUCE(4, 8, false, kDmaU4);
    // need <= 8: S <= 29, task = 32 S <= 928 B, U = 4
    if (need <= 8 && R % 8 == 0) SL_ROWREDUCE(8, 8, false, kDmaU4);
    // need <= 16: S <= 61, task = 16 S <= 976 B, U = 4
    if (R % 4 == 0) SL_ROWREDUCE(16, 8, false, kDmaU4);
  }
#undef SL_ROWREDUCE
  // longer unaligned rows whose tasks still fit an LDS-DMA batch (<= 4 KiB): two rows per task when S is even (S <= 512),
  // four otherwise (S <= 256: 13 x 13, 15 x 15 maps); the lanes walk a row's window in steps
  if (S % 4 != 0 && need > 16) {
    // S even, 126 <= S <= 510: task = 8 S bytes, 1008 B .. 4 KiB, U = 2 up to S = 256 and 1 beyond
    if (S % 2 == 0 && need > 32) SL_TRY_DMA(32, false, true, kDmaU1 | kDmaU2);
    // 62 <= S <= 255: task = 16 S bytes, 992 B .. 4 KiB, U = 2 up to S = 128 and 1 beyond
    SL_TRY_DMA(16, false, true, kDmaU1 | kDmaU2);
  }
#undef SL_TRY_DMA
  // Longer unaligned fp32 rows stay on the round-1 kernel (0.58-0.72 of spec cold).  Tried and dropped in round 3: reading
  // each row from its own 4-byte-aligned start with unaligned 16-byte loads (legal on this part:
  // tools/native/unaligned_probe.hip) — 17 x 17 4.7 -> 4.4 TB/s, 27 x 27 5.8 -> 5.4, 111 x 111 4.95 -> 5.26.
  // Every rung is reachable (rows that do not group into tasks, small inputs): S = 0..12 take G = 4, longer unaligned rows
  // the rung of their window, S >= 2^20 the last one.
  if (need <= 4) launch_rowreduce<4, 8, OP>(c, x, R, S);
  else if (need <= 8) launch_rowreduce<8, 8, OP>(c, x, R, S);
  else if (need <= 16) launch_rowreduce<16, 8, OP>(c, x, R, S);
  else if (need <= 32) launch_rowreduce<32, 8, OP>(c, x, R, S);
  else if (need <= 64) launch_rowreduce<64, 8, OP>(c, x, R, S);
  else launch_rowreduce<64, 4, OP>(c, x, R, S);
  return 0;
}

}  // namespace

int dispatch_rowreduce(int op, const ReduceCall& c, const float* x, int64_t R, int S) {
  SL_SWITCH_OP(op, return dispatch_rowreduce_t<OP>(c, x, R, S));
  return bad_reduce_op("dispatch_rowreduce", op);
}

}  // namespace sl
