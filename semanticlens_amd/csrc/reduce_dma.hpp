// K1 — rowreduce_dma: the LDS-DMA ring kernel of contiguous rows, for fp32 (reduce_row.hip) and for fp16 / bf16
// (reduce_row_half.hip).  Included by those two units only.
#pragma once
#include "reduce_common.hpp"

namespace sl {
namespace {

// ---- rowreduce_dma: the same row arithmetic fed through a wave-private LDS ring ----------------------------------
// rowreduce_fast maps G lanes onto a row and loads the row's 16-byte pieces straight into VGPRs, so a row of 49 (196, 784)
// floats keeps 13 of 16 (49 of 64, 196 of 256) load lanes busy: ~23 % of every wave-load re-reads a clamped piece, and a
// cold 103-411 MB input streamed at 5.4-6.1 TB/s.  Here the global side is decoupled from the row structure:
//   * a *batch* (U tasks = U * 64 / G rows, <= 4 KiB, contiguous in memory) is fetched by up to four LDS-DMA
//     instructions (global_load_lds_dwordx4, nt): 64 lanes x 16 consecutive bytes each, every lane useful, lanes past
//     the batch masked off;
//   * each wave owns TWO slots of exactly one batch each (dynamic LDS: 8 slots + 1 KiB per workgroup), which lets 5-8
//     workgroups = 20-32 waves share a CU: one batch is in flight while one is reduced; counted `s_waitcnt vmcnt`; no
//     barrier, the wave reads only what it fetched itself.  (tools/native/stream_lab.hip: a bare read-once stream
//     reaches 6.6-6.85 TB/s through LDS-DMA, 6.5-6.7 through VGPR loads; occupancy, not ring depth, is what this
//     kernel responds to: 12 waves x 3 slots 6.06 / 5.50 TB/s on the 411 / 206 MB inputs, 24 waves x 2 slots 6.37 / 5.88);
//   * lanes then read their row's pieces with ds_read_b128 from the slot — masked / clamped lanes cost LDS bandwidth,
//     of which the kernel uses ~10 %.
// Arithmetic, NaN handling, rounding and the output packing are those of rowreduce_fast.
constexpr int kDmaMaxBatch = 4096;  // bytes: four 1-KiB LDS-DMA instructions
constexpr int kDmaDepth = 2;        // slots per wave: one batch in flight while one is reduced
constexpr int kDmaLdsPerCu = 160 * 1024;

// T = float, _Float16 or uint16_t (bf16 bits): a 16-byte piece holds EPP = 4 or 8 elements; 2-byte rows start on any
// 2-byte boundary, so the element masks of an unaligned row cover eight positions instead of four (round 3: fp16 / bf16
// NCHW activations took rowreduce_h's VGPR loads, 3.5-3.7 TB/s at 14 x 14 and 7 x 7).
// MULTI (unaligned rows only): a row's window has more pieces than its G lanes — odd maps of 13 x 13 .. 15 x 15 (fp32, four
// rows per task) or up to 30 x 30 (fp16 with S % 4 == 0, two rows per task): the lanes walk the window in steps of G pieces
// and the element masks are recomputed per step (only a window's first and last piece are partial).
// NI = 1-KiB LDS-DMA instructions per batch: 4, or 16 for MULTI tasks of 4-16 KiB (17 x 17 .. 31 x 31 maps), one per batch.
template <typename T, int G, int U, int OP, bool ALIGNED, bool MULTI = false, int NI = kDmaMaxBatch / 1024>
__global__ __launch_bounds__(256) void rowreduce_dma_kernel(const T* __restrict__ x, int64_t R, int S, float denom, int slot_bytes,
                                                             int64_t tail_from, uint16_t* __restrict__ cand,
                                                             float* __restrict__ outf) {
  constexpr int RPT = kWave / G;
  constexpr int EPP = 16 / (int)sizeof(T);  // elements per 16-byte piece
  constexpr bool SUMOP = (OP == OP_SUM || OP == OP_ABSSUM);
  constexpr bool ABS = (OP == OP_ABSMAX || OP == OP_ABSSUM);
  extern __shared__ __align__(1024) unsigned char smem[];  // 4 waves x kDmaDepth slots of `slot_bytes` + 1 KiB (masked tail)
  const float fill = SUMOP ? 0.f : -__builtin_huge_valf();
  const int lane = threadIdx.x & 63;
  const int li = lane & (G - 1);
  const int g = lane / G;
  const int64_t ntask = R / RPT;  // launcher guarantees R % RPT == 0
  const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t wave0 = (int64_t)blockIdx.x * 4 + wave_in_block;
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  static_assert(!(ALIGNED && MULTI), "aligned rows always walk in steps");
  const int npieces = ALIGNED ? S / EPP : (S + 2 * EPP - 2) / EPP;
  const int nsteps = (ALIGNED || MULTI) ? (npieces + G - 1) / G : 1;
  const int h = ALIGNED ? 0 : ((g * S) & (EPP - 1));
  const uint32_t row_byte0 = (uint32_t)(((g * S) / EPP) * 16);
  const uint32_t task_bytes = (uint32_t)(RPT * S) * (uint32_t)sizeof(T);  // multiple of 16
  const int pos0 = li * EPP - h;
  bool km[EPP];  // element e of this lane's piece belongs to the lane's row (unaligned rows; constant per lane)
#pragma unroll
  for (int e = 0; e < EPP; ++e) km[e] = (unsigned)(pos0 + e) < (unsigned)S;
  unsigned char* ring = smem + wave_in_block * (kDmaDepth * slot_bytes);
  unsigned char* spare = smem + 4 * kDmaDepth * slot_bytes;
  typedef __attribute__((address_space(3))) void lds_void;
  typedef const __attribute__((address_space(1))) void glb_void;
  const unsigned char* xb = reinterpret_cast<const unsigned char*>(x);

  // batch tb of the tensor -> slot.  ALWAYS four instructions per batch, so the counted waits are compile-time
  // constants and the loop has no data-dependent branches: lanes past the batch's bytes are masked; an instruction that
  // would be empty (short batches; the tensor's last batch) keeps lane 0 alive on the batch's first 16 bytes.
  const int tail32 = tail_from > (int64_t)0x7fffffff ? 0x7fffffff : (int)tail_from;  // first task of the default-policy tail
  auto issue = [&](int task0, int nu, int slot) __attribute__((always_inline)) {
    const uint32_t nb = (uint32_t)nu * task_bytes;
    const unsigned char* src = xb + task0 * (int64_t)task_bytes;
    unsigned char* d = ring + slot * slot_bytes;
    // cache policy, wave-uniform per batch: streaming (nt) for bytes that come from HBM, default for the part of a
    // just-written input that the Infinity Cache still holds (see launch_rowreduce_dma)
    const bool stream = task0 < tail32;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const uint32_t byte = (uint32_t)i * 1024u + (uint32_t)lane * 16u;
      const bool in = byte < nb;
      // an instruction with no byte of the batch left still goes out (lane 0, the batch's first piece) but lands in the
      // workgroup's spare KiB, not in a slot
      unsigned char* dst_i = (uint32_t)i * 1024u < nb ? d + i * 1024 : spare;
      if (in || lane == 0) {
        if (stream) __builtin_amdgcn_global_load_lds((glb_void*)(src + (in ? byte : 0u)), (lds_void*)dst_i, 16, 0, kLoadAux);
        else __builtin_amdgcn_global_load_lds((glb_void*)(src + (in ? byte : 0u)), (lds_void*)dst_i, 16, 0, 0);
      }
    }
  };
  auto wait_batches = [&](int younger) __attribute__((always_inline)) {  // at most `younger` batches still in flight
    switch (younger * NI) {
#define SL_VMCNT_CASE(n) case n: asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory"); break;
      SL_VMCNT_CASE(0) SL_VMCNT_CASE(4) SL_VMCNT_CASE(8) SL_VMCNT_CASE(12) SL_VMCNT_CASE(16) SL_VMCNT_CASE(24)
#undef SL_VMCNT_CASE
      default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    }
  };

  // Work split.  `full` rounds in which every wave owns a whole batch of U tasks, batches interleaved over the waves
  // (neighbouring waves read neighbouring bytes); the remaining `rem` tasks (< one round) are split EVENLY over the waves
  // as one short batch each instead of leaving most waves idle for a round (the layer4 shape has 5.33 batches per wave:
  // a 6th round for a third of the waves cost 10 %).  The short round covers the tensor's first tasks and is walked last.
  // Walk order of the full rounds: when a tail policy is active (tail_from inside the tensor) the tail goes FIRST —
  // the most recently written bytes are read while the Infinity Cache still holds them, before the head's traffic can
  // displace them (in-pipeline 411 MB: 6.07 -> 6.44 TB/s).
  // 32-bit task / batch indices (the launcher keeps ntask < 2^31): 64-bit scalar compares compile to VALU compares
  // whose result the scalar branch then waits for.
  const int ntask32 = (int)ntask, nwaves32 = (int)nwaves, w0 = (int)wave0;
  const int round_tasks = nwaves32 * U;
  const int full = ntask32 / round_tasks;
  const int rem = ntask32 - full * round_tasks;
  const int u_last = (rem + nwaves32 - 1) / nwaves32;  // <= U
  const int nfull = full * nwaves32;                   // whole batches
  int rot = 0;
  if (tail32 > rem && tail32 < ntask32) rot = (tail32 - rem) / U;
  const int nmine = full + ((int64_t)w0 * u_last < rem ? 1 : 0);
  auto work_of = [&](int it, int& t0, int& n) __attribute__((always_inline)) {
    if (it < full) {
      int v = w0 + it * nwaves32 + rot;
      if (v >= nfull) v -= nfull;
      t0 = rem + v * U;
      n = U;
    } else {
      t0 = w0 * u_last;
      n = rem - t0 < u_last ? rem - t0 : u_last;
    }
  };
  int task0 = 0, task_next = 0;
  int nu = 0, nu_next = 0;
  if (nmine > 0) {
    work_of(0, task_next, nu_next);
    issue(task_next, nu_next, 0);
  }
  static_assert(kDmaDepth == 2, "the loop below keeps exactly one batch in flight beside the one being reduced");
  for (int it = 0; it < nmine; ++it) {
    const int slot = it & 1;
    task0 = task_next;
    nu = nu_next;
    if (it + 1 < nmine) {
      work_of(it + 1, task_next, nu_next);
      issue(task_next, nu_next, slot ^ 1);
      wait_batches(1);  // a constant: one s_waitcnt
    } else {
      wait_batches(0);  // the wave's last batch: drain
    }
    const unsigned char* sl_ = ring + slot * slot_bytes;
    float m[U], sum[U];
    f32x2 sum2[U];  // two partial sums per task, added with one v_pk_add_f32 per half piece
#pragma unroll
    for (int u = 0; u < U; ++u) {
      m[u] = fill;
      sum2[u] = f32x2{0.f, 0.f};
    }
    for (int step = 0; step < nsteps; ++step) {
      const int q = step * G + li;
      uint32_t off;
      bool piece_ok = true;
      if constexpr (ALIGNED) {
        piece_ok = q < npieces;
        off = row_byte0 + (uint32_t)(piece_ok ? q : npieces - 1) * 16u;
      } else if constexpr (MULTI) {
        off = row_byte0 + (uint32_t)(q < npieces ? q : npieces - 1) * 16u;
        const int pos = q * EPP - h;  // q >= npieces: pos >= S, every mask false
#pragma unroll
        for (int e = 0; e < EPP; ++e) km[e] = (unsigned)(pos + e) < (unsigned)S;
      } else {
        off = row_byte0 + (uint32_t)(li < npieces ? li : npieces - 1) * 16u;
      }
      u32x4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const u32x4*>(sl_ + (uint32_t)u * task_bytes + off);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        float e[EPP];
        decode_piece<T, ABS>(v[u], e);
#pragma unroll
        for (int i = 0; i < EPP; ++i) {
          if constexpr (!ALIGNED) e[i] = km[i] ? e[i] : fill;
          if constexpr (SUMOP && ALIGNED) e[i] = piece_ok ? e[i] : 0.f;
        }
        f32x2 ps = f32x2{e[0], e[1]} + f32x2{e[2], e[3]};
        if constexpr (EPP == 8) ps += f32x2{e[4], e[5]} + f32x2{e[6], e[7]};
        if constexpr (SUMOP) {
          sum2[u] += ps;
        } else {
          m[u] = v_max3(v_max3(m[u], e[0], e[1]), e[2], e[3]);
          if constexpr (EPP == 8) m[u] = v_max3(v_max3(m[u], e[4], e[5]), e[6], e[7]);
          sum2[u] += ps;  // NaN detector only
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) sum[u] = sum2[u][0] + sum2[u][1];
    // every ds_read of the slot has returned before a later iteration's DMA may overwrite it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    float r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if constexpr (SUMOP) {
        // sums accumulate in fp32 and are rounded ONCE to the activation dtype, like torch's (identity for fp32)
        r[u] = round_to_dtype<T>(group_allreduce_bcast<G, true>(sum[u], lane) / denom);
      } else {
        r[u] = group_allreduce_bcast<G, false>(m[u], lane);
        const bool row_ok = u < nu;
        // rows of a short last batch read stale slot bytes: their sums are ignored (row_ok)
        if (__builtin_expect(__any(row_ok && sum[u] != sum[u]), 0)) {
          const int64_t row = (int64_t)(task0 + u) * RPT + g;
          if (row_has_nan<T, G>(group_allreduce_f<G, true>(sum[u]), row_ok, x, row, li, S)) r[u] = bits_f32(0x7FC00000u);
        }
      }
    }
#pragma unroll
    for (int p = 0; p < U; p += G) {
      float sel = r[p];
#pragma unroll
      for (int u = p + 1; u < U && u < p + G; ++u) sel = (li == u - p) ? r[u] : sel;
      const int uu = p + li;
      if (li < G && uu < nu) store_outputs(sel, (int64_t)(task0 + uu) * RPT + g, cand, outf);
    }
  }
}

template <typename T, int G, int U, int OP, bool ALIGNED, bool MULTI = false, int NI = kDmaMaxBatch / 1024>
void launch_rowreduce_dma(const ReduceCall& c, const T* x, int64_t R, int S) {
  constexpr int RPT = kWave / G;
  constexpr int ES = (int)sizeof(T);
  const int64_t nbatch = (R / RPT + U - 1) / U;
  const int slot = U * RPT * S * ES;                      // one batch, a multiple of 16 bytes
  const int lds = 4 * kDmaDepth * slot + 1024;            // + 1 KiB: the masked tail of the last slot's last instruction
  int per_cu = kDmaLdsPerCu / lds;
  if (per_cu > 8) per_cu = 8;                             // 32 waves per CU
  const unsigned blocks = grid_blocks((nbatch + 3) / 4, per_cu);
  const int64_t tail_from = nt_head_units(c.policy, R * (int64_t)S * ES, (int64_t)RPT * S * ES);  // tasks from here on: default policy
  if (lds > 64 * 1024) {  // dynamic LDS past 64 KiB has to be allowed per kernel
    static const hipError_t allowed = hipFuncSetAttribute((const void*)rowreduce_dma_kernel<T, G, U, OP, ALIGNED, MULTI, NI>,
                                                          hipFuncAttributeMaxDynamicSharedMemorySize, kDmaLdsPerCu);
    (void)allowed;
  }
  SL_LAUNCH(c.prof, (rowreduce_dma_kernel<T, G, U, OP, ALIGNED, MULTI, NI>), dim3(blocks), dim3(256), (size_t)lds, c.st, x, R,
            S, c.denom, slot, tail_from, c.cand, c.outf);
}

// U values a call site can reach, as a mask of (1 << U); NI = 16 (one 4-16 KiB task per batch) is kDmaU16K
constexpr int kDmaU1 = 1 << 1, kDmaU2 = 1 << 2, kDmaU3 = 1 << 3, kDmaU4 = 1 << 4, kDmaU16K = 1 << 5;
constexpr int kDmaUAll = kDmaU1 | kDmaU2 | kDmaU3 | kDmaU4;

// U = tasks per batch (<= 4) so that a batch is at most 4 KiB.  0: not for this kernel (a task alone is larger, tasks are not
// whole pieces or rows do not group into tasks, or the input is small: launch-bound either way; the kernel indexes tasks with
// 32 bits), 1: launched, negative: a U outside UMASK — the set the call site derived from its guards, the only ones instantiated.
template <int G, int OP, bool ALIGNED, typename T, bool MULTI, int UMASK>
int try_rowreduce_dma(const char* site, const ReduceCall& c, const T* x, int64_t R, int S) {
  constexpr int RPT = kWave / G;
  const int64_t task_bytes = (int64_t)RPT * S * (int64_t)sizeof(T);
  if (task_bytes > (MULTI && sizeof(T) == 2 ? 16 * 1024 : kDmaMaxBatch) || (task_bytes & 15) != 0 || R % RPT != 0 ||
      R * (int64_t)S * (int64_t)sizeof(T) < (8ll << 20) || R > 0x7fffffffll)
    return 0;
  const int u = (int)(kDmaMaxBatch / task_bytes);
#define SL_DMA_U(BIT_, U_, NI_)                                                                            \
  do {                                                                                                     \
    if constexpr ((UMASK & (BIT_)) != 0) {                                                                 \
      launch_rowreduce_dma<T, G, U_, OP, ALIGNED, MULTI, NI_>(c, x, R, S);                                 \
      return 1;                                                                                            \
    } else {                                                                                               \
      return dma_unreachable(site, NI_ == 16 ? 16 : U_, R, S);                                             \
    }                                                                                                      \
  } while (0)
  if constexpr (MULTI) {  // long windows: a task is 1-4 KiB, so one or two tasks per batch
    // 4-16 KiB: one task per batch of sixteen instructions, one workgroup per CU.  2-byte elements only: 17 x 17 fp16 maps
    // 2.8 -> 4.1 TB/s against rowreduce_h, which leaves 27 of 64 lanes idle there; fp32 rows of this length lose
    // (27 x 27: 5.7 -> 5.4 TB/s against launch_rowreduce<64, 4>) and stay on the VGPR-load kernel
    if (task_bytes > kDmaMaxBatch) SL_DMA_U(kDmaU16K, 1, 16);
    if (u >= 2) SL_DMA_U(kDmaU2, 2, 4);
    SL_DMA_U(kDmaU1, 1, 4);
  } else {
    if (u >= 4) SL_DMA_U(kDmaU4, 4, 4);
    if (u == 3) SL_DMA_U(kDmaU3, 3, 4);
    if (u == 2) SL_DMA_U(kDmaU2, 2, 4);
    SL_DMA_U(kDmaU1, 1, 4);
  }
#undef SL_DMA_U
}

}  // namespace
}  // namespace sl
