// K2 (and channels_last K1) — the reduced axis strided, the component axis contiguous: colreduce2 (16-byte pieces, the
// default) and colreduce (4-element loads: what is left when pieces are not legal), and their launchers.  Overview of the
// kernel families: reduce.hip.
#include "reduce_common.hpp"

namespace sl {
namespace {

// ---- colreduce: out[b][f] = op_t x[b][t][f], f contiguous ------------------------------------
// One workgroup (NW = 4 waves, or 16 when there are too few (b, chunk) tasks to fill the chip — small batches of long
// token sequences) per (b, 256-float chunk of F); the waves split T; LDS combine.
// Cache policy as in the row kernels (reduce.hip): tasks below `tail_from` (in memory order: b-major) stream with
// nt, the rest use the default policy, and the walk starts at `tail_from` so that the bytes written last are read first.
template <typename E, int OP, int NW>
__global__ __launch_bounds__(64 * NW) void colreduce_kernel(const E* __restrict__ x, int64_t B, int T, int64_t F,
                                                         int64_t sb, int64_t st, int t_begin, int t_end,
                                                         float denom, int64_t tail_from, uint16_t* __restrict__ cand,
                                                         float* __restrict__ outf) {
  __shared__ float s_part[NW][256];
  constexpr bool SUM = (OP == OP_SUM || OP == OP_ABSSUM);
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int64_t nchunk = (F + 255) / 256;
  const int64_t ntask = B * nchunk;
  const int64_t rot = (tail_from > 0 && tail_from < ntask) ? tail_from : 0;
  for (int64_t ti = blockIdx.x; ti < ntask; ti += gridDim.x) {
    int64_t task = ti + rot;
    if (task >= ntask) task -= ntask;
    const int64_t b = task / nchunk;
    const int64_t f0 = (task % nchunk) * 256 + lane * 4;
    Acc<OP> a0, a1, a2, a3;
    a0.init(); a1.init(); a2.init(); a3.init();
    const bool in = f0 < F;  // F % 4 == 0 on this path
    const E* base = x + b * sb + f0;
    auto walk = [&](auto NT) __attribute__((always_inline)) {
      constexpr bool nt = decltype(NT)::value;
      auto ld = [&](const E* p) __attribute__((always_inline)) { return load4_as_f32<E, nt>(p); };
      int t = t_begin + w;
#pragma unroll 1
      for (; t + 7 * NW < t_end; t += 8 * NW) {  // 8 loads in flight per lane
        float4 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = ld(base + (int64_t)(t + NW * j) * st);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          a0.add(v[j].x, true); a1.add(v[j].y, true); a2.add(v[j].z, true); a3.add(v[j].w, true);
        }
      }
      for (; t < t_end; t += NW) {
        float4 v = ld(base + (int64_t)t * st);
        a0.add(v.x, true); a1.add(v.y, true); a2.add(v.z, true); a3.add(v.w, true);
      }
    };
    if (in) {
      if (task < tail_from) walk(std::true_type());
      else walk(std::false_type());
    }
    s_part[w][lane * 4 + 0] = a0.lane_value();
    s_part[w][lane * 4 + 1] = a1.lane_value();
    s_part[w][lane * 4 + 2] = a2.lane_value();
    s_part[w][lane * 4 + 3] = a3.lane_value();
    __syncthreads();
    if (threadIdx.x < 256) {
      const int f = threadIdx.x;  // 256 threads -> 256 features of the chunk
      const int64_t fg = (task % nchunk) * 256 + f;
      if (fg < F) {
        float r = s_part[0][f];
#pragma unroll
        for (int i = 1; i < NW; ++i) r = combine<SUM>(r, s_part[i][f]);
        r = round_to_dtype<E>(finish<OP>(r, denom));  // the reference aggregates in the activation's dtype
        store_outputs(r, b * F + fg, cand, outf);
      }
    }
    __syncthreads();
  }
}

// ---- colreduce2 (round 4): 16-byte pieces for every dtype, LPR lanes per row, loads never drain ------------------------------
// What the round-4 lab (tools/k2_lab.py, profiles/r04_k2_lab.txt) found wrong with colreduce_kernel on (256, 197, 768):
//  * its row tail ran ONE load per lane and iteration: 197 = 6 x 32 + 5 rows left two serialised memory round trips (~2 us
//    each) at the end of a 26-us launch; (256, 196, 1024) — one tail trip, 16 waves per CU — ran 6.3 TB/s, this shape 5.9;
//  * a round of eight loads was reduced before the next eight were issued: the bytes in flight swung between 8 KB per wave and
//    nothing (the LDS-DMA ring kernel, reduce_dma.hpp, removes that too, but its rings cap a CU at 16 waves: 5.6-6.1 TB/s);
//  * half-precision rows were read with 8-byte loads (512 B per wave instruction): 5.0 TB/s where fp32 reads 5.9.
// Here every load is 16 bytes (a *piece*: 4 fp32 or 8 half components).  A row chunk is LPR pieces (64, 32 or 16 lanes), so a
// wave instruction covers 64 / LPR rows x LPR x 16 bytes = 1 KiB whatever the row length: fp16 F = 768 (96 pieces) takes LPR = 32
// (three full chunks) instead of 1.5 chunks of 64; lanes that share a piece column combine once at the end (one xor-shuffle per
// level).  Rows are walked in blocks of INFL loads per lane; block k + 1 is issued BEFORE block k is reduced (two register
// sets, ping-pong), so 8-16 loads per lane are in flight from the first block to the last.  No predicated loads: a row past the
// end is clamped to the last row (a cache hit) and its values are discarded by the accumulator's `valid` flag, so the last
// block costs one round trip like any other.
// Round 5: the input is a TABLE of up to kMaxReduceSources same-shape tensors (the outputs of L identical transformer blocks,
// kept alive until the last one exists): "virtual" batch b of the B = L * per batches lives in tensor b / per at batch b % per,
// and the (L, per, F) outputs are one contiguous buffer, so nothing else in the kernel changes.  One 1.9 GB launch instead of
// twelve 155 MB ones: the ~2.5 us a launch costs beyond bytes / 6.45 TB/s is paid once (a single tensor is a table of one).

template <typename E, int OP, int NW, int LPR, int INFL>
__global__ __launch_bounds__(64 * NW) void colreduce2_kernel(MultiSrc src, int64_t B, int T, int64_t F, int64_t sb,
                                                              int64_t st, int t_begin, int t_end, float denom, int64_t tail_from,
                                                              uint16_t* __restrict__ cand, float* __restrict__ outf) {
  constexpr int EPP = 16 / (int)sizeof(E);
  constexpr int RPI = 64 / LPR;  // rows per wave instruction
  constexpr int CW = LPR * EPP;  // components per chunk
  constexpr bool SUM = (OP == OP_SUM || OP == OP_ABSSUM);
  constexpr bool ABS = (OP == OP_ABSMAX || OP == OP_ABSSUM);
  constexpr int STEP = NW * RPI;  // rows one instruction of every wave of the workgroup covers
  __shared__ float s_part[NW][CW];
  const int lane = threadIdx.x & 63;
  const int w = threadIdx.x >> 6;
  const int sub = lane / LPR, pl = lane % LPR;
  const int64_t nchunk = (F + CW - 1) / CW;
  const int64_t ntask = B * nchunk;
  const int64_t rot = (tail_from > 0 && tail_from < ntask) ? tail_from : 0;
  const int tw = t_begin + w * RPI + sub;  // this lane's first row
  const int last = t_end - 1;
  const int rows_w = t_end - (t_begin + w * RPI);                 // rows from the wave's first row on
  const int ninst = rows_w > 0 ? (rows_w + STEP - 1) / STEP : 0;  // wave instructions that touch a valid row
  const int nblk = (ninst + INFL - 1) / INFL;
  const int64_t row_pieces = st * (int64_t)sizeof(E) / 16;
  for (int64_t ti = blockIdx.x; ti < ntask; ti += gridDim.x) {
    int64_t task = ti + rot;
    if (task >= ntask) task -= ntask;
    const int64_t b = task / nchunk;
    const int64_t f0 = (task % nchunk) * CW + (int64_t)pl * EPP;
    const bool in = f0 < F;  // F % EPP == 0 on this path; lanes past the row re-read its first piece and are never stored
    const E* x = static_cast<const E*>(src.ptr[b / src.per]);
    const u32x4* base = reinterpret_cast<const u32x4*>(x + (b % src.per) * sb + (in ? f0 : 0));
    // max ops: v_max_f32 drops NaN, torch.amax propagates it.  As in K1 a running SUM rides along (v_pk_add_f32: NaN in => NaN
    // out) and only columns whose sum is NaN (a NaN, or +inf with -inf) are looked at again, exactly.  Rows past the end are
    // CLAMPED to the last row: a duplicate changes neither a max nor the detector's verdict; sums mask them instead.
    float m[EPP];
    f32x2 det[EPP / 2];
#pragma unroll
    for (int e = 0; e < EPP; ++e) m[e] = SUM ? 0.f : -__builtin_huge_valf();
#pragma unroll
    for (int e = 0; e < EPP / 2; ++e) det[e] = f32x2{0.f, 0.f};
    auto walk = [&](auto NT) __attribute__((always_inline)) {
      constexpr bool nt = decltype(NT)::value;
      auto load = [&](u32x4(&v)[INFL], int k) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < INFL; ++j) {
          int row = tw + (k * INFL + j) * STEP;
          row = row < last ? row : last;
          const u32x4* p = base + (int64_t)row * row_pieces;
          if constexpr (nt) v[j] = __builtin_nontemporal_load(p);
          else v[j] = *p;
        }
      };
      auto reduce = [&](const u32x4(&v)[INFL], int k) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < INFL; ++j) {
          float e[EPP];
          decode_piece<E, ABS>(v[j], e);
          if constexpr (SUM) {
            const bool ok = tw + (k * INFL + j) * STEP <= last;
#pragma unroll
            for (int i = 0; i < EPP; ++i) m[i] += ok ? e[i] : 0.f;
          } else {
#pragma unroll
            for (int i = 0; i < EPP; ++i) m[i] = __builtin_fmaxf(m[i], e[i]);
#pragma unroll
            for (int i = 0; i < EPP / 2; ++i) det[i] += f32x2{e[2 * i], e[2 * i + 1]};
          }
        }
      };
      u32x4 va[INFL], vb[INFL];
      if (nblk > 0) load(va, 0);
#pragma unroll 1
      for (int k = 0; k < nblk; k += 2) {
        const bool more1 = k + 1 < nblk;
        if (more1) load(vb, k + 1);
        reduce(va, k);
        if (more1) {
          if (k + 2 < nblk) load(va, k + 2);
          reduce(vb, k + 1);
        }
      }
    };
    if (task < tail_from) walk(std::true_type());
    else walk(std::false_type());
    if constexpr (!SUM) {
      bool sus = false;
#pragma unroll
      for (int i = 0; i < EPP / 2; ++i) sus |= (det[i][0] != det[i][0]) | (det[i][1] != det[i][1]);
      if (__builtin_expect(__any(sus), 0)) {  // rare: a NaN, or +inf and -inf in one column — look again, exactly
        bool nan[EPP];
#pragma unroll
        for (int i = 0; i < EPP; ++i) nan[i] = false;
        if (sus) {
          for (int row = tw; row <= last; row += STEP) {
            float e[EPP];
            decode_piece<E, ABS>(base[(int64_t)row * row_pieces], e);
#pragma unroll
            for (int i = 0; i < EPP; ++i) nan[i] |= (e[i] != e[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < EPP; ++i) m[i] = nan[i] ? bits_f32(0x7FC00000u) : m[i];
      }
    }
#pragma unroll
    for (int e = 0; e < EPP; ++e) {
      float r = m[e];
      if constexpr (RPI >= 4) r = combine<SUM>(r, __shfl_xor(r, 16, 64));
      if constexpr (RPI >= 2) r = combine<SUM>(r, __shfl_xor(r, 32, 64));
      if (lane < LPR) s_part[w][lane * EPP + e] = r;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < CW; f += 64 * NW) {
      const int64_t fg = (task % nchunk) * CW + f;
      if (fg < F) {
        float v = s_part[0][f];
#pragma unroll
        for (int i = 1; i < NW; ++i) v = combine<SUM>(v, s_part[i][f]);
        v = round_to_dtype<E>(finish<OP>(v, denom));  // the reference aggregates in the activation's dtype
        store_outputs(v, b * F + fg, cand, outf);
      }
    }
    __syncthreads();
  }
}

// colreduce2: the default component-contiguous kernel where 16-byte pieces are legal (see the kernel's header).
// loads per lane and block, two blocks in flight.  4 (tools/k2_lab.py): 72 VGPRs in fp32 / 100 in half precision (6-7 / 4 waves
// per SIMD); with 8 the half-precision kernels need 140 registers and fall from 5.3 to 4.0 TB/s, fp32 gains nothing
constexpr int kCol2Infl = 4;
template <typename T, int OP, int NW, int LPR>
void launch_colreduce2_as(const ReduceCall& c, const MultiSrc& x, int64_t B, int T_, int64_t F, int64_t sb, int64_t st_, int t0, int t1,
                          int64_t tail_from) {
  constexpr int CW = LPR * (16 / (int)sizeof(T));
  const unsigned blocks = grid_blocks(B * ((F + CW - 1) / CW), 8);
  SL_LAUNCH(c.prof, (colreduce2_kernel<T, OP, NW, LPR, kCol2Infl>), dim3(blocks), dim3(64 * NW), 0, c.st, x, B, T_, F, sb, st_, t0,
            t1, c.denom, tail_from, c.cand, c.outf);
}

// `x`: a table of L = B / x.per tensors of x.per batches each (L = 1: one tensor); B counts the batches of all of them
template <typename T, int OP>
bool launch_colreduce2_t(const ReduceCall& c, const MultiSrc& x, int64_t B, int T_, int64_t F, int64_t sb, int64_t st_, int t0, int t1) {
  const int forced_nw = (int)option(OPT_COLREDUCE_NW);  // sl_set_option("colreduce_nw", 4 / 8 / 16): tests walk every instance
  constexpr int EPP = 16 / (int)sizeof(T);
  const int64_t rows = t1 - t0;
  const int64_t L = B / x.per;
  bool aligned = true;
  for (int64_t l = 0; l < L; ++l) aligned = aligned && ((uintptr_t)x.ptr[l] & 15) == 0;
  if (!aligned || (F % EPP) != 0 || ((st_ * (int64_t)sizeof(T)) & 15) != 0 ||
      ((sb * (int64_t)sizeof(T)) & 15) != 0 || rows < 1)
    return false;
  // lanes per row: the widest chunk that wastes no lane, else the one that wastes least (ties: wider = fewer tasks)
  const int64_t pr = F / EPP;  // pieces per row
  int lpr = 64;
  double best = 0;
  for (int c : {64, 32, 16}) {
    const double util = (double)pr / (double)(((pr + c - 1) / c) * c);
    if (util > best + 1e-9) best = util, lpr = c;
  }
  const int64_t cw = (int64_t)lpr * EPP, nchunk = (F + cw - 1) / cw, cus = num_cus();
  const int64_t per_b = (int64_t)T_ * F * (int64_t)sizeof(T);
  // cache policy in tasks = (b, chunk) pairs, b-major like the bytes.  Of a table of tensors only the LAST one was written a
  // moment ago: the default-policy tail never reaches into the others
  const int64_t tail_from = nt_head_units(c.policy, B * per_b, per_b, nchunk, L > 1 ? x.per * per_b : INT64_MAX);
  // waves per task split the reduced axis; a wave instruction covers 64 / lpr rows, so short axes want few waves
  const int64_t inst_rows = rows * lpr / 64;  // wave instructions per task
  // 8 waves per task only below two tasks per CU.  tools/k2_lab.py (an elementwise producer, then K2) showed the fp32 kernel
  // 2-5 % faster with 8 waves up to four tasks per CU ((256, 197, 768): 6.09 -> 6.19 TB/s cold), but INSIDE the bench's leg
  // (behind a ViT block's GEMMs, tools/k2_leg_probe.py) the same shape reads 0.717 of spec with four waves and 0.671 with
  // eight; the half-precision kernels (100 registers, 16 waves per CU) lose 15 % with eight once there are two tasks per CU
  // ((256, 257, 1024) bf16: 6.07 -> 5.15 TB/s).  profiles/r04_k2_lab.txt
  // A table of L tensors takes the wave count ONE of its tensors would take alone: the waves split the reduced axis, so the
  // fp32 summation order of mean / absmean / sum follows NW, and a layer's candidates must not depend on whether its batch
  // was reduced alone (a collector's first batch, SEMANTICLENS_AMD_GROUP_LAYERS=0) or as a member of a group.
  const int64_t tasks_one = x.per * nchunk;
  int nw = 4;
  if (tasks_one * 2 < cus && inst_rows >= 128 && lpr == 64) nw = 16;
  else if (tasks_one < (sizeof(T) == 4 ? 2 : 1) * cus && inst_rows >= 64) nw = 8;
  if (forced_nw == 4 || forced_nw == 8 || (forced_nw == 16 && lpr == 64)) nw = forced_nw;
#define SL_COL2(NW_, LPR_) launch_colreduce2_as<T, OP, NW_, LPR_>(c, x, B, T_, F, sb, st_, t0, t1, tail_from)
#define SL_COL2_NW(LPR_)                 \
  do {                                   \
    if (nw == 16) SL_COL2(16, LPR_);     \
    else if (nw == 8) SL_COL2(8, LPR_);  \
    else SL_COL2(4, LPR_);               \
  } while (0)
  if (lpr == 64) {
    SL_COL2_NW(64);
  } else if (lpr == 32) {
    if (nw == 8) SL_COL2(8, 32);
    else SL_COL2(4, 32);
  } else {
    if (nw == 8) SL_COL2(8, 16);
    else SL_COL2(4, 16);
  }
#undef SL_COL2_NW
#undef SL_COL2
  return true;
}

template <typename T, int OP>
void launch_colreduce_t(const ReduceCall& c, const T* x, int64_t B, int T_, int64_t F, int64_t sb, int64_t st_, int t0, int t1) {
  MultiSrc one;
  one.ptr[0] = x;
  one.per = B;
  if (launch_colreduce2_t<T, OP>(c, one, B, T_, F, sb, st_, t0, t1)) return;
  const int64_t nchunk = (F + 255) / 256, per_b = (int64_t)T_ * F * (int64_t)sizeof(T);
  const unsigned blocks = grid_blocks(B * nchunk, 8);
  // cache policy in tasks = (b, chunk) pairs, b-major like the bytes
  const int64_t tail_from = nt_head_units(c.policy, B * per_b, per_b, nchunk);
  // waves per task (they split the reduced axis): enough of them that a CU holds ~24 waves with 8 loads in flight each.
  // (B, 197, 768) at B = 256 is 768 tasks: 4-wave workgroups put 12 waves on a CU (5.4 TB/s cold), 8-wave ones 24.
  const int forced_nw = (int)option(OPT_COLREDUCE_NW);
  const int64_t tasks = B * nchunk, rows = t1 - t0, cus = num_cus();
  int nw = 4;
  // measured cold (tools/reduce_dtype_bench.py, SL_COLREDUCE_NW = 4 / 8 / 16): (256, 197, 768) fp32 5.52 / 5.63 / 5.46 TB/s,
  // (48, 729, 1152) fp32 5.46 / 5.73 / 5.45 and fp16 3.7 / 5.45 / 5.03, channels_last 14 x 14 fp16 5.74 / 5.94 / 4.0;
  // short reduced axes (7 x 7 = 49 rows, 50 tokens) lose with more than four waves
  // In the pipeline (input just written, bench leg `tokens_collect`, seven runs) the 768-task shape reads 0.60-0.69 of spec with
  // four waves against 0.55-0.65 with eight, so eight-wave workgroups are kept for grids below two tasks per CU.
  if (tasks * 2 < cus && rows >= 128) nw = 16;
  else if (tasks < 2 * cus && rows >= 64) nw = 8;
  if (forced_nw == 4 || forced_nw == 8 || forced_nw == 16) nw = forced_nw;
  if (nw == 16)
    SL_LAUNCH(c.prof, (colreduce_kernel<T, OP, 16>), dim3(blocks), dim3(1024), 0, c.st, x, B, T_, F, sb, st_, t0, t1, c.denom,
              tail_from, c.cand, c.outf);
  else if (nw == 8)
    SL_LAUNCH(c.prof, (colreduce_kernel<T, OP, 8>), dim3(blocks), dim3(512), 0, c.st, x, B, T_, F, sb, st_, t0, t1, c.denom,
              tail_from, c.cand, c.outf);
  else
    SL_LAUNCH(c.prof, (colreduce_kernel<T, OP, 4>), dim3(blocks), dim3(256), 0, c.st, x, B, T_, F, sb, st_, t0, t1, c.denom,
              tail_from, c.cand, c.outf);
}

// dtype -> element tag T inside the statement
#define SL_SWITCH_DTYPE(dtype, ...)                        \
  do {                                                     \
    if (dtype == SL_F32) { using T = float; __VA_ARGS__; } \
    else if (dtype == SL_F16) { using T = _Float16; __VA_ARGS__; } \
    else { using T = uint16_t; __VA_ARGS__; }              \
  } while (0)

}  // namespace

int launch_colreduce2(int op, int dtype, const ReduceCall& c, const void* const* srcs, int64_t per, int64_t B, int T_, int64_t F,
                      int64_t sb, int64_t st_, int t0, int t1) {
  MultiSrc x;
  for (int64_t l = 0; l < B / per; ++l) x.ptr[l] = srcs[l];
  x.per = per;
  SL_SWITCH_OP(op, SL_SWITCH_DTYPE(dtype, return (launch_colreduce2_t<T, OP>(c, x, B, T_, F, sb, st_, t0, t1) ? 1 : 0)));
  return bad_reduce_op("launch_colreduce2", op);
}

int launch_colreduce(int op, int dtype, const ReduceCall& c, const void* x, int64_t B, int T_, int64_t F, int64_t sb, int64_t st_,
                     int t0, int t1) {
  SL_SWITCH_OP(op, SL_SWITCH_DTYPE(dtype, launch_colreduce_t<T, OP>(c, (const T*)x, B, T_, F, sb, st_, t0, t1);
                                   return 0));
  return bad_reduce_op("launch_colreduce", op);
}

}  // namespace sl
