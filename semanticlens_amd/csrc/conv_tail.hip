// K27 — the 64 -> 256 channel 1x1 convolutions of layer1 inside the residual tail.
//   FORM_CONV      y = W x                                   (the raw product: what the tests and the probe compare)
//   FORM_ADD_RELU  y = clamp_min(bn(W x) + identity, 0)      (an identity block's conv3 -> bn3 -> add -> relu)
//   FORM_DUAL      y = clamp_min(bn_a(Wa xa) + bn_b(Wb xb), 0)  (layer1.0: conv3 and the shortcut's conv, operands as in K19)
// over contiguous NCHW fp32, Ci = 64, Co = 256.  One read of x (and of the identity or the second x), one write of y: the
// product never goes through memory.
//
// The contract is bit equality with the unfused model, so the product restates the GEMM kernel MIOpen's 1x1 solver runs: the
// same instruction (v_mfma_f32_16x16x4_f32), k ascending, K = 64 taken in S partial chains that are added at the end.  Which
// split a site's kernel uses is not documented; `split` selects among the candidates below and tools/conv_tail_probe.py counts
// their mismatches on the device.  This file is compiled with -ffp-contract=off like batchnorm.hip, whose BatchNorm forms it
// applies (bn_apply.hpp).
//
// Mapping.  A wave owns 32 pixels of one image and all 256 output channels.  MFMA rows are pixels and columns output channels,
// so a lane's four accumulator registers are four adjacent pixels of one channel: the epilogue loads the identity and stores y in
// 16-byte pieces.  The A operand of step s is x[k = order[4 s + lane / 16]][pixel = lane % 16], read from global memory in that
// layout (64-byte runs), once per wave.  W sits in LDS for the whole launch as B fragments, four steps per ds_read_b128.
// Per-channel constants: a {mean, inv_std, scale, bias} table in LDS behind W, built by every block as in batchnorm.hip.
// W and the BatchNorm tensors are read on every launch; nothing survives it.
#include "bn_apply.hpp"

namespace sl {
namespace {

enum { FORM_CONV = 0, FORM_ADD_RELU = 1, FORM_DUAL = 2 };

constexpr int kCi = 64, kCo = 256;
constexpr int kSteps = kCi / 4;   // MFMA steps of one product
constexpr int kNt = kCo / 16;     // column tiles
constexpr int kBlock = 512, kWaves = kBlock / 64;
constexpr int kTilePx = 32;       // pixels per wave and trip: two MFMA row tiles
constexpr int kWFloats = kCi * kCo;
constexpr int kSplits = 7;
constexpr int64_t kMaxTotal = (int64_t)1 << 31;

// split: 0  one chain
//        1  two chains over k [0,32) [32,64)             2  two chains, MFMA steps dealt alternately
//        3  four chains over runs of 16, added in order   4  the same, added pairwise
//        5  four chains, steps dealt round-robin, in order  6  the same, pairwise
template <int S, bool INTER>
__device__ constexpr int chain_of(int s) {
  return INTER ? s % S : s / (kSteps / S);
}

template <int S, bool PAIR>
__device__ inline f4 combine(const f4 (&p)[S]) {
  if constexpr (S == 1)
    return p[0];
  else if constexpr (S == 2)
    return p[0] + p[1];
  else if constexpr (PAIR)
    return (p[0] + p[1]) + (p[2] + p[3]);
  else
    return ((p[0] + p[1]) + p[2]) + p[3];
}

// W (Co, Ci) as B fragments: float ((nt * 4 + s / 4) * 64 + lane) * 4 + s % 4 holds W[16 nt + lane % 16][order[4 s + lane / 16]]
__device__ inline void stage_w(float* wl, const float* __restrict__ w, const int32_t* __restrict__ order) {
  for (int d = threadIdx.x; d < kWFloats; d += kBlock) {
    const int sj = d & 3, lane = (d >> 2) & 63, s4 = (d >> 8) & 3, nt = d >> 10;
    const int slot = 4 * (4 * s4 + sj) + (lane >> 4);
    const int k = order ? order[slot] : slot;
    wl[d] = w[(16 * nt + (lane & 15)) * kCi + k];
  }
}

// the A fragments of a wave's 32 pixels: a[t][s] = x[k(s, lane / 16)][p0 + 16 t + lane % 16].  A row past the image reads the
// image's last pixel instead (no branch between the loads: all 32 are in flight at once); its products are never stored.
__device__ inline void load_a(float (&a)[2][kSteps], const float* __restrict__ xn, const uint32_t (&koff)[kSteps], uint32_t p0,
                              uint32_t HW, uint32_t j) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const uint32_t px = p0 + 16 * t + j, at = px < HW ? px : HW - 1;
#pragma unroll
    for (int s = 0; s < kSteps; ++s) a[t][s] = xn[koff[s] + at];
  }
}

// r[t]: pixels 4 (lane / 16) .. + 3 of row tile t, channel 16 nt + lane % 16.  wl4 points at this lane's fragments of tile nt.
template <int S, bool INTER, bool PAIR>
__device__ inline void product(const float (&a)[2][kSteps], const f4* wl4, f4 (&r)[2]) {
  f4 p[2][S];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int c = 0; c < S; ++c) p[t][c] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s4 = 0; s4 < kSteps / 4; ++s4) {
    const f4 b = wl4[s4 * 64];
#pragma unroll
    for (int sj = 0; sj < 4; ++sj) {
      const int s = 4 * s4 + sj, c = chain_of<S, INTER>(s);
#pragma unroll
      for (int t = 0; t < 2; ++t) p[t][c] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][s], b[sj], p[t][c], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < 2; ++t) r[t] = combine<S, PAIR>(p[t]);
}

// four adjacent pixels of one plane row; ALIGNED: HW % 4 == 0, so a piece that starts inside the image ends inside it
template <bool ALIGNED>
__device__ inline f4 load_px4(const float* __restrict__ plane, uint32_t px, uint32_t HW) {
  f4 v = {0.f, 0.f, 0.f, 0.f};
  if constexpr (ALIGNED) {  // past the image: the image's last piece, which the epilogue does not store (no branch, as in load_a)
    v = __builtin_nontemporal_load(reinterpret_cast<const f4*>(plane + (px < HW ? px : HW - 4)));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (px + e < HW) v[e] = __builtin_nontemporal_load(plane + px + e);
  }
  return v;
}
template <bool ALIGNED>
__device__ inline void store_px4(float* __restrict__ plane, uint32_t px, uint32_t HW, f4 v) {
  if constexpr (ALIGNED) {
    if (px < HW) *reinterpret_cast<f4*>(plane + px) = v;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (px + e < HW) plane[px + e] = v[e];
  }
}

// `other`: the identity (FORM_ADD_RELU) or the second convolution's input (FORM_DUAL, with wb and bnb).  tiles = ceil(HW / 32);
// the waves of the grid stride over the N * tiles (image, pixel tile) pairs.
template <int FORM, int S, bool INTER, bool PAIR, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void conv_tail_kernel(const float* __restrict__ xa, const float* __restrict__ wa,
                                                           const BnParams bna, const float* __restrict__ other,
                                                           const float* __restrict__ wb, const BnParams bnb,
                                                           float* __restrict__ y, const int32_t* __restrict__ order, uint32_t N,
                                                           uint32_t HW, uint32_t tiles) {
  constexpr bool DUAL = FORM == FORM_DUAL;
  constexpr int EPI = DUAL ? EPI_ADD_BN_RELU : EPI_ADD_RELU;
  extern __shared__ f4 lds[];
  float* wl = reinterpret_cast<float*>(lds);
  f4* tab = lds + (DUAL ? 2 : 1) * (kWFloats / 4);
  stage_w(wl, wa, order);
  if constexpr (DUAL) stage_w(wl + kWFloats, wb, order);
  if constexpr (FORM != FORM_CONV) {
    for (uint32_t c = threadIdx.x; c < (uint32_t)kCo; c += kBlock) {
      tab[c] = bn_constants(bna, c);
      if constexpr (DUAL) tab[kCo + c] = bn_constants(bnb, c);
    }
  }
  __syncthreads();

  const uint32_t lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  const uint32_t wave = blockIdx.x * kWaves + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t nwaves = gridDim.x * kWaves, nwork = N * tiles;
  uint32_t koff[kSteps];
#pragma unroll
  for (int s = 0; s < kSteps; ++s) koff[s] = (uint32_t)(order ? order[4 * s + g] : 4 * s + (int)g) * HW;
  const f4* wl4 = lds + lane;

  for (uint32_t work = wave; work < nwork; work += nwaves) {
    const uint32_t n = work / tiles, p0 = (work - n * tiles) * kTilePx;
    float a[2][kSteps], ab[DUAL ? 2 : 1][kSteps];
    load_a(a, xa + (size_t)n * kCi * HW, koff, p0, HW, j);
    if constexpr (DUAL) load_a(ab, other + (size_t)n * kCi * HW, koff, p0, HW, j);
    // The column tiles are unrolled so that the identity of tile nt + 1 is asked for before the product of tile nt and is
    // there when that tile's epilogue wants it, and so that nothing but a tile's own operands is waited for.
    const size_t row0 = ((size_t)n * kCo + j) * HW;
    f4 ahead[2];
    if constexpr (FORM == FORM_ADD_RELU) {
#pragma unroll
      for (int t = 0; t < 2; ++t) ahead[t] = load_px4<ALIGNED>(other + row0, p0 + 16 * t + 4 * g, HW);
    }
#pragma unroll
    for (int nt = 0; nt < kNt; ++nt) {
      const uint32_t co = 16 * nt + j;
      const size_t row = row0 + (size_t)(16 * nt) * HW;
      f4 r[2], rb[2];
      if constexpr (FORM == FORM_ADD_RELU) {
#pragma unroll
        for (int t = 0; t < 2; ++t) rb[t] = ahead[t];
        if (nt + 1 < kNt) {
#pragma unroll
          for (int t = 0; t < 2; ++t) ahead[t] = load_px4<ALIGNED>(other + row + (size_t)16 * HW, p0 + 16 * t + 4 * g, HW);
        }
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler otherwise sinks the loads to where their values are used)
      }
      // (the raw product has nothing to keep in place, but without a fence between its tiles the scheduler hoists the LDS reads
      // and accumulators of all sixteen together: 256 VGPRs and 300+ bytes of scratch per lane)
      if constexpr (FORM == FORM_CONV) __builtin_amdgcn_sched_barrier(0);
      product<S, INTER, PAIR>(a, wl4 + nt * 256, r);
      if constexpr (DUAL) product<S, INTER, PAIR>(ab, wl4 + kWFloats / 4 + nt * 256, rb);
      f4 k = {}, kb = {};
      if constexpr (FORM != FORM_CONV) k = tab[co];
      if constexpr (DUAL) kb = tab[kCo + co];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        f4 o = r[t];
        if constexpr (FORM != FORM_CONV) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = bn_finish<EPI>(r[t][e], k, rb[t][e], kb);
        }
        store_px4<ALIGNED>(y + row, p0 + 16 * t + 4 * g, HW, o);
      }
    }
  }
}

// what SL_LAUNCH sees when a launch leaves no profile record
struct NoProf {
  hipEvent_t start = nullptr, stop = nullptr;
};

template <int FORM, int S, bool INTER, bool PAIR, bool ALIGNED, class Prof>
int launch_instance(Prof& prof, dim3 grid, size_t lds, hipStream_t st, const float* xa, const float* wa, const BnParams& bna,
                    const float* other, const float* wb, const BnParams& bnb, float* y, const int32_t* order, uint32_t N,
                    uint32_t HW, uint32_t tiles) {
  // W alone is 64 KiB: more dynamic LDS than a kernel gets without asking (per device, so asked at every launch)
  SL_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_tail_kernel<FORM, S, INTER, PAIR, ALIGNED>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  SL_LAUNCH(prof, (conv_tail_kernel<FORM, S, INTER, PAIR, ALIGNED>), grid, dim3(kBlock), lds, st, xa, wa, bna, other, wb, bnb, y,
            order, N, HW, tiles);
  return 0;
}

template <int FORM, bool ALIGNED, class Prof>
int launch_split(int split, Prof& prof, dim3 grid, size_t lds, hipStream_t st, const float* xa, const float* wa,
                 const BnParams& bna, const float* other, const float* wb, const BnParams& bnb, float* y, const int32_t* order,
                 uint32_t N, uint32_t HW, uint32_t tiles) {
#define SL_CT(S_, I_, P_) \
  return launch_instance<FORM, S_, I_, P_, ALIGNED>(prof, grid, lds, st, xa, wa, bna, other, wb, bnb, y, order, N, HW, tiles)
  if constexpr (FORM != FORM_CONV) {
    SL_CT(1, false, false);  // the tails take the split that Step 0 proved: no other instance of them is built
  } else {
    switch (split) {
      case 0: SL_CT(1, false, false);
      case 1: SL_CT(2, false, false);
      case 2: SL_CT(2, true, false);
      case 3: SL_CT(4, false, false);
      case 4: SL_CT(4, false, true);
      case 5: SL_CT(4, true, false);
      default: SL_CT(4, true, true);
    }
  }
#undef SL_CT
}

// blocks resident at once: 68 KiB of LDS per block for one W and its table, 136 KiB for two, of a CU's 160 KiB
int blocks_per_cu(int form) { return form == FORM_DUAL ? 1 : 2; }

int launch_conv_tail(int form, int split, const float* xa, const float* wa, const BnParams& bna, const float* other,
                     const float* wb, const BnParams& bnb, float* y, const int32_t* order, int64_t N, int64_t HW, hipStream_t st,
                     const char* who) {
  SL_REQUIRE(N >= 0 && HW >= 0, "%s: negative shape", who);
  SL_REQUIRE(split >= 0 && split < kSplits, "%s: split %d is not one of 0..%d", who, split, kSplits - 1);
  const int64_t total = N * kCo * HW;
  if (total == 0) return 0;
  SL_REQUIRE(total < kMaxTotal, "%s: %lld output elements exceed the supported maximum of 2^31 - 1", who, (long long)total);
  SL_REQUIRE(xa && wa && y && (form == FORM_CONV || other), "%s: null pointer", who);
  SL_REQUIRE(form == FORM_CONV || (bna.mean && bna.var && bna.scale && bna.bias), "%s: null pointer", who);
  SL_REQUIRE(form != FORM_DUAL || (wb && bnb.mean && bnb.var && bnb.scale && bnb.bias), "%s: null pointer", who);
  SL_REQUIRE((((uintptr_t)xa | (uintptr_t)y | (uintptr_t)other | (uintptr_t)wa | (uintptr_t)wb) & 15) == 0,
             "%s: tensors must be 16-byte aligned", who);
  const int64_t tiles = (HW + kTilePx - 1) / kTilePx, nwork = N * tiles;
  int64_t blocks = (nwork + kWaves - 1) / kWaves;
  const int64_t cap = (int64_t)num_cus() * blocks_per_cu(form);
  if (blocks > cap) blocks = cap;
  const dim3 grid((unsigned)blocks);
  const size_t lds = (size_t)(form == FORM_DUAL ? 2 : 1) * (kWFloats * 4 + (form == FORM_CONV ? 0 : kCo * sizeof(f4)));
  const uint32_t n = (uint32_t)N, hw = (uint32_t)HW, nt = (uint32_t)tiles;
  int rc;
  if (form == FORM_CONV) {  // no BatchNorm2d is evaluated: no record in the slot that counts them
    NoProf none;
    rc = HW % 4 == 0 ? launch_split<FORM_CONV, true>(split, none, grid, lds, st, xa, wa, bna, other, wb, bnb, y, order, n, hw, nt)
                     : launch_split<FORM_CONV, false>(split, none, grid, lds, st, xa, wa, bna, other, wb, bnb, y, order, n, hw, nt);
  } else {
    const double bytes = ((double)total + (double)N * kCi * HW * (form == FORM_DUAL ? 2 : 1) + (form == FORM_ADD_RELU ? (double)total : 0.0)) * 4;
    ProfScope prof(SL_PROF_BATCHNORM, st, bytes);
#define SL_CT_FORM(F_)                                                                                                           \
  rc = HW % 4 == 0 ? launch_split<F_, true>(split, prof, grid, lds, st, xa, wa, bna, other, wb, bnb, y, order, n, hw, nt)        \
                   : launch_split<F_, false>(split, prof, grid, lds, st, xa, wa, bna, other, wb, bnb, y, order, n, hw, nt)
    if (form == FORM_ADD_RELU)
      SL_CT_FORM(FORM_ADD_RELU);
    else
      SL_CT_FORM(FORM_DUAL);
#undef SL_CT_FORM
  }
  if (rc) return rc;
  SL_CHECK_HIP(hipGetLastError());
  if (form == FORM_DUAL) {  // the second BatchNorm2d of this call: an empty record, as sl_batchnorm_infer_add_bn_relu leaves
    ProfScope second(SL_PROF_BATCHNORM, st, 0.0);
    if (second.start) {
      SL_CHECK_HIP(hipEventRecord(second.start, st));
      SL_CHECK_HIP(hipEventRecord(second.stop, st));
    }
  }
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API int sl_conv1x1_64_256(const float* d_x, const float* d_w, int64_t N, int64_t HW, int split, const int32_t* d_korder,
                             float* d_y, void* stream) {
  return launch_conv_tail(FORM_CONV, split, d_x, d_w, BnParams{}, nullptr, nullptr, BnParams{}, d_y, d_korder, N, HW,
                          (hipStream_t)stream, "sl_conv1x1_64_256");
}

SL_API int sl_conv1x1_bn_add_relu(const float* d_x, const float* d_w, const float* d_mean, const float* d_var,
                                  const float* d_scale, const float* d_bias, double eps, const float* d_identity, int64_t N,
                                  int64_t HW, float* d_y, void* stream) {
  return launch_conv_tail(FORM_ADD_RELU, 0, d_x, d_w, BnParams{d_mean, d_var, d_scale, d_bias, eps}, d_identity, nullptr,
                          BnParams{}, d_y, nullptr, N, HW, (hipStream_t)stream, "sl_conv1x1_bn_add_relu");
}

SL_API int sl_conv1x1_bn_add_conv1x1_bn_relu(const float* d_xa, const float* d_wa, const float* d_mean_a, const float* d_var_a,
                                             const float* d_scale_a, const float* d_bias_a, double eps_a, const float* d_xb,
                                             const float* d_wb, const float* d_mean_b, const float* d_var_b,
                                             const float* d_scale_b, const float* d_bias_b, double eps_b, int64_t N, int64_t HW,
                                             float* d_y, void* stream) {
  return launch_conv_tail(FORM_DUAL, 0, d_xa, d_wa, BnParams{d_mean_a, d_var_a, d_scale_a, d_bias_a, eps_a}, d_xb, d_wb,
                          BnParams{d_mean_b, d_var_b, d_scale_b, d_bias_b, eps_b}, d_y, nullptr, N, HW, (hipStream_t)stream,
                          "sl_conv1x1_bn_add_conv1x1_bn_relu");
}
