// K11 — primitives of a native CLIP-family ViT tower.
//
// The reference's OpenClip.encode_image / encode_text (foundation_models/clip.py:103-135) only forward
// to the third-party open_clip model; its arithmetic is a standard pre-LN transformer:
//   tokens -> ln_pre -> L x [ x += out_proj(MHA(ln_1(x))) ; x += c_proj(gelu(c_fc(ln_2(x)))) ] -> ln_post -> proj
// These kernels run that tower in fp32 on the device: every linear layer is the fp32-input MFMA GEMM of
// gemm_f32.hpp with bias / GELU / residual (and, for the patch embedding, the token scatter + positional
// add) fused into its epilogue; LayerNorm, attention and patch extraction are small bandwidth-bound kernels.
// The orchestration (weights, layer loop) lives in semanticlens_amd/foundation_models/native_clip.py.
// Four units that compile side by side: the linear layers in encoder_linear.hip (fp32-input MFMA) and encoder_linear3.hip
// (split-bf16 x3) over the epilogue of encoder_epilogue.hpp, the attention family in encoder_attention.hip, and here the
// small kernels: LayerNorm, patch extraction, class-token broadcast, token embedding, tokens from a feature map.
#include "gemm_bf16x3.hpp"

namespace sl {
namespace {

using gemm3::split_kp;
using gemm3::store_split;   // (v, row, col, Kp, split matrix): see gemm_bf16x3.hpp for the layout
using gemm3::store_split4;

// ---- LayerNorm over the last dim: one wave per row -------------------------------------------------------------
// Fast path (J > 0: cols % 4 == 0, cols <= 256 J, 16-byte aligned rows): the row is read once into registers (up to J
// float4 per lane: J = 4 up to 1024 columns, J = 8 up to 2048 — SigLIP-so400m's 1152 took the three-pass path until round 4:
// 227 us per LayerNorm at 65 536 rows, 2.7 TB/s), mean and variance are two wave reductions, the result leaves as 16-byte
// fp32 stores or as 8-byte packed bf16 hi / lo stores.  J = 0: any shape, three passes over the (L1-resident) row.
template <int J>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ x, int64_t rows, int cols,
                                                         int64_t xs, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         float* __restrict__ out, int64_t os, uint16_t* __restrict__ osp) {
  const int64_t okp = split_kp(cols);  // split output: a (rows x cols) split matrix
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int64_t nw = (int64_t)gridDim.x * 4;
  if constexpr (J > 0) {
    const int nq = cols >> 2;  // float4 chunks per row, <= 64 J
    // gamma / beta: in registers for J = 4 (32 of 83); for J = 8 they would be 64 of 147 registers (three waves per SIMD, 55 KB
    // of loads in flight per CU: 4.2 TB/s at so400m's 1152 columns) — there the workgroup keeps them in LDS instead
    constexpr bool kLds = J > 4;
    __shared__ float4 s_g[kLds ? 64 * J : 1], s_b[kLds ? 64 * J : 1];
    float4 g[kLds ? 1 : J], bt[kLds ? 1 : J];
    if constexpr (kLds) {
      for (int q = threadIdx.x; q < 64 * J; q += 256) {
        s_g[q] = q < nq ? reinterpret_cast<const float4*>(gamma)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        s_b[q] = q < nq ? reinterpret_cast<const float4*>(beta)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      __syncthreads();
    } else {
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int q = lane + 64 * j;
        g[j] = q < nq ? reinterpret_cast<const float4*>(gamma)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        bt[j] = q < nq ? reinterpret_cast<const float4*>(beta)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    for (int64_t r = wave; r < rows; r += nw) {
      const float4* p = reinterpret_cast<const float4*>(x + r * xs);
      float4 v[J];
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int q = lane + 64 * j;
        v[j] = q < nq ? p[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
      }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      const float mean = s / (float)cols;
      float var = 0.f;
#pragma unroll
      for (int j = 0; j < J; ++j) {
        if (lane + 64 * j < nq) {
          const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
          var += (a * a + b * b) + (c * c + d * d);
        }
      }
      for (int off = 32; off > 0; off >>= 1) var += __shfl_xor(var, off, 64);
      const float rstd = 1.f / sqrtf(var / (float)cols + eps);
#pragma unroll
      for (int j = 0; j < J; ++j) {
        const int q = lane + 64 * j;
        if (q < nq) {
          const float4 gj = kLds ? s_g[q] : g[kLds ? 0 : j], bj = kLds ? s_b[q] : bt[kLds ? 0 : j];
          const float4 y = make_float4((v[j].x - mean) * rstd * gj.x + bj.x, (v[j].y - mean) * rstd * gj.y + bj.y,
                                       (v[j].z - mean) * rstd * gj.z + bj.z, (v[j].w - mean) * rstd * gj.w + bj.w);
          if (out) *reinterpret_cast<float4*>(out + r * os + q * 4) = y;
          if (osp) store_split4(y, r, q * 4, okp, osp);
        }
      }
    }
    return;
  }
  for (int64_t r = wave; r < rows; r += nw) {
    const float* p = x + r * xs;
    float s = 0.f;
    for (int i = lane; i < cols; i += 64) s += p[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)cols;
    float v = 0.f;
    for (int i = lane; i < cols; i += 64) {
      const float d = p[i] - mean;
      v += d * d;
    }
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const float rstd = 1.f / sqrtf(v / (float)cols + eps);
    for (int i = lane; i < cols; i += 64) {
      const float y = (p[i] - mean) * rstd * gamma[i] + beta[i];
      if (out) out[r * os + i] = y;
      if (osp) store_split(y, r, i, okp, osp);
    }
  }
}
// ---- patch extraction: (B, C, Hi, Wi) -> (B * gh * gw, C * P * P), k = c*P*P + py*P + px (conv weight order) --
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ img, int64_t B, int C, int Hi, int Wi,
                                                        int P, float* __restrict__ out, uint16_t* __restrict__ osp) {
  const int gh = Hi / P, gw = Wi / P;
  const int64_t kdim = (int64_t)C * P * P;
  const int64_t total4 = B * gh * gw * kdim / 4;  // P % 4 == 0
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t idx = e * 4;
    const int64_t row = idx / kdim;
    const int k = (int)(idx % kdim);
    const int c = k / (P * P), py = (k / P) % P, px = k % P;
    const int64_t bb = row / (gh * gw);
    const int pr = (int)(row % (gh * gw));
    const int gy = pr / gw, gx = pr % gw;
    const float* src = img + ((bb * C + c) * Hi + gy * P + py) * (int64_t)Wi + gx * P + px;
    const float4 v = *reinterpret_cast<const float4*>(src);
    if (out) reinterpret_cast<float4*>(out)[e] = v;
    if (osp) store_split4(v, row, k, split_kp(kdim), osp);
  }
}

// any patch size (14 x 14 of ViT-L/14 and SigLIP-so400m): one element per thread
__global__ __launch_bounds__(256) void patchify_scalar_kernel(const float* __restrict__ img, int64_t B, int C, int Hi, int Wi,
                                                               int P, float* __restrict__ out, uint16_t* __restrict__ osp) {
  const int gh = Hi / P, gw = Wi / P;
  const int64_t kdim = (int64_t)C * P * P;
  const int64_t total = B * gh * gw * kdim;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = idx / kdim;
    const int k = (int)(idx % kdim);
    const int c = k / (P * P), py = (k / P) % P, px = k % P;
    const int64_t bb = row / (gh * gw);
    const int pr = (int)(row % (gh * gw));
    const int gy = pr / gw, gx = pr % gw;
    const float v = img[((bb * C + c) * Hi + gy * P + py) * (int64_t)Wi + gx * P + px];
    if (out) out[idx] = v;
    if (osp) store_split(v, row, k, split_kp(kdim), osp);
  }
}

// out[g * gstride + row] = v[:] (+ add[:]) for every group g: the class token row of every image
__global__ __launch_bounds__(256) void broadcast_row_kernel(const float* __restrict__ v, const float* __restrict__ add,
                                                             int64_t G, int64_t gstride_elems, int N,
                                                             float* __restrict__ out) {
  const int64_t total = G * N;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = e / N;
    const int c = (int)(e % N);
    out[g * gstride_elems + c] = v[c] + (add ? add[c] : 0.f);
  }
}

// token embedding lookup + positional embedding: out[b][t][:] = table[ids[b][t]][:] + pos[t][:]
__global__ __launch_bounds__(256) void embed_tokens_kernel(const float* __restrict__ table, int64_t vocab,
                                                            const int64_t* __restrict__ ids, int64_t B, int T, int W,
                                                            const float* __restrict__ pos, float* __restrict__ out) {
  const int64_t total = B * T * (int64_t)W;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(e % W);
    const int64_t bt = e / W;
    const int t = (int)(bt % T);
    int64_t id = ids[bt];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    out[e] = table[id * W + c] + pos[(int64_t)t * W + c];
  }
}
// CLIP-ResNet attention pool input (open_clip ModifiedResNet.attnpool, foundation_models/clip.py:52-62 `OpenClip("RN50", ...)`):
// tokens[b][0][c] = mean_s map[b][c][s] + pos[0][c], tokens[b][1 + s][c] = map[b][c][s] + pos[1 + s][c] — the NCHW trunk output
// turned into (B, S + 1, C) token rows.  One workgroup per (b, 64-channel block): the (64 x S) tile goes through LDS so that both
// the reads (s contiguous) and the writes (c contiguous) are coalesced.
__global__ __launch_bounds__(256) void tokens_from_map_kernel(const float* __restrict__ map, const float* __restrict__ pos, int C, int S,
                                                              float* __restrict__ out) {
  extern __shared__ float s_tile[];  // 64 x (S + 1)
  const int ld = S + 1;
  const int64_t b = blockIdx.y;
  const int c0 = blockIdx.x * 64;
  const int nc = C - c0 < 64 ? C - c0 : 64;
  const float* src = map + (b * C + c0) * (int64_t)S;
  for (int i = threadIdx.x; i < nc * S; i += 256) s_tile[(i / S) * ld + (i % S)] = src[i];
  __syncthreads();
  if ((int)threadIdx.x < nc) {  // the mean token: fp32 sum in index order, then / S (torch: x.mean(dim=0))
    float acc = 0.f;
    for (int s = 0; s < S; ++s) acc += s_tile[threadIdx.x * ld + s];
    s_tile[threadIdx.x * ld + S] = acc / (float)S;
  }
  __syncthreads();
  float* dst = out + b * (int64_t)(S + 1) * C + c0;
  for (int i = threadIdx.x; i < 64 * (S + 1); i += 256) {
    const int t = i / 64, c = i % 64;  // t = 0: mean token
    if (c < nc) dst[(int64_t)t * C + c] = s_tile[c * ld + (t == 0 ? S : t - 1)] + pos[(int64_t)t * C + c0 + c];
  }
}

int64_t grid_for(int64_t items) {
  int64_t blocks = (items + 255) / 256;
  const int64_t cap = (int64_t)num_cus() * 16;
  if (blocks > cap) blocks = cap;
  return blocks < 1 ? 1 : blocks;
}

}  // namespace
}  // namespace sl

using namespace sl;
SL_API int sl_layernorm(const float* d_x, int64_t rows, int64_t cols, int64_t x_row_stride, const float* d_gamma,
                        const float* d_beta, float eps, float* d_out, uint16_t* d_out_split, int64_t out_row_stride,
                        void* stream) {
  SL_REQUIRE(rows >= 0 && cols >= 1 && cols < (1 << 30), "sl_layernorm: bad shape");
  if (rows == 0) return 0;
  SL_REQUIRE(d_x && d_gamma && d_beta && (d_out || d_out_split), "sl_layernorm: null pointer");
  int64_t blocks = (rows + 3) / 4;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (blocks > cap) blocks = cap;
  const uintptr_t ptrs = (uintptr_t)d_x | (uintptr_t)d_gamma | (uintptr_t)d_beta | (uintptr_t)d_out | (uintptr_t)d_out_split;
  const bool fast = cols % 4 == 0 && cols <= 2048 && x_row_stride % 4 == 0 && out_row_stride % 4 == 0 && (ptrs & 15) == 0;
  const auto kernel = !fast ? layernorm_kernel<0> : cols <= 1024 ? layernorm_kernel<4> : layernorm_kernel<8>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_x, rows, (int)cols, x_row_stride, d_gamma,
                     d_beta, eps, d_out, out_row_stride, d_out_split);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
SL_API int sl_tokens_from_map(const float* d_map, int64_t B, int64_t C, int64_t S, const float* d_pos, float* d_out, void* stream) {
  SL_REQUIRE(B >= 0 && C >= 1 && S >= 1, "sl_tokens_from_map: bad shape");
  if (B == 0) return 0;
  SL_REQUIRE(d_map && d_pos && d_out, "sl_tokens_from_map: null pointer");
  const size_t lds = (size_t)64 * (S + 1) * sizeof(float);
  // the (64 channels x S positions) tile lives in LDS: S is bounded by the 160 KiB a gfx950 workgroup may declare (S <= 639)
  SL_REQUIRE(B < 65536 && lds <= 160 * 1024, "sl_tokens_from_map: B=%lld S=%lld (limits 65535 / %d: the 64 x (S + 1) fp32 tile must fit the LDS)",
             (long long)B, (long long)S, (int)(160 * 1024 / (64 * sizeof(float)) - 1));
  if (lds > 64 * 1024)
    SL_CHECK_HIP(hipFuncSetAttribute((const void*)tokens_from_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(tokens_from_map_kernel, dim3((unsigned)((C + 63) / 64), (unsigned)B), dim3(256), lds, (hipStream_t)stream, d_map, d_pos,
                     (int)C, (int)S, d_out);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_patchify(const float* d_img, int64_t B, int64_t C, int64_t Hi, int64_t Wi, int64_t P, float* d_out,
                       uint16_t* d_out_split, void* stream) {
  SL_REQUIRE(B >= 0 && C >= 1 && P >= 1 && Hi % P == 0 && Wi % P == 0, "sl_patchify: bad geometry");
  if (B == 0) return 0;
  SL_REQUIRE(d_img && (d_out || d_out_split), "sl_patchify: null pointer");
  if (P % 4 == 0 && (((uintptr_t)d_img | (uintptr_t)d_out) & 15) == 0 && Wi % 4 == 0) {  // 16-byte pieces
    const int64_t total4 = B * C * Hi * Wi / 4;
    hipLaunchKernelGGL(patchify_kernel, dim3((unsigned)grid_for(total4)), dim3(256), 0, (hipStream_t)stream, d_img, B, (int)C,
                       (int)Hi, (int)Wi, (int)P, d_out, d_out_split);
  } else {
    hipLaunchKernelGGL(patchify_scalar_kernel, dim3((unsigned)grid_for(B * C * Hi * Wi)), dim3(256), 0, (hipStream_t)stream, d_img,
                       B, (int)C, (int)Hi, (int)Wi, (int)P, d_out, d_out_split);
  }
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_broadcast_row(const float* d_v, const float* d_add, int64_t G, int64_t group_stride_elems, int64_t N,
                            float* d_out, void* stream) {
  SL_REQUIRE(G >= 0 && N >= 1, "sl_broadcast_row: bad shape");
  if (G == 0) return 0;
  SL_REQUIRE(d_v && d_out, "sl_broadcast_row: null pointer");
  hipLaunchKernelGGL(broadcast_row_kernel, dim3((unsigned)grid_for(G * N)), dim3(256), 0, (hipStream_t)stream, d_v, d_add, G,
                     group_stride_elems, (int)N, d_out);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_embed_tokens(const float* d_table, int64_t vocab, const int64_t* d_ids, int64_t B, int64_t T, int64_t W,
                           const float* d_pos, float* d_out, void* stream) {
  SL_REQUIRE(B >= 0 && T >= 1 && W >= 1 && vocab >= 1, "sl_embed_tokens: bad shape");
  if (B == 0) return 0;
  SL_REQUIRE(d_table && d_ids && d_pos && d_out, "sl_embed_tokens: null pointer");
  hipLaunchKernelGGL(embed_tokens_kernel, dim3((unsigned)grid_for(B * T * W)), dim3(256), 0, (hipStream_t)stream, d_table,
                     vocab, d_ids, B, (int)T, (int)W, d_pos, d_out);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
