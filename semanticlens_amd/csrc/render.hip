// K13 — concept-conditional heatmap rendering (utils/render.py:13-341) and the start relevance of a
// conditional backward (zennit-crp's CondAttribution with a channel condition).
//
// sl_render_heatmaps: one workgroup per image runs the whole per-image chain of the reference's three plot
// functions — channel sum, separable Gaussian blur with reflect padding (torchvision gaussian_blur), |b| / max
// normalisation, crop range + square box, the crop decision, the composite, min-max `imgify` and the one-pixel
// stroke of `mystroke` + two Pillow pastes — and writes the uint8 canvas with the crop at its top-left.  The
// blur's two planes live in a caller-provided workspace (2 x H x W fp32 per image, L2-resident while the block
// works on them); both passes are tiled through LDS.  Every other step is a sweep over the plane with
// block-level reductions in between.  Rules restated in DESIGN.md §K13.
//
// K14 (sl_activation_heat_boxes, sl_heat_boxes): the CROP-style box alone, one workgroup per (sample, component) pair,
// no image and no canvas.  The activation form upsamples the layer's low-resolution channel map straight into the
// horizontal blur pass (the full-resolution heat reaches global memory only when asked for).  DESIGN.md §K14.
#include "common.hpp"

namespace sl {
namespace {

constexpr int kThreads = 1024;  // 16 waves per image: the tap loops are LDS-latency bound, more waves hide it
constexpr int kTile = 16384;     // fp32 elements of the LDS tile shared by both blur passes (64 KB)
constexpr int kTileCols = 64;    // column strip of the vertical pass: one lane per column
constexpr int kMaxKernel = 255;  // kernel_size limit: the vertical tile needs kernel_size - 1 halo rows + 1

__device__ inline int reflect_index(int x, int n) { return x < 0 ? -x : (x >= n ? 2 * (n - 1) - x : x); }

__device__ inline float block_max(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__device__ inline float block_min(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fminf(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

__device__ inline float block_sum(float v, float* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

template <bool MAX>
__device__ inline int block_ext_i(int v, int* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = MAX ? max(red[threadIdx.x], red[threadIdx.x + s]) : min(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  const int r = red[0];
  __syncthreads();
  return r;
}

// The composited value of one channel: CROP none, OPAQUE img*m + img*!m*alpha, LIGHTEN img*m + (img*(1-alpha) + alpha)*!m
// (render.py:122, 208).  Separate roundings (no contraction), as torch evaluates them op by op.
__device__ inline float composite(float v, bool m, int style, float alpha, float one_minus_alpha) {
  if (style == SL_RENDER_OPAQUE) return m ? v : __fmul_rn(v, alpha);
  if (style == SL_RENDER_LIGHTEN) return m ? v : __fadd_rn(__fmul_rn(v, one_minus_alpha), alpha);
  return v;
}

// 1-D kernel of torchvision's _get_gaussian_kernel1d: x = -r..r, pdf = exp(-0.5 (x / sigma)^2), pdf / sum(pdf),
// sigma = 0.15 k + 0.35 (its default), all in fp32
__device__ inline void gaussian_taps(int ksize, float* taps, float* redf) {
  const int tid = threadIdx.x, r = ksize / 2;
  const float sigma = (float)(0.15 * ksize + 0.35);
  if (tid < ksize) {
    const float q = (float)(tid - r) / sigma;
    taps[tid] = expf(-0.5f * (q * q));
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
    for (int t = 0; t < ksize; ++t) s += taps[t];
    redf[0] = s;
  }
  __syncthreads();
  const float tsum = redf[0];
  __syncthreads();
  if (tid < ksize) taps[tid] = taps[tid] / tsum;
  __syncthreads();
}

// Separable blur of an H x W plane with reflect padding into `bl`, through `hb` (both global, L2-resident while the block
// works on them).  `heat(y, x)` yields the unblurred value at (y, x) and is called exactly once per padded tile element:
// the horizontal pass reads its rows reflect-padded into LDS, the vertical pass a 64-column strip of TH output rows plus
// 2r reflected halo rows.
template <class Heat>
__device__ inline void blur_plane(const Heat& heat, int H, int W, int ksize, const float* taps, float* tile, float* hb, float* bl) {
  const int tid = threadIdx.x, r = ksize / 2;
  const int PW = W + 2 * r;
  const int rows_per_tile = kTile / PW;
  for (int h0 = 0; h0 < H; h0 += rows_per_tile) {
    const int nr = min(rows_per_tile, H - h0);
    for (int e = tid; e < nr * PW; e += kThreads) {
      const int row = e / PW, x = e - row * PW;
      tile[e] = heat(h0 + row, reflect_index(x - r, W), x >= r && x < r + W);
    }
    __syncthreads();
    for (int e = tid; e < nr * W; e += kThreads) {
      const int row = e / W, w = e - row * W;
      const float* p = tile + row * PW + w;
      float acc = 0.f;
      for (int t = 0; t < ksize; ++t) acc += taps[t] * p[t];
      hb[(int64_t)(h0 + row) * W + w] = acc;
    }
    __syncthreads();
  }

  const int TH = kTile / kTileCols - 2 * r;
  const int lane = tid & (kTileCols - 1), phase = tid / kTileCols;
  for (int c0 = 0; c0 < W; c0 += kTileCols) {
    const int nc = min(kTileCols, W - c0);
    for (int h0 = 0; h0 < H; h0 += TH) {
      const int nh = min(TH, H - h0), rows = nh + 2 * r;
      for (int e = tid; e < rows * kTileCols; e += kThreads) {
        const int i = e / kTileCols, cw = e - i * kTileCols;
        tile[e] = cw < nc ? hb[(int64_t)reflect_index(h0 - r + i, H) * W + c0 + cw] : 0.f;
      }
      __syncthreads();
      if (lane < nc) {
        for (int j = phase; j < nh; j += kThreads / kTileCols) {
          const float* p = tile + j * kTileCols + lane;
          float acc = 0.f;
          for (int t = 0; t < ksize; ++t) acc += taps[t] * p[t * kTileCols];
          bl[(int64_t)(h0 + j) * W + c0 + lane] = acc;
        }
      }
      __syncthreads();
    }
  }
}

// crp get_crop_range: min / max row and column above crop_th (rmax < 0: none), the max used as an exclusive slice end; the
// full image when nothing exceeds crop_th or when both extents are empty.  Then _get_square_crop_box (render.py:13-33).
__device__ inline void square_box(int rmin, int rmax, int cmin, int cmax, int H, int W, int* box) {
  int row1 = rmin, row2 = rmax, col1 = cmin, col2 = cmax;
  if (rmax < 0 || (row1 >= row2 && col1 >= col2)) row1 = 0, row2 = H, col1 = 0, col2 = W;
  const int dr = row2 - row1, dc = col2 - col1;
  if (dr > dc) {
    col1 -= (dr - dc) / 2;
    col2 += (dr - dc) / 2;
    if (col1 < 0) col2 -= col1, col1 = 0;
  } else if (dc > dr) {
    row1 -= (dc - dr) / 2;
    row2 += (dc - dr) / 2;
    if (row1 < 0) row2 -= row1, row1 = 0;
  }
  box[0] = row1, box[1] = row2, box[2] = col1, box[3] = col2;
}

// heat = d_rel[b].sum(0) at one pixel (crp's attr.heatmap)
struct ChannelSumHeat {
  const float* relb;
  int64_t Cin, HW;
  int W;
  __device__ float operator()(int y, int x, bool) const {
    const int64_t src = (int64_t)y * W + x;
    float s = 0.f;
    for (int64_t c = 0; c < Cin; ++c) s += relb[c * HW + src];
    return s;
  }
};

__global__ __launch_bounds__(kThreads) void render_kernel(const float* __restrict__ rel, int64_t Cin, const float* __restrict__ img,
                                                          int H, int W, int ksize, float vis_th, float crop_th, float alpha,
                                                          float one_minus_alpha, int style, int rf, float* __restrict__ ws,
                                                          float* __restrict__ out_heat, int32_t* __restrict__ out_box,
                                                          int32_t* __restrict__ out_flags, uint8_t* __restrict__ out_rgb) {
  __shared__ float tile[kTile];
  __shared__ float taps[kMaxKernel + 1];
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  __shared__ int sbox[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  float* hb = ws + (int64_t)b * 2 * HW;  // horizontal pass
  float* bl = hb + HW;                   // blurred, then normalised in place
  const float* relb = rel + (int64_t)b * Cin * HW;
  const float* imgb = img + (int64_t)b * 3 * HW;

  gaussian_taps(ksize, taps, redf);
  blur_plane(ChannelSumHeat{relb, Cin, HW, W}, H, W, ksize, taps, tile, hb, bl);

  // ---- normalisation: |b| / (max|b| + 1e-8) (OPAQUE, LIGHTEN) or |b| / max|b| (CROP: 0/0 = NaN for an all-zero heat)
  float m = 0.f;
  for (int64_t i = tid; i < HW; i += kThreads) m = fmaxf(m, fabsf(bl[i]));
  const float mx = block_max(m, redf);
  const float den = style == SL_RENDER_CROP ? mx : mx + 1e-8f;
  int rmin = INT32_MAX, rmax = -1, cmin = INT32_MAX, cmax = -1;
  for (int64_t i = tid; i < HW; i += kThreads) {
    const float n = fabsf(bl[i]) / den;
    bl[i] = n;
    if (out_heat) out_heat[(int64_t)b * HW + i] = n;
    if (n > crop_th) {
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      rmin = min(rmin, y), rmax = max(rmax, y), cmin = min(cmin, x), cmax = max(cmax, x);
    }
  }
  rmin = block_ext_i<false>(rmin, redi);
  rmax = block_ext_i<true>(rmax, redi);
  cmin = block_ext_i<false>(cmin, redi);
  cmax = block_ext_i<true>(cmax, redi);
  if (tid == 0) {
    square_box(rmin, rmax, cmin, cmax, H, W, sbox);
    int32_t* ob = out_box + (int64_t)b * 4;
    ob[0] = sbox[0], ob[1] = sbox[1], ob[2] = sbox[2], ob[3] = sbox[3];
  }
  __syncthreads();
  // the box as a slice: the high ends clamp to the image (Python slicing)
  const int br0 = sbox[0], br1 = min(sbox[1], H), bc0 = sbox[2], bc1 = min(sbox[3], W);

  // ---- crop decision: CROP always; OPAQUE / LIGHTEN with rf when the cropped image and the cropped mask each have a
  // non-zero sum (render.py:110-119, 198-205)
  bool crop = style == SL_RENDER_CROP;
  if (style != SL_RENDER_CROP && rf) {
    const int bh = max(br1 - br0, 0), bw = max(bc1 - bc0, 0);
    float s = 0.f;
    int cnt = 0;
    for (int e = tid; e < bh * bw; e += kThreads) {
      const int y = br0 + e / bw, x = bc0 + e % bw;
      const int64_t i = (int64_t)y * W + x;
      s += imgb[i] + imgb[HW + i] + imgb[2 * HW + i];
      cnt += bl[i] > vis_th;
    }
    s = block_sum(s, redf);
    cnt = block_ext_i<true>(cnt > 0, redi);
    crop = s != 0.f && cnt != 0;
  }
  const int y0 = crop ? br0 : 0, y1 = crop ? br1 : H, x0 = crop ? bc0 : 0, x1 = crop ? bc1 : W;
  const int hc = max(y1 - y0, 0), wc = max(x1 - x0, 0);

  // ---- composite: min / max over the cropped image (imgify's bounds) and whether any pixel is masked
  float lo = INFINITY, hi = -INFINITY;
  int any = 0;
  for (int e = tid; e < hc * wc; e += kThreads) {
    const int y = y0 + e / wc, x = x0 + e % wc;
    const int64_t i = (int64_t)y * W + x;
    const bool mk = bl[i] > vis_th;
    any |= mk;
    for (int ch = 0; ch < 3; ++ch) {
      const float v = composite(imgb[ch * HW + i], mk, style, alpha, one_minus_alpha);
      lo = fminf(lo, v), hi = fmaxf(hi, v);
    }
  }
  lo = block_min(lo, redf);
  hi = block_max(hi, redf);
  any = block_ext_i<true>(any, redi);
  if (tid == 0) out_flags[b] = (crop ? 1 : 0) | (any ? 2 : 0);

  // ---- imgify + stroke: u = trunc(clip((v - lo) / (hi - lo) * 255, 0, 255)) (0 for a constant image); an unmasked
  // pixel with a masked 4-neighbour inside the crop carries the stroke: u' = (u * 75 + 128 + ((u * 75 + 128) >> 8)) >> 8
  const float range = __fsub_rn(hi, lo);
  uint8_t* outb = out_rgb + (int64_t)b * HW * 3;
  for (int e = tid; e < hc * wc; e += kThreads) {
    const int yy = e / wc, xx = e % wc, y = y0 + yy, x = x0 + xx;
    const int64_t i = (int64_t)y * W + x;
    const bool mk = bl[i] > vis_th;
    bool stroke = false;
    if (style != SL_RENDER_CROP && !mk)
      stroke = (y > y0 && bl[i - W] > vis_th) || (y + 1 < y1 && bl[i + W] > vis_th) || (x > x0 && bl[i - 1] > vis_th) ||
               (x + 1 < x1 && bl[i + 1] > vis_th);
    uint8_t* o = outb + ((int64_t)yy * W + xx) * 3;
    for (int ch = 0; ch < 3; ++ch) {
      const float v = composite(imgb[ch * HW + i], mk, style, alpha, one_minus_alpha);
      unsigned u = 0;
      if (range > 0.f) {
        const float s = __fmul_rn(__fdiv_rn(__fsub_rn(v, lo), range), 255.f);
        u = s >= 255.f ? 255u : (s > 0.f ? (unsigned)s : 0u);
      }
      if (stroke) {
        const unsigned t = u * 75u + 128u;
        u = (t + (t >> 8)) >> 8;
      }
      o[ch] = (uint8_t)u;
    }
  }
}

// R[i, c_i, :] for one row i per block; rf: only the first argmax position of a[i, c_i, :] keeps its value.
__global__ __launch_bounds__(kThreads) void condition_init_kernel(const float* __restrict__ act, int64_t C, int64_t S, int64_t sb,
                                                                  int64_t sc, int64_t ss, const int64_t* __restrict__ channels,
                                                                  int rf, float* __restrict__ out, int64_t ob, int64_t oc,
                                                                  int64_t os) {
  __shared__ float rv[kThreads];
  __shared__ int64_t ri[kThreads];
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x;
  const int64_t c = channels[i];
  const bool valid = c >= 0 && c < C;  // an out-of-range channel leaves its row all zero (the host refuses it first)
  const float* a = act + i * sb + (valid ? c : 0) * sc;
  int64_t p = -1;
  if (rf && valid) {
    // torch.argmax: NaN is the largest value, ties (-0 == +0 included) go to the first index
    float best = -INFINITY;
    int64_t bi = INT64_MAX;
    for (int64_t s = tid; s < S; s += kThreads) {
      const float v = a[s * ss];
      const bool take = bi == INT64_MAX || (isnan(v) && !isnan(best)) || (!isnan(best) && v > best);
      if (take) best = v, bi = s;
    }
    rv[tid] = best, ri[tid] = bi;
    __syncthreads();
    for (int st = kThreads / 2; st > 0; st >>= 1) {
      if (tid < st) {
        const float va = rv[tid], vb = rv[tid + st];
        const int64_t ia = ri[tid], ib = ri[tid + st];
        const bool na = isnan(va), nb = isnan(vb);
        bool take_b;
        if (ib == INT64_MAX) take_b = false;
        else if (ia == INT64_MAX) take_b = true;
        else if (na != nb) take_b = nb;
        else if (!na && va != vb) take_b = vb > va;
        else take_b = ib < ia;
        if (take_b) rv[tid] = vb, ri[tid] = ib;
      }
      __syncthreads();
    }
    p = ri[0];
  }
  const int64_t n = C * S;
  for (int64_t e = tid; e < n; e += kThreads) {
    const int64_t cc = e / S, s = e - cc * S;
    float v = 0.f;
    if (valid && cc == c && (!rf || s == p)) v = a[s * ss];
    out[i * ob + cc * oc + s * os] = v;
  }
}

// ---- K14: the CROP-style box of a heat plane without a canvas ---------------------------------------------------------------

// positive part of channel c of row u of a (B, C, S) strided layer output, bilinearly upsampled to H x W with ATen's fp32
// arithmetic of F.interpolate(mode="bilinear", align_corners=False); S position prefix + gy * gw + gx.  a == nullptr: an
// all-zero map.  The unblurred value is also written to `out` (if any) on the call for its unpadded position.
struct UpsampledActHeat {
  const float* a;
  int64_t ss;
  int gh, gw;
  float sh, sw;
  float* out;
  int W;
  __device__ float operator()(int y, int x, bool own) const {
    float v = 0.f;
    if (a) {
      const float hr = fmaxf(sh * ((float)y + 0.5f) - 0.5f, 0.f);
      const int h1 = min((int)hr, gh - 1), h1p = h1 < gh - 1 ? 1 : 0;
      const float h1l = hr - (float)h1, h0l = 1.f - h1l;
      const float wr = fmaxf(sw * ((float)x + 0.5f) - 0.5f, 0.f);
      const int w1 = min((int)wr, gw - 1), w1p = w1 < gw - 1 ? 1 : 0;
      const float w1l = wr - (float)w1, w0l = 1.f - w1l;
      const float* r0 = a + (int64_t)h1 * gw * ss;
      const float* r1 = a + (int64_t)(h1 + h1p) * gw * ss;
      // an axis of one cell has nothing to interpolate: ATen blends the cell with itself, l0 * a + l1 * a, a few ulp off a
      if (gh == 1 && gw == 1)
        v = r0[0];
      else if (gh == 1)
        v = w0l * r0[(int64_t)w1 * ss] + w1l * r0[(int64_t)(w1 + w1p) * ss];
      else if (gw == 1)
        v = h0l * r0[0] + h1l * r1[0];
      else
        v = h0l * (w0l * r0[(int64_t)w1 * ss] + w1l * r0[(int64_t)(w1 + w1p) * ss]) +
            h1l * (w0l * r1[(int64_t)w1 * ss] + w1l * r1[(int64_t)(w1 + w1p) * ss]);
      v = fmaxf(v, 0.f);
    }
    if (out && own) out[(int64_t)y * W + x] = v;
    return v;
  }
};

// one plane of a (P, H, W) heat, read as K13 reads a one-channel relevance (0 + v)
struct PlaneHeat {
  const float* p;
  int W;
  __device__ float operator()(int y, int x, bool) const { return 0.f + p[(int64_t)y * W + x]; }
};

// blurred plane -> |b| / max|b| -> crop range + square box, K13's CROP-style arithmetic (an all-zero plane: 0 / 0 = NaN, nothing
// exceeds crop_th, the full image)
__device__ inline void crop_box(const float* bl, int H, int W, float crop_th, float* redf, int* redi, int* sbox, int32_t* ob) {
  const int tid = threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  float m = 0.f;
  for (int64_t i = tid; i < HW; i += kThreads) m = fmaxf(m, fabsf(bl[i]));
  const float mx = block_max(m, redf);
  int rmin = INT32_MAX, rmax = -1, cmin = INT32_MAX, cmax = -1;
  for (int64_t i = tid; i < HW; i += kThreads) {
    if (fabsf(bl[i]) / mx > crop_th) {
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      rmin = min(rmin, y), rmax = max(rmax, y), cmin = min(cmin, x), cmax = max(cmax, x);
    }
  }
  rmin = block_ext_i<false>(rmin, redi);
  rmax = block_ext_i<true>(rmax, redi);
  cmin = block_ext_i<false>(cmin, redi);
  cmax = block_ext_i<true>(cmax, redi);
  if (tid == 0) {
    square_box(rmin, rmax, cmin, cmax, H, W, sbox);
    ob[0] = sbox[0], ob[1] = sbox[1], ob[2] = sbox[2], ob[3] = sbox[3];
  }
}

// one workgroup per pair j: row rows[j], channel channels[j] (out of range: an all-zero map; the host refuses it first)
__global__ __launch_bounds__(kThreads) void activation_heat_box_kernel(const float* __restrict__ act, int64_t B, int64_t C, int64_t sb,
                                                                       int64_t sc, int64_t ss, int64_t prefix, int gh, int gw,
                                                                       const int64_t* __restrict__ rows,
                                                                       const int64_t* __restrict__ channels, int H, int W, int ksize,
                                                                       float crop_th, float* __restrict__ ws,
                                                                       float* __restrict__ out_heat, int32_t* __restrict__ out_box) {
  __shared__ float tile[kTile];
  __shared__ float taps[kMaxKernel + 1];
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  __shared__ int sbox[4];
  const int64_t j = blockIdx.x, HW = (int64_t)H * W;
  const int64_t u = rows[j], c = channels[j];
  const bool valid = u >= 0 && u < B && c >= 0 && c < C;
  const UpsampledActHeat heat{valid ? act + u * sb + c * sc + prefix * ss : nullptr, ss, gh, gw, (float)gh / (float)H,
                              (float)gw / (float)W, out_heat ? out_heat + j * HW : nullptr, W};
  float* hb = ws + j * 2 * HW;
  gaussian_taps(ksize, taps, redf);
  blur_plane(heat, H, W, ksize, taps, tile, hb, hb + HW);
  crop_box(hb + HW, H, W, crop_th, redf, redi, sbox, out_box + j * 4);
}

__global__ __launch_bounds__(kThreads) void heat_box_kernel(const float* __restrict__ heat_in, int H, int W, int ksize, float crop_th,
                                                            float* __restrict__ ws, int32_t* __restrict__ out_box) {
  __shared__ float tile[kTile];
  __shared__ float taps[kMaxKernel + 1];
  __shared__ float redf[kThreads];
  __shared__ int redi[kThreads];
  __shared__ int sbox[4];
  const int64_t j = blockIdx.x, HW = (int64_t)H * W;
  float* hb = ws + j * 2 * HW;
  gaussian_taps(ksize, taps, redf);
  blur_plane(PlaneHeat{heat_in + j * HW, W}, H, W, ksize, taps, tile, hb, hb + HW);
  crop_box(hb + HW, H, W, crop_th, redf, redi, sbox, out_box + j * 4);
}

// K13's limits on the blur geometry, shared by both K14 entry points
int check_box_args(const char* fn, int64_t P, int64_t H, int64_t W, int kernel_size, float crop_th, size_t ws_bytes) {
  SL_REQUIRE(P >= 0 && H >= 1 && W >= 1 && H <= INT32_MAX / 2 && W <= INT32_MAX / 2, "%s: bad shape P=%lld H=%lld W=%lld", fn,
             (long long)P, (long long)H, (long long)W);
  SL_REQUIRE(kernel_size > 0 && kernel_size % 2 == 1, "%s: kernel_size must be an odd positive integer, got %d", fn, kernel_size);
  SL_REQUIRE(kernel_size / 2 < H && kernel_size / 2 < W, "%s: kernel_size // 2 = %d must be smaller than H and W (%lld x %lld) for reflect padding",
             fn, kernel_size / 2, (long long)H, (long long)W);
  if (kernel_size > kMaxKernel || W + 2 * (kernel_size / 2) > kTile) {
    set_error("%s: kernel_size %d with W %lld exceeds the supported maximum (kernel_size <= %d, W + kernel_size - 1 <= %d)", fn,
              kernel_size, (long long)W, kMaxKernel, kTile);
    return SL_E_UNSUPPORTED;
  }
  SL_REQUIRE(crop_th >= 0.f && crop_th < 1.f, "'crop_th' must be between [0, 1)");
  SL_REQUIRE(ws_bytes >= (size_t)P * 2 * (size_t)H * (size_t)W * sizeof(float), "%s: workspace too small (%zu < %zu bytes)", fn,
             ws_bytes, (size_t)P * 2 * (size_t)H * (size_t)W * sizeof(float));
  SL_REQUIRE(P <= INT32_MAX, "%s: P too large", fn);
  return 0;
}

}  // namespace
}  // namespace sl

using namespace sl;

SL_API size_t sl_render_ws_bytes(int64_t B, int64_t H, int64_t W) {
  if (B < 0 || H < 0 || W < 0) return 0;
  return (size_t)B * 2 * (size_t)H * (size_t)W * sizeof(float);
}

SL_API int sl_render_heatmaps(const float* d_rel, int64_t B, int64_t Cin, int64_t H, int64_t W, const float* d_img, int kernel_size,
                              float vis_th, float crop_th, double alpha, int style, int rf, float* d_heat, int32_t* d_box,
                              int32_t* d_flags, uint8_t* d_rgb, void* d_ws, size_t ws_bytes, void* stream) {
  SL_REQUIRE(d_rel && d_img && d_box && d_flags && d_rgb && d_ws, "sl_render_heatmaps: null pointer");
  SL_REQUIRE(B >= 0 && Cin >= 1 && H >= 1 && W >= 1 && H <= INT32_MAX / 2 && W <= INT32_MAX / 2,
             "sl_render_heatmaps: bad shape B=%lld Cin=%lld H=%lld W=%lld", (long long)B, (long long)Cin, (long long)H, (long long)W);
  SL_REQUIRE(kernel_size > 0 && kernel_size % 2 == 1, "sl_render_heatmaps: kernel_size must be an odd positive integer, got %d",
             kernel_size);
  SL_REQUIRE(kernel_size / 2 < H && kernel_size / 2 < W,
             "sl_render_heatmaps: kernel_size // 2 = %d must be smaller than H and W (%lld x %lld) for reflect padding",
             kernel_size / 2, (long long)H, (long long)W);
  if (kernel_size > kMaxKernel || W + 2 * (kernel_size / 2) > kTile) {
    set_error("sl_render_heatmaps: kernel_size %d with W %lld exceeds the supported maximum (kernel_size <= %d, W + kernel_size - 1 <= %d)",
              kernel_size, (long long)W, kMaxKernel, kTile);
    return SL_E_UNSUPPORTED;
  }
  // the reference's ValueError texts (render.py:92-97)
  SL_REQUIRE(alpha >= 0.0 && alpha <= 1.0, "'alpha' must be between [0, 1]");
  SL_REQUIRE(vis_th >= 0.f && vis_th < 1.f, "'vis_th' must be between [0, 1)");
  SL_REQUIRE(crop_th >= 0.f && crop_th < 1.f, "'crop_th' must be between [0, 1)");
  SL_REQUIRE(style == SL_RENDER_CROP || style == SL_RENDER_OPAQUE || style == SL_RENDER_LIGHTEN,
             "sl_render_heatmaps: unknown style %d", style);
  SL_REQUIRE(ws_bytes >= sl_render_ws_bytes(B, H, W), "sl_render_heatmaps: workspace too small (%zu < %zu bytes)", ws_bytes,
             sl_render_ws_bytes(B, H, W));
  if (B == 0) return 0;
  SL_REQUIRE(B <= INT32_MAX, "sl_render_heatmaps: B too large");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(render_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, d_rel, Cin, d_img, (int)H, (int)W, kernel_size, vis_th,
                     crop_th, (float)alpha, (float)(1.0 - alpha), style, rf ? 1 : 0, (float*)d_ws, d_heat, d_box, d_flags, d_rgb);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_condition_init(const float* d_act, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                             const int64_t* d_channels, int rf, float* d_out, int64_t ob, int64_t oc, int64_t os, void* stream) {
  SL_REQUIRE(d_act && d_channels && d_out, "sl_condition_init: null pointer");
  SL_REQUIRE(B >= 0 && C >= 1 && S >= 1, "sl_condition_init: bad shape B=%lld C=%lld S=%lld", (long long)B, (long long)C, (long long)S);
  if (B == 0) return 0;
  SL_REQUIRE(B <= INT32_MAX, "sl_condition_init: B too large");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(condition_init_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, d_act, C, S, sb, sc, ss, d_channels, rf ? 1 : 0,
                     d_out, ob, oc, os);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_activation_heat_boxes(const float* d_act, int64_t B, int64_t C, int64_t S, int64_t sb, int64_t sc, int64_t ss,
                                    int64_t prefix, int64_t gh, int64_t gw, const int64_t* d_rows, const int64_t* d_channels,
                                    int64_t P, int64_t H, int64_t W, int kernel_size, float crop_th, float* d_heat, int32_t* d_box,
                                    void* d_ws, size_t ws_bytes, void* stream) {
  SL_REQUIRE(d_act && d_rows && d_channels && d_box && d_ws, "sl_activation_heat_boxes: null pointer");
  SL_REQUIRE(B >= 1 && C >= 1 && S >= 1, "sl_activation_heat_boxes: bad shape B=%lld C=%lld S=%lld", (long long)B, (long long)C,
             (long long)S);
  SL_REQUIRE(gh >= 1 && gw >= 1 && prefix >= 0 && gh <= INT32_MAX / 2 && gw <= INT32_MAX / 2 && prefix + gh * gw <= S,
             "sl_activation_heat_boxes: prefix %lld + grid %lld x %lld does not fit S = %lld", (long long)prefix, (long long)gh,
             (long long)gw, (long long)S);
  const int rc = check_box_args("sl_activation_heat_boxes", P, H, W, kernel_size, crop_th, ws_bytes);
  if (rc) return rc;
  if (P == 0) return 0;
  hipLaunchKernelGGL(activation_heat_box_kernel, dim3((unsigned)P), dim3(kThreads), 0, (hipStream_t)stream, d_act, B, C, sb, sc, ss, prefix,
                     (int)gh, (int)gw, d_rows, d_channels, (int)H, (int)W, kernel_size, crop_th, (float*)d_ws, d_heat, d_box);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}

SL_API int sl_heat_boxes(const float* d_heat, int64_t P, int64_t H, int64_t W, int kernel_size, float crop_th, int32_t* d_box,
                         void* d_ws, size_t ws_bytes, void* stream) {
  SL_REQUIRE(d_heat && d_box && d_ws, "sl_heat_boxes: null pointer");
  const int rc = check_box_args("sl_heat_boxes", P, H, W, kernel_size, crop_th, ws_bytes);
  if (rc) return rc;
  if (P == 0) return 0;
  hipLaunchKernelGGL(heat_box_kernel, dim3((unsigned)P), dim3(kThreads), 0, (hipStream_t)stream, d_heat, (int)H, (int)W, kernel_size,
                     crop_th, (float*)d_ws, d_box);
  SL_CHECK_HIP(hipGetLastError());
  return 0;
}
