// The evaluation loops' epilogue on device (gfx950): what utils/estimate.py:49-129 and
// test_video_superresolution_by_patch.py:198-224 do per frame between `model(lr)` and their prints, after `.to('cpu')`:
//   baseline = interpolate(lr_each, (H, W), mode='bilinear'[, align_corners=True])            estimate.py:80,98,122
//   psnr(sr, hr), psnr_y(sr, hr), psnr(baseline, hr) with a shave, the Charbonnier `test loss`  :70,:102-104
//   save_image(x.clamp(0, 1)) of sr, baseline and hr                                            :84-86
//   total_variation / time_variation of the LR patch                                            by_patch.py:43-69
// Here the SR frames stay in HBM: one reduction launch per clip returns the four numbers PER FRAME, the baseline is blended
// in registers from its four LR taps and never stored in float, and the 8-bit frames are packed NCHW f32 -> NHWC uint8.
// Memory-bound reductions and a pack: plain HIP, no LDS beyond the 4-wave sum, no atomics (same input, same bits).
#pragma once
#include "sr_common.h"

namespace evalk {
// one axis of ATen's upsample_bilinear2d (UpSampleKernel.cpp, compute_source_index_and_lambda): sy, sx are
// area_pixel_compute_scale -- float(in) / float(out), or float(in - 1) / (out - 1) (0 when out == 1) with align_corners
struct Resize { float sy, sx; int h, w, align; };
struct Tap { int i0, i1; float l0, l1; };

// src = scale (d + 0.5) - 0.5 clamped at 0 (align_corners: scale d).  ATen's CPU kernels are built with contraction on and
// evaluate the first form as ONE fused multiply-add on every host with FMA units (tests/test_eval_ref_host.py holds the
// reference to torch's own interpolate); rounding the product on its own moves src by an ulp of src, i.e. l1 by up to
// 2^-24 * in, far more than the blend's roundings.  So the fma is written out, not left to the compiler's choice.
SR_DEV Tap tap(int d, float scale, int n, int align) {
#pragma clang fp contract(off)
  float src;
  if (align) {
    src = scale * (float)d;
  } else {
    src = __builtin_fmaf(scale, (float)d + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
  }
  Tap t;
  t.i0 = min((int)src, n - 1);
  t.i1 = min(t.i0 + 1, n - 1);
  t.l1 = fminf(fmaxf(src - (float)t.i0, 0.f), 1.f);
  t.l0 = 1.f - t.l1;
  return t;
}

// l0y (l0x a + l1x b) + l1y (l0x c + l1x d) on one LR plane [h][w]
SR_DEV float blend(const float* __restrict__ p, int w, const Tap& ty, const Tap& tx) {
  const float* r0 = p + (size_t)ty.i0 * w;
  const float* r1 = p + (size_t)ty.i1 * w;
  const float top = tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1];
  const float bot = tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1];
  return ty.l0 * top + ty.l1 * bot;
}

// common/metrics.py:13-14: (v * 255).round().clamp(0, 255) / 255, then clamp(0, 1), as csrc/metrics.h
SR_DEV float quant_psnr(float v) {
  return fminf(fmaxf(fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f) / 255.f, 0.f), 1.f);
}

// torchvision save_image: x.clamp(0, 1).mul(255).add_(0.5).clamp_(0, 255).to(uint8) -- product and sum rounded separately
SR_DEV unsigned quant_u8(float v) {
#pragma clang fp contract(off)
  const float s = fminf(fmaxf(v, 0.f), 1.f) * 255.f;
  const float r = s + 0.5f;
  return (unsigned)(int)fminf(fmaxf(r, 0.f), 255.f);
}

SR_DEV double wave_sum_f64(const float* __restrict__ p, int n, int stride, int lane) {
  double s = 0.0;
  for (int i = lane; i < n; i += 64) s += (double)p[(size_t)i * stride];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
  return s;
}
}  // namespace evalk

// sr, hr [F][3][H][W], lr [F][CL][h][w] (channels 0..2 used); grid (wgs, F).  The walk covers the UNSHAVED frame in groups of
// four pixels of a row (16-byte loads when `vec`: W % 4 == 0 and 16-byte aligned bases), each HR pixel once; sums (a)-(c)
// take the pixels inside the shave, (d) all.  partial [F][wgs][4] = {sq psnr, sq psnr_y, sq psnr(baseline), charbonnier}
__global__ __launch_bounds__(256) void eval_clip_kernel(const float* __restrict__ sr, const float* __restrict__ lr,
                                                        const float* __restrict__ hr, float* __restrict__ partial, int H, int W,
                                                        int CL, evalk::Resize rz, int shave, int vec) {
  __shared__ float red[4][4];
  const int f = blockIdx.y, G = (W + 3) >> 2, items = H * G;
  const size_t plane = (size_t)H * W, lplane = (size_t)rz.h * rz.w;
  const float* s = sr + (size_t)f * 3 * plane;
  const float* t = hr + (size_t)f * 3 * plane;
  const float* l = lr + (size_t)f * CL * lplane;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
    const int y = it / G, x0 = (it - y * G) << 2, npx = min(4, W - x0);
    const size_t o = (size_t)y * W + x0;
    float sv[3][4], tv[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (vec) {
        const float4 a = *reinterpret_cast<const float4*>(s + c * plane + o);
        const float4 b = *reinterpret_cast<const float4*>(t + c * plane + o);
        sv[c][0] = a.x; sv[c][1] = a.y; sv[c][2] = a.z; sv[c][3] = a.w;
        tv[c][0] = b.x; tv[c][1] = b.y; tv[c][2] = b.z; tv[c][3] = b.w;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          sv[c][j] = j < npx ? s[c * plane + o + j] : 0.f;
          tv[c][j] = j < npx ? t[c * plane + o + j] : 0.f;
        }
      }
    }
    const bool yin = y >= shave && y < H - shave;
    const evalk::Tap ty = evalk::tap(y, rz.sy, rz.h, rz.align);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < npx) {
        const int x = x0 + j;
        float dl[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d = sv[c][j] - tv[c][j];
          acc[3] += sqrtf(d * d + 1e-12f);
          dl[c] = fminf(fmaxf(sv[c][j], 0.f), 1.f) - tv[c][j];
        }
        if (yin && x >= shave && x < W - shave) {
          const evalk::Tap tx = evalk::tap(x, rz.sx, rz.w, rz.align);
          const float dy = 0.257f * dl[0] + 0.504f * dl[1] + 0.098f * dl[2];
          acc[1] += dy * dy;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float da = evalk::quant_psnr(sv[c][j]) - tv[c][j];
            const float db = evalk::quant_psnr(evalk::blend(l + c * lplane, rz.w, ty, tx)) - tv[c][j];
            acc[0] += da * da;
            acc[2] += db * db;
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc[k] += __shfl_xor(acc[k], m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < 4)
    partial[((size_t)f * gridDim.x + blockIdx.x) * 4 + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// out [4][F]: rows 0-2 = -10 log10(sum / count), row 3 = sum / count, sums in double.  One wave per frame, waves loop over
// the frames (F is not bounded by the block).  count == 0 (everything shaved): 0 / 0 = nan, as csrc/metrics.h
__global__ __launch_bounds__(256) void eval_clip_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int F, int wgs,
                                                               double n_shaved, double n_all) {
  const int lane = threadIdx.x & 63;
  for (int f = threadIdx.x >> 6; f < F; f += 4) {
    const float* p = partial + (size_t)f * wgs * 4;
    const double a = evalk::wave_sum_f64(p, wgs, 4, lane), b = evalk::wave_sum_f64(p + 1, wgs, 4, lane);
    const double c = evalk::wave_sum_f64(p + 2, wgs, 4, lane), d = evalk::wave_sum_f64(p + 3, wgs, 4, lane);
    if (lane == 0) {
      out[f] = (float)(-10.0 * log10(a / (3.0 * n_shaved)));
      out[(size_t)F + f] = (float)(-10.0 * log10(b / n_shaved));
      out[2 * (size_t)F + f] = (float)(-10.0 * log10(c / (3.0 * n_shaved)));
      out[3 * (size_t)F + f] = (float)(d / n_all);
    }
  }
}

// NCHW f32 -> NHWC uint8.  FROM_LR 0: src [F][3][H][W] as given; 1: src [F][CL][h][w], the bilinear baseline of its first three
// channels, blended in registers.  grid (blocks, F); an item is one 4-pixel group of a row, the groups aligned on the LINEAR
// pixel index of the output so that a whole group is 12 bytes at a 4-byte aligned address and goes out as one 3-dword store;
// a group cut by a row end (W % 4 != 0) writes its pixels byte by byte.  `vec` (FROM_LR 0): 16-byte loads, W % 4 == 0
template <int FROM_LR>
__global__ __launch_bounds__(256) void eval_u8_kernel(const float* __restrict__ src, unsigned char* __restrict__ out, int H, int W,
                                                      int CL, evalk::Resize rz, int vec) {
  struct alignas(4) Px4 { unsigned w0, w1, w2; };
  const int f = blockIdx.y, S = ((W + 2) >> 2) + 1, items = H * S;
  const size_t plane = FROM_LR ? (size_t)rz.h * rz.w : (size_t)H * W;
  const float* p = src + (size_t)f * (FROM_LR ? CL : 3) * plane;
  for (int it = blockIdx.x * 256 + threadIdx.x; it < items; it += gridDim.x * 256) {
    const int y = it / S, j = it - y * S;
    const size_t q0 = ((size_t)f * H + y) * W;                // linear pixel index of the row's first pixel
    const int x0 = 4 * j - (int)(q0 & 3);                     // the group's first pixel, relative to the row: -3 .. W + 2
    const int xa = max(x0, 0), xb = min(x0 + 4, W);           // its pixels inside the row
    if (xa >= xb) continue;
    unsigned b[4][3];
    evalk::Tap ty;
    if (FROM_LR) ty = evalk::tap(y, rz.sy, rz.h, rz.align);
    if (!FROM_LR && vec) {                                    // W % 4 == 0: q0 & 3 == 0, every group whole
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(p + c * plane + (size_t)y * W + x0);
        b[0][c] = evalk::quant_u8(v.x); b[1][c] = evalk::quant_u8(v.y); b[2][c] = evalk::quant_u8(v.z); b[3][c] = evalk::quant_u8(v.w);
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int x = x0 + k;
        if (x >= xa && x < xb) {
          evalk::Tap tx;
          if (FROM_LR) tx = evalk::tap(x, rz.sx, rz.w, rz.align);
#pragma unroll
          for (int c = 0; c < 3; ++c)
            b[k][c] = evalk::quant_u8(FROM_LR ? evalk::blend(p + c * plane, rz.w, ty, tx) : p[c * plane + (size_t)y * W + x]);
        } else {
          b[k][0] = b[k][1] = b[k][2] = 0u;
        }
      }
    }
    if (xb - xa == 4) {                                        // whole group: x0 >= 0 and (q0 + x0) % 4 == 0
      unsigned char* o = out + 3 * (q0 + (size_t)x0);
      Px4 v;
      v.w0 = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
      v.w1 = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
      v.w2 = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
      *reinterpret_cast<Px4*>(o) = v;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x0 + k >= xa && x0 + k < xb) {
          unsigned char* ok = out + 3 * (q0 + (size_t)(x0 + k));
          ok[0] = (unsigned char)b[k][0]; ok[1] = (unsigned char)b[k][1]; ok[2] = (unsigned char)b[k][2];
        }
    }
  }
}

// lr [B][N][C][h][w], frame f = b N + n; grid (wgs, B N).  partial [F][wgs][2] = {sum |down - x| + |right - x| with the last
// row / column replicated (F.pad(.., 'replicate'): those differences are 0), sum |x[n + 1] - x| (0 for the clip's last frame)}
__global__ __launch_bounds__(256) void eval_variation_kernel(const float* __restrict__ lr, float* __restrict__ partial, int N, int C,
                                                             int h, int w) {
  __shared__ float red[4][2];
  const int f = blockIdx.y, total = C * h * w;
  const float* p = lr + (size_t)f * total;
  const bool has_next = f % N < N - 1;
  float tv = 0.f, dt = 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int row = i / w, x = i - row * w, y = row % h;
    const float v = p[i];
    const float r = x < w - 1 ? p[i + 1] : v;
    const float d = y < h - 1 ? p[i + w] : v;
    tv += fabsf(d - v) + fabsf(r - v);
    if (has_next) dt += fabsf(p[(size_t)total + i] - v);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { tv += __shfl_xor(tv, m); dt += __shfl_xor(dt, m); }
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = tv; red[threadIdx.x >> 6][1] = dt; }
  __syncthreads();
  if (threadIdx.x < 2)
    partial[((size_t)f * gridDim.x + blockIdx.x) * 2 + threadIdx.x] =
        red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// out [2][B N]: row 0 total_variation, row 1 time_variation = d[n] + d[n - 1] (each where it exists), doubled at n == 0 and at
// n == N - 1 (by_patch.py:63-67: `tv[:-1] += d; tv[1:] += d`, then the two ends times 2); all zeros for N == 1
__global__ __launch_bounds__(256) void eval_variation_finish_kernel(const float* __restrict__ partial, float* __restrict__ out, int F,
                                                                    int N, int wgs) {
  const int lane = threadIdx.x & 63;
  for (int f = threadIdx.x >> 6; f < F; f += 4) {
    const int n = f % N;
    const float* p = partial + (size_t)f * wgs * 2;
    const double tv = evalk::wave_sum_f64(p, wgs, 2, lane);
    double t = 0.0;
    if (n < N - 1) t += evalk::wave_sum_f64(p + 1, wgs, 2, lane);
    if (n > 0) t += evalk::wave_sum_f64(p + 1 - (size_t)wgs * 2, wgs, 2, lane);
    if (n == 0) t *= 2.0;
    if (n == N - 1) t *= 2.0;
    if (lane == 0) {
      out[f] = (float)tv;
      out[(size_t)F + f] = (float)t;
    }
  }
}
