// ssim of the evaluation loop on device (gfx950).  Reference op replaced: common/metrics.py:41-68, called by
// utils/estimate.py:126-129 on `model(lr).to('cpu')`, which hands two float64 luma images to skimage's
// structural_similarity(win_size=11, gaussian_weights=True, sigma=1.5, data_range=1, K1=0.01, K2=0.03):
//   sr -> round-half-even(sr * 255) clamped to [0, 255], / 255 (hr is not quantised); luma of both =
//   (R c0 + G c1) + B c2 with c = float32([65.738, 129.057, 25.064]) / 256, three rounded fp32 products added in fp32
//   (no fma: one fp32 ulp of luma is visible in the result); crop `shave`; everything below in double:
//   ux, uy, uxx, uyy, uxy = the 11-tap Gaussian (sigma 1.5, normalised) of X, Y, XX, YY, XY, applied separably;
//   vx = c (uxx - ux^2), vy = c (uyy - uy^2), vxy = c (uxy - ux uy), c = 121 / 120 (sample covariance);
//   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)); mean of S without its 5-pixel border.
// The border crop equals the filter radius, so no kept pixel's window leaves the shaved image: the filter's border mode
// never shows, and the kernel computes the "valid" region only, (H - 2 shave - 10) x (W - 2 shave - 10) pixels.
//
// One workgroup owns a TH x TW tile of output pixels of one image: the two fp32 lumas of the tile + 10 halo go to LDS
// (computed on load from the three planes), the horizontal pass writes five double maps to LDS, the vertical pass reads
// them, evaluates S and the workgroup writes ONE partial sum.  Nothing else goes to HBM; no atomics, fixed summation
// order: two calls give the same bits.
//   LDS banking (MI355X: 32 dword banks for ds_read_b32 and every ds_write, 64 for ds_read_b64, lanes conflict within
//   a 32-lane half, ds_write_b64 within 16 contiguous lanes): the horizontal pass puts ROWS on lanes, so its fp32 reads
//   are LS = 43 dwords apart (odd: conflict-free) and its double stores HS = 33 doubles = 66 dwords apart (2 mod 32:
//   16 lanes cover 32 banks once); the vertical pass puts COLUMNS on lanes: 32 lanes read 256 contiguous bytes.
#pragma once
#include "sr_common.h"

namespace ssim {
constexpr int TW = 32, TH = 32, R = 5, TAPS = 2 * R + 1;          // output tile, filter radius
constexpr int IW = TW + 2 * R, IH = TH + 2 * R;                   // luma tile with halo
constexpr int LS = IW + 1;                                        // luma row stride in floats (odd)
constexpr int HS = TW + 1;                                        // row stride of the horizontal-pass maps in doubles
constexpr int CW = 2;                                             // adjacent columns per thread in the horizontal pass
constexpr int RH = 4;                                             // adjacent rows per thread in the vertical pass
constexpr int THREADS = 256;
static_assert(TW % CW == 0 && TH % RH == 0 && TW * (TH / RH) == THREADS, "vertical pass: one item per thread");
static_assert((LS & 1) == 1 && (2 * HS) % 32 == 2, "LDS strides chosen against bank conflicts (see above)");
struct Weights { double w[TAPS]; };

// (r c0 + g c1) + b c2 as three rounded fp32 products and two rounded fp32 sums.  hipcc defines __fmul_rn / __fadd_rn as plain
// `*` / `+`, which it contracts into v_fma_f32 / v_pk_fma_f32 under its default -ffp-contract=fast: the pragma is what holds.
SR_DEV float luma(float r, float g, float b) {
#pragma clang fp contract(off)
  const float c0 = 65.738f / 256.f, c1 = 129.057f / 256.f, c2 = 25.064f / 256.f;
  const float p0 = r * c0, p1 = g * c1, p2 = b * c2;
  const float s01 = p0 + p1;
  return s01 + p2;
}
// the reference's 8-bit quantisation of sr: (v * 255).round().clamp(0, 255) / 255 in fp32 (round half to even, true division)
SR_DEV float quant8(float v) {
#pragma clang fp contract(off)
  return fminf(fmaxf(rintf(v * 255.f), 0.f), 255.f) / 255.f;
}
}  // namespace ssim

// grid (tiles_x * tiles_y, N); partial[n * gridDim.x + tile] = sum of S over the tile's pixels inside the image
__global__ __launch_bounds__(ssim::THREADS) void sr_ssim_tile_kernel(const float* __restrict__ sr, const float* __restrict__ hr,
                                                                     double* __restrict__ partial, int H, int W, int shave,
                                                                     int tiles_x, ssim::Weights wt) {
  using namespace ssim;
  __shared__ float lx[IH * LS], ly[IH * LS];
  __shared__ double hm[5][IH * HS];
  __shared__ double red[THREADS / 64];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int ty0 = (int)(blockIdx.x / tiles_x) * TH, tx0 = (int)(blockIdx.x % tiles_x) * TW;   // in output coordinates
  const int hc = H - 2 * shave, wc = W - 2 * shave;                                           // the shaved image
  const size_t plane = (size_t)H * W;
  const float* s = sr + (size_t)n * 3 * plane;
  const float* h = hr + (size_t)n * 3 * plane;

  // lumas of the tile + halo; pixels past the shaved image read as 0 (their outputs are not summed)
  for (int i = tid; i < IH * IW; i += THREADS) {
    const int r = i / IW, c = i - r * IW;
    float x = 0.f, y = 0.f;
    if (ty0 + r < hc && tx0 + c < wc) {
      const size_t o = (size_t)(ty0 + r + shave) * W + (tx0 + c + shave);
      x = luma(quant8(s[o]), quant8(s[o + plane]), quant8(s[o + 2 * plane]));
      y = luma(h[o], h[o + plane], h[o + 2 * plane]);
    }
    lx[r * LS + c] = x;
    ly[r * LS + c] = y;
  }
  __syncthreads();

  // horizontal pass: item = (column pair, row), rows on lanes
  for (int i = tid; i < IH * (TW / CW); i += THREADS) {
    const int cg = i / IH, r = i - cg * IH, c = cg * CW;
    double a[5][CW];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int j = 0; j < CW; ++j) a[m][j] = 0.0;
#pragma unroll
    for (int k = 0; k < TAPS + CW - 1; ++k) {
      const double x = (double)lx[r * LS + c + k], y = (double)ly[r * LS + c + k];
      const double xx = x * x, yy = y * y, xy = x * y;
#pragma unroll
      for (int j = 0; j < CW; ++j) {
        if (k - j < 0 || k - j >= TAPS) continue;
        const double w = wt.w[k - j];
        a[0][j] += w * x;
        a[1][j] += w * y;
        a[2][j] += w * xx;
        a[3][j] += w * yy;
        a[4][j] += w * xy;
      }
    }
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int j = 0; j < CW; ++j) hm[m][r * HS + c + j] = a[m][j];
  }
  __syncthreads();

  // vertical pass and S: item = (row group, column), columns on lanes
  double sum = 0.0;
  {
    const int c = tid % TW, r0 = (tid / TW) * RH;
    double a[5][RH];
#pragma unroll
    for (int m = 0; m < 5; ++m)
#pragma unroll
      for (int j = 0; j < RH; ++j) a[m][j] = 0.0;
#pragma unroll
    for (int k = 0; k < TAPS + RH - 1; ++k) {
      double v[5];
#pragma unroll
      for (int m = 0; m < 5; ++m) v[m] = hm[m][(r0 + k) * HS + c];
#pragma unroll
      for (int j = 0; j < RH; ++j) {
        if (k - j < 0 || k - j >= TAPS) continue;
        const double w = wt.w[k - j];
#pragma unroll
        for (int m = 0; m < 5; ++m) a[m][j] += w * v[m];
      }
    }
    const double C1 = 0.01 * 0.01, C2 = 0.03 * 0.03, cov = 121.0 / 120.0;
#pragma unroll
    for (int j = 0; j < RH; ++j) {
      const double ux = a[0][j], uy = a[1][j];
      const double vx = cov * (a[2][j] - ux * ux), vy = cov * (a[3][j] - uy * uy), vxy = cov * (a[4][j] - ux * uy);
      const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
      if (ty0 + r0 + j < hc - 2 * R && tx0 + c < wc - 2 * R) sum += S;
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// one wave per image (images w, w + 4, ...): mean of S = sum of the image's partials / count; out[0] = sum over images
__global__ __launch_bounds__(256) void sr_ssim_finish_kernel(const double* __restrict__ partial, double* __restrict__ out, int N,
                                                             int tiles, double count) {
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total = 0.0;
  for (int n = wave; n < N; n += 4) {
    double sum = 0.0;
    for (int t = lane; t < tiles; t += 64) sum += partial[(size_t)n * tiles + t];
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    total += sum / count;
  }
  if (lane == 0) red[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (red[0] + red[1]) + (red[2] + red[3]);
}
