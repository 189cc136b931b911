// Reconstruction of BasicVSR_origin, INFERENCE only (gfx950).  Reference ops replaced (models/basicvsr_arch_origin.py:84-93):
//   out = lrelu(fusion(cat[feat_b, feat_f]));  out = lrelu(pixel_shuffle(upconv1(out)));  out = lrelu(pixel_shuffle(upconv2(out)));
//   out = lrelu(conv_hr(out));  out = conv_last(out) + interpolate(x_i, scale_factor=4, 'bilinear', align_corners=False)
// Built on conv64.h: NHWC images with 64 channels per pixel, 16 x 16 tiles, 8 waves, wave w owns output half ch = w & 1 and (bf16)
// holds that half's packed weights in registers.  num_feat < 64 is embedded with zero rows / columns (packing.c64_recon_tables).
//
//   vr_fusion_kernel  1x1, 2F -> F, + LeakyReLU.  Reads the two trunks' NHWC state images directly (cw = 64 channels per pixel from
//                     the wide route, 24 from the conv3x3.h route; channels >= F are exact zeros there): the B fragment of k-step s
//                     is one 16-byte global load per lane, no LDS, no halo, no concat.
//   vr_upconv_kernel  3x3, 64 -> 256, + PixelShuffle(2) + LeakyReLU: four 64-output sub-convs q = 2 dy + dx over ONE staged input
//                     tile; sub-conv q's output channel c is the layer's channel 4 c + q and is stored to channel c of pixel
//                     (2 Y + dy, 2 X + dx) of the 2H x 2W image (LeakyReLU commutes with the shuffle).
//   conv_hr           c64_conv_kernel<T, 64, 2, false, false> of conv64.h.
//   vr_last_kernel    3x3, 64 -> 3, + bias + bilinear x4 base of the input frame -> NCHW fp32 in the caller's output.  Three real
//                     output rows: v_mfma_f32_16x16x32_bf16 (fp32: 8 x v_mfma_f32_16x16x4_f32), weights as the A operand (row co =
//                     lane & 15), 16 pixels of one tile row as B; accumulator regs 0..2 of lanes 0..15 are the three channels.
#pragma once
#include "conv64.h"

struct VRCfg {
  static constexpr int KS_FUS = 8;                                       // 128 kernel channels / 16
  static constexpr int FUS_ELEMS = 2 * KS_FUS * 512 + 64;
  static constexpr int SUB_ELEMS = C64Cfg::blob_elems(64);               // one sub-pixel conv of an upconv
  static constexpr int KS_LAST = 18;                                     // 9 taps x 2 chunks of 32 channels
  static constexpr int LAST_ELEMS = KS_LAST * 512 + 64;
};

// store 32 output channels (half ch) of one pixel: accumulator regs 4 g + j = channels 32 ch + 8 g + 4 hh + j
template <typename T, int ACT> SR_DEV void vr_store_half(T* yp, const f32x16& acc) {
  typedef typename FragOf<T>::half_type HalfT;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    HalfT v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (T)c3_act<ACT>(acc[4 * g + j]);
    *reinterpret_cast<HalfT*>(yp + 8 * g) = v;
  }
}

// ---------------------------------------------------------------------------------------------
// fusion: y[N][H][W][64] = lrelu(W [fb | ff] + b); fb, ff [N][H][W][cw].  grid = (tiles, N)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_fusion_kernel(const T* __restrict__ fb, const T* __restrict__ ff, int cw,
                                                                   T* __restrict__ y, const T* __restrict__ wconv, int H, int W,
                                                                   int tiles_x) {
  typedef C64Cfg C;
  typedef typename FragOf<T>::type FragT;
  constexpr int KS = VRCfg::KS_FUS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, ch = wave & 1;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  C64W<T, KS> w;
  w.load(wconv, ch, lane);
  const T* const bias = wconv + 2 * KS * 512;
#pragma unroll 1
  for (int pt = wave >> 1; pt < C::NPT_O; pt += C::NWAVES / 2) {
    const int pc = pt * 32 + r, oy = pc / C::TW, ox = pc - oy * C::TW;
    const int Y = ty0 + oy, X = tx0 + ox;
    const bool in = Y < H && X < W;
    const size_t pix = in ? ((size_t)n * H + Y) * W + X : 0;
    f32x16 acc = c64_bias<T>(bias, ch, hh);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const T* const src = s < KS / 2 ? fb : ff;
      const int q = 2 * (s & 3) + hh;                  // 8-channel chunk of the state row
      FragT b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = (T)0.f;
      if (in && q * 8 < cw) b = *reinterpret_cast<const FragT*>(src + pix * cw + q * 8);
      acc = mma16<T>(w.get(s, lane), b, acc);
    }
    if (in) vr_store_half<T, 2>(y + pix * C::CO + 32 * ch + 4 * hh, acc);
  }
}

// ---------------------------------------------------------------------------------------------
// upconv + PixelShuffle(2) + LeakyReLU: x [N][H][W][64] -> y [N][2H][2W][64].  grid = (tiles of the H x W image, N)
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_upconv_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                   const T* __restrict__ wblob, int H, int W, int tiles_x) {
  typedef C64Cfg C;
  constexpr int RS = C::rs<T>(64), KS = C::ks(64);
  __shared__ __attribute__((aligned(16))) T xs[C::NPXH * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, ch = wave & 1;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  C64W<T, KS> w;
  w.load(wblob, ch, lane);                             // sub-conv 0, in flight while the tile is staged
  c64_stage<T, 64, C::HW, C::NPXH>(xs, x + (size_t)n * H * W * C::CO, H, W, ty0 - 1, tx0 - 1, tid);
  __syncthreads();
  const int H2 = 2 * H, W2 = 2 * W;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const T* const wq = wblob + (size_t)q * VRCfg::SUB_ELEMS;
    if (q > 0) w.load(wq, ch, lane);
    const T* const bias = wq + 2 * KS * 512;
    const int dy = q >> 1, dx = q & 1;
#pragma unroll 1
    for (int pt = wave >> 1; pt < C::NPT_O; pt += C::NWAVES / 2) {
      const int pc = pt * 32 + r, oy = pc / C::TW, ox = pc - oy * C::TW;
      const f32x16 acc = c64_mma<T, 64, KS>(xs, (oy * C::HW + ox) * RS, C::HW, w, c64_bias<T>(bias, ch, hh), lane);
      const int Y = ty0 + oy, X = tx0 + ox;
      if (Y < H && X < W)
        vr_store_half<T, 2>(y + (((size_t)n * H2 + 2 * Y + dy) * W2 + 2 * X + dx) * C::CO + 32 * ch + 4 * hh, acc);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// conv_last + bias + bilinear x4 base
// ---------------------------------------------------------------------------------------------
// D = A B + C over one 32-deep k-step of a 16 x 16 tile: lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k][col l & 15];
// accumulator reg i = D[row 4 (l >> 4) + i][col l & 15].  fp32: MFMA #j contracts k in {j, 8 + j, 16 + j, 24 + j}.
template <typename T> SR_DEV f32x4 vr_mma32(typename FragOf<T>::type a, typename FragOf<T>::type b, f32x4 c);
template <> SR_DEV f32x4 vr_mma32<__bf16>(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <> SR_DEV f32x4 vr_mma32<float>(f32x8 a, f32x8 b, f32x4 c) {
#pragma unroll
  for (int j = 0; j < 8; ++j) c = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b[j], c, 0, 0, 0);
  return c;
}

// source taps of output index d of a x4 bilinear upsample with align_corners = False, as ATen computes them
// (area_pixel_compute_source_index: src = max(0.25 (d + 0.5) - 0.5, 0); i1 = min(i0 + 1, n - 1); l1 = src - i0, l0 = 1 - l1)
struct VRTap { int i0, i1; float l0, l1; };
SR_DEV VRTap vr_tap(int d, int n) {
  float src = 0.25f * ((float)d + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  VRTap t;
  t.i0 = (int)src;
  t.i1 = t.i0 + (t.i0 < n - 1 ? 1 : 0);
  t.l1 = src - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// base value at HR pixel (Y, X) of one LR plane [h][w]: fma(l0y, top, l1y bot) with top = fma(l0x, v00, l1x v01), bot =
// fma(l0x, v10, l1x v11) -- the second product of each pair rounded on its own, the first fused into the sum: the order in
// which ATen's vectorised CPU kernel evaluates it (pinned bit for bit by tests/test_vsr_recon_host.py)
SR_DEV float vr_base(const float* __restrict__ p, int w, const VRTap& ty, const VRTap& tx) {
#pragma clang fp contract(off)
  const float v00 = p[(size_t)ty.i0 * w + tx.i0], v01 = p[(size_t)ty.i0 * w + tx.i1];
  const float v10 = p[(size_t)ty.i1 * w + tx.i0], v11 = p[(size_t)ty.i1 * w + tx.i1];
  const float t1 = tx.l1 * v01, b1 = tx.l1 * v11;
  const float top = __builtin_fmaf(tx.l0, v00, t1);
  const float bot = __builtin_fmaf(tx.l0, v10, b1);
  const float yb = ty.l1 * bot;
  return __builtin_fmaf(ty.l0, top, yb);
}

// x [N][H][W][64] (H, W = the x4 size) -> out[n * out_bs + (c * H + Y) * W + X], c < 3; frame [n * frame_bs + (c * H/4 + y) * W/4 + x].
// grid = (tiles, N); wave w computes tile rows w and w + 8 (16 pixels per MFMA column set)
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void vr_last_kernel(const T* __restrict__ x, const T* __restrict__ wconv,
                                                                 const float* __restrict__ frame, long frame_bs,
                                                                 float* __restrict__ out, long out_bs, int H, int W, int tiles_x) {
  typedef C64Cfg C;
  constexpr int RS = C::rs<T>(64), KS = VRCfg::KS_LAST;
  __shared__ __attribute__((aligned(16))) T xs[C::NPXH * RS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, kq = lane >> 4;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  C64W<T, KS> w;
  w.load(wconv, 0, lane);
  c64_stage<T, 64, C::HW, C::NPXH>(xs, x + (size_t)n * H * W * C::CO, H, W, ty0 - 1, tx0 - 1, tid);
  __syncthreads();
  const T* const bias = wconv + KS * 512;
  const int h = H >> 2, wl = W >> 2;
  const float* const fr = frame + (size_t)n * frame_bs;
  float* const o = out + (size_t)n * out_bs;
#pragma unroll 1
  for (int oy = wave; oy < C::TH; oy += C::NWAVES) {
    const int win = (oy * C::HW + l16) * RS + kq * 8;
    f32x4 acc;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (kq == 0 && i < 3) ? (float)bias[i] : 0.f;
    if constexpr (C64W<T, KS>::REG) {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int tap = s >> 1, c = s & 1;
        acc = vr_mma32<T>(w.get(s, lane), lds_chunk<T>(xs, win + ((tap / 3) * C::HW + (tap % 3)) * RS + c * 32), acc);
      }
    } else {
#pragma unroll 1
      for (int tap = 0; tap < 9; ++tap) {
        const int row = win + ((tap / 3) * C::HW + (tap % 3)) * RS;
#pragma unroll
        for (int c = 0; c < 2; ++c) acc = vr_mma32<T>(w.get(2 * tap + c, lane), lds_chunk<T>(xs, row + c * 32), acc);
      }
    }
    const int Y = ty0 + oy, X = tx0 + l16;
    if (kq == 0 && Y < H && X < W) {
      const VRTap ty = vr_tap(Y, h), tx = vr_tap(X, wl);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        o[((size_t)c * H + Y) * W + X] = acc[c] + vr_base(fr + (size_t)c * h * wl, wl, ty, tx);
    }
  }
}
