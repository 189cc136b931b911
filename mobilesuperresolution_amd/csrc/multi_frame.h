// Multi-frame video network (models/naive_multi_model_easy.py Naive_model, the trainers' 'multi' model), inference on 32-wide NHWC
// activations (gfx950).  Reference ops replaced, per frame i of a clip (flows given):
//   e_i = encode(x_i);  y = body0(cat(flow, flow_warp(e_{i-1}, flow), e_i)) + e_i  (frame 0 of a clip: flow = 0, warp = e_0);
//   y = body_j(y) + y;  out_i = PixelShuffle(4)(decode(y)) + interpolate(x_i, scale_factor=4, 'bilinear', align_corners=False)
// Activations follow frame_net.h: [frame][H][W][32] in the hot dtype, channels >= C exactly zero; the encoder is sr_head_fwd with
// mean 0 and blocks 1.. are fn_block_kernel<T, false>.  New here:
//   mf_first_kernel<T>  block 0 in one launch, one workgroup = one 8 x 32 tile of one frame.  conv1's K dimension is three groups
//                       that pass through ONE staged 12 x 36 tile in turn while conv1's accumulators (the wave's <= 3 pixel tiles of
//                       the 10 x 34 region) stay in registers:  e_i (rm_stage)  ->  warp: e_{i-1} gathered at pixel + flow with
//                       flow_warp.h's warp_pos / warp_taps, the four taps blended in fp32 in flow_warp_fwd_kernel's order, rounded
//                       once to T  ->  flow: the two flow channels rounded to T, 8 elements per pixel in a small tile of its own.
//                       Every staged operand at a pixel OUTSIDE the image is zero, warp and flow included (the conv pads the
//                       concatenated tensor; it does not warp out-of-image positions); taps outside the image contribute zero.
//                       Frame 0 of each clip (frame n = b NF + i, i == 0) runs the warp group on the staged e_i itself and skips the
//                       flow group; it never reads frame n - 1.  t = ReLU(conv1 + b1) then overwrites the staged tile (zero outside
//                       the image) and y = conv2(t) + b2 + e_i, e_i read back from global memory.
//   mf_tail_kernel<T>   decode 3 x 3, C -> 48 (two 32-row tiles, one after the other with its 18 fragments in registers) on the
//                       feature tile + 1-pixel halo; accumulator regs 4g..4g+3 are four neighbouring HR pixels of one row, so
//                       PixelShuffle(4) is the store address; + the x4 bilinear base (vr_tap / vr_base of vsr_recon.h) of the fp32
//                       input frame, staged as a 3 x 10 x 34 tile.  NCHW fp32, every element written once.
// Packed blob (packing.mf_tables), elements of T: block 0 = [e group 18 fragments][warp group 18][flow group 5: lane l, element j of
// fragment s = W1[row l & 31][flow channel j < 2][tap 2 s + (l >> 5) < 9]][32 biases], conv2 as an fn conv; blocks 1.. as fn convs;
// decode = 2 x 18 fragments + 64 biases.  No atomics.
#pragma once
#include "frame_net.h"
#include "flow_warp.h"
#include "vsr_recon.h"

struct MfCfg {
  static constexpr int FS = 8, KF = 5;                                  // flow tile: elements per pixel, k-steps
  static constexpr int C1_ELEMS = (2 * FnCfg::KS + KF) * 512 + 32;      // block 0 conv1
  static constexpr int FIRST_ELEMS = C1_ELEMS + FnCfg::CONV_ELEMS;
  static constexpr int DEC_ELEMS = 2 * FnCfg::KS * 512 + 64;
  static constexpr int NK = (FnCfg::NTT + FnCfg::NW - 1) / FnCfg::NW;   // conv1 pixel tiles per wave
};

// e: the frame stack's base pointer (s0); flows: fp32 (B, NF - 1, 2, H, W), channel 0 = dx; y: the output stack; wp: block 0
// TRAIN: the tile's 8 x 32 core of t goes to tsave, bit c of mask[pixel] = (conv1's fp32 accumulator of channel c > 0), the warp
// operand as staged (rounded once to T; frame 0 of a clip: a copy of e_0) to wsave and the rounded flow to channels 0, 1 of fsave
// (channels 2.., and all of frame 0 of a clip, zero); y is computed by the same instructions either way.
template <typename T, bool TRAIN>
SR_DEV void mf_first_body(const T* __restrict__ e, const float* __restrict__ flows, T* __restrict__ y, const T* __restrict__ wp,
                          T* __restrict__ tsave, uint32_t* __restrict__ mask, T* __restrict__ wsave, T* __restrict__ fsave, int H, int W,
                          int tiles_x, int NF) {
  typedef FnCfg C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int SW = C::XW, NPS = C::NPX, X_ELEMS = NPS * C::CS;
  static_assert(C::NTT * 32 * C::CS <= X_ELEMS, "t overwrites the staged tile");
  __shared__ __attribute__((aligned(16))) unsigned char mf_smem[(X_ELEMS + NPS * MfCfg::FS) * sizeof(T)];
  T* const xs = reinterpret_cast<T*>(mf_smem);
  T* const fs = xs + X_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ty0 = ty * C::TH, tx0 = tx * C::TW;
  const int clip = n / NF, fi = n - clip * NF;
  const bool has_prev = fi > 0;                                         // block-uniform
  const size_t plane = (size_t)H * W, img = (size_t)n * plane;
  rm_stage<T, C::C, C::CS, SW, NPS, false, 256>(xs, e + img * C::C, nullptr, H, W, ty0 - 2, tx0 - 2, tid);
  __syncthreads();

  // this lane's conv1 pixels: tile q = wave + 4 k of the 10 x 34 region
  int base[MfCfg::NK];
#pragma unroll
  for (int k = 0; k < MfCfg::NK; ++k) {
    const int p = 32 * (wave + C::NW * k) + r, pc = p < C::NPT ? p : C::NPT - 1;     // lanes past the region: a copy of its last pixel
    const int py = pc / C::TTW, px = pc - py * C::TTW;
    base[k] = py * SW + px;
  }
  FragT a[C::KS];
  f32x16 acc[MfCfg::NK];
  {
    const f32x16 c1 = fn_bias_init<T>(wp + (2 * C::KS + MfCfg::KF) * 512, hh);
#pragma unroll
    for (int k = 0; k < MfCfg::NK; ++k) acc[k] = c1;
  }
  // group e
#pragma unroll
  for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(wp, s, lane);
#pragma unroll
  for (int k = 0; k < MfCfg::NK; ++k)
    if (wave + C::NW * k < C::NTT) acc[k] = fn_conv_tile<T>(a, xs, base[k] * C::CS, SW, hh, acc[k]);

  if (has_prev) {
    __syncthreads();                                                    // every wave is done with e_i in xs
    const T* const ep = e + (img - plane) * C::C;                       // e_{i-1}: the same clip's previous frame
    const float* const fl = flows + ((size_t)clip * (NF - 1) + (fi - 1)) * 2 * plane;
    for (int idx = tid; idx < NPS * 4; idx += 256) {
      const int p = idx >> 2, c = idx & 3;
      const int py = p / SW, px = p - py * SW;
      const int Y = ty0 - 2 + py, X = tx0 - 2 + px;
      FragT v, f8;
#pragma unroll
      for (int j = 0; j < 8; ++j) { v[j] = (T)0.f; f8[j] = (T)0.f; }
      if (Y >= 0 && Y < H && X >= 0 && X < W) {
        const size_t pix = (size_t)Y * W + X;
        const float fx = fl[pix], fy = fl[plane + pix];
        f8[0] = (T)fx; f8[1] = (T)fy;
        const WarpTaps t = warp_taps(warp_pos((float)X + fx, W), warp_pos((float)Y + fy, H), H, W);
        const float w00 = (1.f - t.wx) * (1.f - t.wy), w01 = t.wx * (1.f - t.wy), w10 = (1.f - t.wx) * t.wy, w11 = t.wx * t.wy;
        const long o00 = ((long)t.y0 * W + t.x0) * C::C + c * 8;        // used only where the tap is inside the image
        float b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) b[j] = 0.f;
        if (t.vy0 && t.vx0) {
          const FragT g = *reinterpret_cast<const FragT*>(ep + o00);
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] += w00 * (float)g[j];
        }
        if (t.vy0 && t.vx1) {
          const FragT g = *reinterpret_cast<const FragT*>(ep + o00 + C::C);
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] += w01 * (float)g[j];
        }
        if (t.vy1 && t.vx0) {
          const FragT g = *reinterpret_cast<const FragT*>(ep + o00 + (long)W * C::C);
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] += w10 * (float)g[j];
        }
        if (t.vy1 && t.vx1) {
          const FragT g = *reinterpret_cast<const FragT*>(ep + o00 + (long)(W + 1) * C::C);
#pragma unroll
          for (int j = 0; j < 8; ++j) b[j] += w11 * (float)g[j];
        }
#pragma unroll
        for (int j = 0; j < 8; j += 2) {
          T lo, hi;
          cvt_pair<T>(lo, hi, b[j], b[j + 1]);
          v[j] = lo; v[j + 1] = hi;
        }
      }
      *reinterpret_cast<FragT*>(xs + p * C::CS + c * 8) = v;
      if (c == 0) *reinterpret_cast<FragT*>(fs + p * MfCfg::FS) = f8;
      if constexpr (TRAIN) {
        if (py >= 2 && py < 2 + C::TH && px >= 2 && px < 2 + C::TW && Y < H && X < W) {     // core pixels are at Y, X >= 0
          const size_t o = (img + (size_t)Y * W + X) * C::C + c * 8;
          *reinterpret_cast<FragT*>(wsave + o) = v;
          if (c != 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f8[j] = (T)0.f;
          }
          *reinterpret_cast<FragT*>(fsave + o) = f8;
        }
      }
    }
    __syncthreads();
  } else if constexpr (TRAIN) {                                          // frame 0 of a clip: warp = the staged e_0, flow = 0
    for (int idx = tid; idx < C::TH * C::TW * 4; idx += 256) {
      const int p = idx >> 2, c = idx & 3;
      const int py = p / C::TW, px = p - py * C::TW;
      const int Y = ty0 + py, X = tx0 + px;
      if (Y < H && X < W) {
        const size_t o = (img + (size_t)Y * W + X) * C::C + c * 8;
        FragT z;
#pragma unroll
        for (int j = 0; j < 8; ++j) z[j] = (T)0.f;
        *reinterpret_cast<FragT*>(wsave + o) = *reinterpret_cast<const FragT*>(xs + ((py + 2) * SW + px + 2) * C::CS + c * 8);
        *reinterpret_cast<FragT*>(fsave + o) = z;
      }
    }
  }
  // group warp (frame 0 of a clip: the staged e_i itself)
#pragma unroll
  for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(wp, C::KS + s, lane);
#pragma unroll
  for (int k = 0; k < MfCfg::NK; ++k)
    if (wave + C::NW * k < C::NTT) acc[k] = fn_conv_tile<T>(a, xs, base[k] * C::CS, SW, hh, acc[k]);
  // group flow (frame 0 of a clip: flow = 0, nothing to add)
  if (has_prev) {
#pragma unroll
    for (int s = 0; s < MfCfg::KF; ++s) a[s] = load_wfrag<T>(wp, 2 * C::KS + s, lane);
#pragma unroll
    for (int k = 0; k < MfCfg::NK; ++k) {
      if (wave + C::NW * k < C::NTT) {
#pragma unroll
        for (int s = 0; s < MfCfg::KF; ++s) {
          const int tap = 2 * s + hh, tc = tap < 9 ? tap : 8, dy = tc / 3, dx = tc - 3 * dy;
          FragT b = lds_chunk<T>(fs, (base[k] + dy * SW + dx) * MfCfg::FS);
          if (tap >= 9) {
#pragma unroll
            for (int j = 0; j < 8; ++j) b[j] = (T)0.f;
          }
          acc[k] = mma16<T>(a[s], b, acc[k]);
        }
      }
    }
  }
  __syncthreads();                                                      // every wave is done with xs: t takes its place
  T* const ts = xs;
#pragma unroll
  for (int k = 0; k < MfCfg::NK; ++k) {
    const int q = wave + C::NW * k;
    if (q < C::NTT) {
      const int p = 32 * q + r, pc = p < C::NPT ? p : C::NPT - 1;
      const int py = pc / C::TTW, px = pc - py * C::TTW;
      const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
      const bool in = Y >= 0 && Y < H && X >= 0 && X < W;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        HalfT v;
        T e0, e1, e2, e3;
        cvt_pair<T>(e0, e1, fmaxf(acc[k][4 * g], 0.f), fmaxf(acc[k][4 * g + 1], 0.f));
        cvt_pair<T>(e2, e3, fmaxf(acc[k][4 * g + 2], 0.f), fmaxf(acc[k][4 * g + 3], 0.f));
        v[0] = in ? e0 : (T)0.f; v[1] = in ? e1 : (T)0.f; v[2] = in ? e2 : (T)0.f; v[3] = in ? e3 : (T)0.f;
        *reinterpret_cast<HalfT*>(ts + p * C::CS + 8 * g + 4 * hh) = v;     // p < NTT * 32: inside the t image
        if constexpr (TRAIN) {
          if (in && p < C::NPT && py >= 1 && py <= C::TH && px >= 1 && px <= C::TW)
            *reinterpret_cast<HalfT*>(tsave + (img + (size_t)Y * W + X) * C::C + 8 * g + 4 * hh) = v;
        }
      }
      if constexpr (TRAIN) {
        uint32_t mbits = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) mbits |= (acc[k][i] > 0.f ? 1u : 0u) << ((i & 3) + 8 * (i >> 2) + 4 * hh);
        mbits |= __shfl_xor(mbits, 32);
        if (hh == 0 && in && p < C::NPT && py >= 1 && py <= C::TH && px >= 1 && px <= C::TW) mask[img + (size_t)Y * W + X] = mbits;
      }
    }
  }
  __syncthreads();
  const T* const w2 = wp + MfCfg::C1_ELEMS;
#pragma unroll
  for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(w2, s, lane);
  const f32x16 c2 = fn_bias_init<T>(w2 + C::KS * 512, hh);
  const int X = tx0 + r;
#pragma unroll 1
  for (int q = wave; q < C::TH; q += C::NW) {
    const f32x16 o = fn_conv_tile<T>(a, ts, (q * C::TTW + r) * C::CS, C::TTW, hh, c2);
    const int Y = ty0 + q;
    if (Y < H && X < W) {
      const size_t pix = img + (size_t)Y * W + X;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 8 * g + 4 * hh;
        const HalfT x4 = *reinterpret_cast<const HalfT*>(e + pix * C::C + c0);
        HalfT o4;
        T e0, e1, e2, e3;
        cvt_pair<T>(e0, e1, o[4 * g] + (float)x4[0], o[4 * g + 1] + (float)x4[1]);
        cvt_pair<T>(e2, e3, o[4 * g + 2] + (float)x4[2], o[4 * g + 3] + (float)x4[3]);
        o4[0] = e0; o4[1] = e1; o4[2] = e2; o4[3] = e3;
        *reinterpret_cast<HalfT*>(y + pix * C::C + c0) = o4;
      }
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(256) mf_first_kernel(const T* __restrict__ e, const float* __restrict__ flows, T* __restrict__ y,
                                                       const T* __restrict__ wp, int H, int W, int tiles_x, int NF) {
  mf_first_body<T, false>(e, flows, y, wp, nullptr, nullptr, nullptr, nullptr, H, W, tiles_x, NF);
}

// the training forward of block 0: mf_first_kernel that also leaves t, the ReLU bit mask, the warp operand and the flow image behind
template <typename T>
__global__ void __launch_bounds__(256) mf_first_train_kernel(const T* __restrict__ e, const float* __restrict__ flows, T* __restrict__ y,
                                                             const T* __restrict__ wp, T* __restrict__ tsave, uint32_t* __restrict__ mask,
                                                             T* __restrict__ wsave, T* __restrict__ fsave, int H, int W, int tiles_x,
                                                             int NF) {
  mf_first_body<T, true>(e, flows, y, wp, tsave, mask, wsave, fsave, H, W, tiles_x, NF);
}

// f: [frame][H][W][32]; frames: fp32 (frames, 3, H, W); out: fp32 (frames, 3, 4H, 4W); wp: the decode conv
template <typename T>
__global__ void __launch_bounds__(256) mf_tail_kernel(const T* __restrict__ f, const float* __restrict__ frames, float* __restrict__ out,
                                                      const T* __restrict__ wp, int H, int W, int tiles_x) {
  typedef FnCfg C;
  typedef typename FragOf<T>::type FragT;
  constexpr int X_ELEMS = C::NPL * C::CS;
  __shared__ __attribute__((aligned(16))) unsigned char mf_smem[X_ELEMS * sizeof(T) + 3 * C::NPL * 4];
  T* const xs = reinterpret_cast<T*>(mf_smem);
  float* const bs = reinterpret_cast<float*>(mf_smem + X_ELEMS * sizeof(T));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ty0 = ty * C::TH, tx0 = tx * C::TW;
  const size_t plane = (size_t)H * W;
  rm_stage<T, C::C, C::CS, C::LW, C::NPL, false, 256>(xs, f + (size_t)n * plane * C::C, nullptr, H, W, ty0 - 1, tx0 - 1, tid);
  const float* const fr = frames + (size_t)n * 3 * plane;
  for (int idx = tid; idx < 3 * C::NPL; idx += 256) {
    const int c = idx / C::NPL, p = idx - c * C::NPL;
    const int py = p / C::LW, px = p - py * C::LW;
    const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
    bs[idx] = (Y >= 0 && Y < H && X >= 0 && X < W) ? fr[(size_t)c * plane + (size_t)Y * W + X] : 0.f;
  }
  __syncthreads();
  const int H4 = 4 * H, W4 = 4 * W;
  float* const o_ = out + (size_t)n * 3 * H4 * W4;
  const int X = tx0 + r;
  VRTap txs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    txs[j] = vr_tap(4 * X + j, W);                                        // taps of the frame, moved into the staged tile
    txs[j].i0 -= tx0 - 1; txs[j].i1 -= tx0 - 1;
  }
#pragma unroll 1
  for (int rt = 0; rt < 2; ++rt) {
    FragT a[C::KS];
#pragma unroll
    for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(wp, rt * C::KS + s, lane);
    const f32x16 c0 = fn_bias_init<T>(wp + 2 * C::KS * 512 + 32 * rt, hh);
#pragma unroll 1
    for (int q = wave; q < C::TH; q += C::NW) {
      const f32x16 acc = fn_conv_tile<T>(a, xs, (q * C::LW + r) * C::CS, C::LW, hh, c0);
      const int Y = ty0 + q;
      if (Y < H && X < W) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int ch = 32 * rt + 8 * g + 4 * hh;                        // channels ch..ch+3 = HR pixels (4Y + si, 4X..4X+3) of plane c
          if (ch < 48) {
            const int c = ch >> 4, si = (ch >> 2) & 3;
            VRTap tyv = vr_tap(4 * Y + si, H);
            tyv.i0 -= ty0 - 1; tyv.i1 -= ty0 - 1;
            const float* const bp = bs + c * C::NPL;
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = acc[4 * g + j] + vr_base(bp, C::LW, tyv, txs[j]);
            *reinterpret_cast<f32x4*>(o_ + ((size_t)c * H4 + 4 * Y + si) * W4 + 4 * X) = v;
          }
        }
      }
    }
  }
}
