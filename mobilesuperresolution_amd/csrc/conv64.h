// 64-feature BasicVSR propagation trunk: the forward kernels (gfx950).  Reference ops replaced: ConvResidualBlocks /
// ResidualBlockNoBN at the reference's default num_feat = 64 (models/basicvsr_arch.py:108-147, basicvsr_arch_origin.py:98-152):
// conv3x3(F + 3 -> F) + LeakyReLU(0.1), then num_block x [x + conv2(relu(conv1(x)))], 24 < F <= 64 embedded in 64 channels with
// zero rows / columns (they stay exactly zero through every activation and residual add).  The inference route (sr_c64_trunk_fwd)
// writes nothing a backward would need; the opt-in training route (sr_c64_trunk_train_fwd, csrc/conv64_bwd.h) runs the per-conv
// kernel twice per block and keeps a_i and t_i.
//
// Layout: activations NHWC with 64 channels per pixel.  The first conv's input has CI = 80 channels as the kernels see it:
// warped state 0..63 | frame 64..66 | zeros (the state's chunks stay 16-byte aligned); CI = 64 for a trunk built as (F, F, n).
// Packed weights per conv (packing.c64_tables): 2 x KS fragments, fragment (half ch, k-step s) = A[row co = 32 ch + r][k = 16 c + 8 hh
// + j] of tap s / (CI / 16), chunk c = s % (CI / 16), then the 64 biases (C-init of the accumulator).
//
// Work split: 8 waves per 16 x 16 output tile, wave w owns output-channel half ch = w & 1 and HOLDS that half's
// weights in registers for the whole conv (bf16: KS x 4 VGPRs, 144 at CI = 64), so an MFMA reads only its 32-pixel activation fragment
// from LDS (1 KiB per wave, one ds_read_b128 per lane).  LDS rows are padded by 16 bytes (odd multiples of 16 B: conflict-free
// ds_read_b128 over consecutive pixels).  fp32 (parity mode): the same k order with fragments read from global memory per k-step.
#pragma once
#include "conv3x3.h"

struct C64Cfg {
  static constexpr int CO = 64, TH = 16, TW = 16, HW = TW + 2, HH = TH + 2, NPXH = HW * HH;   // 18 x 18 = 324 (1-pixel halo)
  static constexpr int NWAVES = 8, NTHREADS = 64 * NWAVES, NPT_O = TH * TW / 32;             // 8 pixel tiles of 32 in the core
  static constexpr int W2 = TW + 4, NP2 = W2 * (TH + 4);                                     // 20 x 20 = 400 (2-pixel halo)
  static constexpr int NPT_H = (NPXH + 31) / 32;                                             // 11 pixel tiles over 18 x 18
  template <typename T> static constexpr int rs(int ci) { return ci + 16 / (int)sizeof(T); }   // LDS row stride (elements)
  static constexpr int ks(int ci) { return 9 * ci / 16; }                                      // k-steps per conv
  static constexpr int blob_elems(int ci) { return 2 * ks(ci) * 512 + CO; }                    // one conv's packed size
};

// the first conv's input gathered on the fly: frame [N][3][H][W] fp32, state [N][H][W][64] (nullptr: zero state), flow [N][2][H][W]
template <typename T> struct C64WarpSrc {
  const float* frame;
  const T* state;
  const float* flow;
  long frame_bs, flow_bs;
  T* x0_save;              // SAVE kernels: the gathered 80-channel input [N][H][W][80], kept for the first conv's weight gradient
};

// the bilinear sample of 8 state channels (chunk) at taps t: flow_warp_fwd_kernel's blend, term by term
template <typename T> SR_DEV typename FragOf<T>::type c64_warp_chunk(const T* __restrict__ st, int W, const WarpTaps& t, int chunk) {
  typedef typename FragOf<T>::type FragT;
  const float w00 = (1.f - t.wx) * (1.f - t.wy), w01 = t.wx * (1.f - t.wy), w10 = (1.f - t.wx) * t.wy, w11 = t.wx * t.wy;
  const T* p00 = st + ((size_t)t.y0 * W + t.x0) * C64Cfg::CO + chunk * 8;
  FragT a, b, c, d, o;
#pragma unroll
  for (int j = 0; j < 8; ++j) { a[j] = (T)0.f; b[j] = (T)0.f; c[j] = (T)0.f; d[j] = (T)0.f; }
  if (t.vy0 && t.vx0) a = *reinterpret_cast<const FragT*>(p00);
  if (t.vy0 && t.vx1) b = *reinterpret_cast<const FragT*>(p00 + C64Cfg::CO);
  if (t.vy1 && t.vx0) c = *reinterpret_cast<const FragT*>(p00 + (size_t)W * C64Cfg::CO);
  if (t.vy1 && t.vx1) d = *reinterpret_cast<const FragT*>(p00 + (size_t)(W + 1) * C64Cfg::CO);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float v = 0.f;
    if (t.vy0 && t.vx0) v += w00 * (float)a[j];
    if (t.vy0 && t.vx1) v += w01 * (float)b[j];
    if (t.vy1 && t.vx0) v += w10 * (float)c[j];
    if (t.vy1 && t.vx1) v += w11 * (float)d[j];
    o[j] = (T)v;
  }
  return o;
}

// a region of an NHWC image with CI channels -> LDS rows of stride rs(CI), zero outside the image (padding = 1 of the conv)
template <typename T, int CI, int RW, int NPX>
SR_DEV void c64_stage(T* dst, const T* __restrict__ img, int H, int W, int y0, int x0, int tid) {
  typedef typename FragOf<T>::type FragT;
  constexpr int CC = CI / 8, RS = C64Cfg::rs<T>(CI);
  for (int idx = tid; idx < NPX * CC; idx += C64Cfg::NTHREADS) {
    const int p = idx / CC, c = idx - p * CC, py = p / RW, px = p - py * RW;
    const int Y = y0 + py, X = x0 + px;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) v = *reinterpret_cast<const FragT*>(img + ((size_t)Y * W + X) * CI + c * 8);
    *reinterpret_cast<FragT*>(dst + p * RS + c * 8) = v;
  }
}

// backward-data staging (c3_stage_dz at 64 channels): dz = g * act'(A) on the tile + 1-pixel halo, A the SAVED post-activation
// image (ReLU: t_i, LeakyReLU: a_0), zero outside the image
template <typename T, int ACT>
SR_DEV void c64_stage_dz(T* dst, const T* __restrict__ g, const T* __restrict__ a, int H, int W, int y0, int x0, int tid) {
  typedef typename FragOf<T>::type FragT;
  typedef C64Cfg C;
  constexpr int CC = 8, RS = C::rs<T>(64);
  for (int idx = tid; idx < C::NPXH * CC; idx += C::NTHREADS) {
    const int p = idx / CC, c = idx - p * CC, py = p / C::HW, px = p - py * C::HW;
    const int Y = y0 + py, X = x0 + px;
    FragT z;
#pragma unroll
    for (int j = 0; j < 8; ++j) z[j] = (T)0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
      const size_t o = ((size_t)Y * W + X) * C::CO + c * 8;
      const FragT gv = *reinterpret_cast<const FragT*>(g + o), av = *reinterpret_cast<const FragT*>(a + o);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = (T)((float)gv[j] * c3_dact<ACT>((float)av[j]));
    }
    *reinterpret_cast<FragT*>(dst + p * RS + c * 8) = z;
  }
}

// the gathered 80-channel input of the first conv on the tile + 1-pixel halo: chunks 0..7 = flow_warp(state), chunk 8 = frame | 0
template <typename T>
SR_DEV void c64_stage_warp(T* dst, const C64WarpSrc<T>& s, int n, int H, int W, int ty0, int tx0, int tid) {
  typedef typename FragOf<T>::type FragT;
  typedef C64Cfg C;
  constexpr int CC = 10, RS = C::rs<T>(80);
  const T* st = s.state ? s.state + (size_t)n * H * W * C::CO : nullptr;
  for (int idx = tid; idx < C::NPXH * CC; idx += C::NTHREADS) {
    const int p = idx / CC, c = idx - p * CC, py = p / C::HW, px = p - py * C::HW;
    const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (Y >= 0 && Y < H && X >= 0 && X < W) {
      if (c < 8) {
        if (st) v = c64_warp_chunk<T>(st, W, c3_taps_of(s.flow, s.flow_bs, n, Y, X, H, W), c);
      } else if (c == 8) {
        const float* fr = s.frame + (size_t)n * s.frame_bs + (size_t)Y * W + X;
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = (T)fr[(size_t)j * H * W];
      }
    }
    *reinterpret_cast<FragT*>(dst + p * RS + c * 8) = v;
  }
}

// this wave's half of the packed weights: bf16 in registers for the whole conv (KS x 4 VGPRs); fp32 re-read per k-step from
// global memory (L1 / L2 hits; 2 x the registers would not fit)
template <typename T, int KS> struct C64W {
  static constexpr bool REG = sizeof(T) == 2;
  typename FragOf<T>::type r[REG ? KS : 1];
  const T* p;
  SR_DEV void load(const T* wconv, int ch, int lane) {
    if constexpr (REG) {
#pragma unroll
      for (int s = 0; s < KS; ++s) r[s] = load_wfrag<T>(wconv, ch * KS + s, lane);
    } else {
      p = weights_for_tile<false>(wconv) + (size_t)ch * KS * 512;
    }
  }
  SR_DEV typename FragOf<T>::type get(int s, int lane) const {
    if constexpr (REG) return r[s];
    else return load_wfrag<T>(p, s, lane);
  }
};

// accumulator C-init: the bias of output channels 32 ch + 8 g + 4 hh + j (acc reg 4 g + j)
template <typename T> SR_DEV f32x16 c64_bias(const T* __restrict__ bias, int ch, int hh) {
  typedef typename FragOf<T>::half_type HalfT;
  f32x16 acc;
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const HalfT b = *reinterpret_cast<const HalfT*>(bias + 32 * ch + 8 * g + 4 * hh);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[4 * g + j] = (float)b[j];
  }
  return acc;
}

// one 32-pixel tile x 32 output channels: `win` = element offset of the lane's 3 x 3 window's top-left pixel row, `rw` = region width
template <typename T, int CI, int KS>
SR_DEV f32x16 c64_mma(const T* xs, int win, int rw, const C64W<T, KS>& w, f32x16 acc, int lane) {
  constexpr int RS = C64Cfg::rs<T>(CI), CPT = CI / 16;
  const int hh = lane >> 5;
  if constexpr (C64W<T, KS>::REG) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int tap = s / CPT, c = s - tap * CPT;
      acc = mma16<T>(w.get(s, lane), lds_chunk<T>(xs, win + ((tap / 3) * rw + (tap % 3)) * RS + c * 16 + hh * 8), acc);
    }
  } else {                                             // fp32: one tap per iteration, so the fragment loads are not all hoisted
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int row = win + ((tap / 3) * rw + (tap % 3)) * RS;
#pragma unroll
      for (int c = 0; c < CPT; ++c) acc = mma16<T>(w.get(tap * CPT + c, lane), lds_chunk<T>(xs, row + c * 16 + hh * 8), acc);
    }
  }
  return acc;
}

// ---------------------------------------------------------------------------------------------
// one conv: y = act(conv3x3(x) + b) [+ res], 64 output channels.  grid = (tiles, N), 8 waves.  `res` may alias `y` (each
// workgroup reads the residual only at the pixels it writes).
// DZ != 0 (backward-data: the conv of the flipped, transposed weights): the input is staged as x * act'(mask), act = DZ (1 ReLU,
// 2 LeakyReLU).  SAVE (training forward of the gathered first conv): the core of the gathered tile is also written to warp.x0_save.
// ---------------------------------------------------------------------------------------------
template <typename T, int CI, int ACT, bool ADD, bool WARP, int DZ = 0, bool SAVE = false>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void c64_conv_kernel(const T* __restrict__ x, const T* res, T* y,
                                                                  const T* __restrict__ wblob_, int H, int W, int tiles_x,
                                                                  C64WarpSrc<T> warp, C3Dir dir, const T* __restrict__ mask) {
  static_assert(!WARP || CI == 80, "the gathered input is the 80-channel state | frame row");
  static_assert(DZ == 0 || (CI == 64 && !WARP), "the masked staging reads a 64-channel gradient image");
  static_assert(!SAVE || WARP, "only the gathered input is saved");
  typedef C64Cfg C;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int RS = C::rs<T>(CI), KS = C::ks(CI);
  __shared__ __attribute__((aligned(16))) T xs[C::NPXH * RS];
  const T* const wconv = wblob_ + c3_dir_off(dir, blockIdx.y);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, ch = wave & 1;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  C64W<T, KS> w;
  w.load(wconv, ch, lane);                             // in flight while the tile is staged
  if constexpr (WARP) c64_stage_warp<T>(xs, warp, n, H, W, ty0, tx0, tid);
  else if constexpr (DZ != 0)
    c64_stage_dz<T, DZ>(xs, x + (size_t)n * H * W * CI, mask + (size_t)n * H * W * CI, H, W, ty0 - 1, tx0 - 1, tid);
  else c64_stage<T, CI, C::HW, C::NPXH>(xs, x + (size_t)n * H * W * CI, H, W, ty0 - 1, tx0 - 1, tid);
  __syncthreads();
  if constexpr (SAVE) {
    typedef typename FragOf<T>::type FragT;
    for (int idx = tid; idx < C::TH * C::TW * 10; idx += C::NTHREADS) {
      const int p = idx / 10, c = idx - p * 10, py = p / C::TW, px = p - py * C::TW;
      const int Y = ty0 + py, X = tx0 + px;
      if (Y < H && X < W)
        *reinterpret_cast<FragT*>(warp.x0_save + (((size_t)n * H + Y) * W + X) * 80 + c * 8) =
            *reinterpret_cast<const FragT*>(xs + ((py + 1) * C::HW + px + 1) * RS + c * 8);
    }
  }
  const T* const bias = wconv + 2 * KS * 512;
#pragma unroll 1
  for (int pt = wave >> 1; pt < C::NPT_O; pt += C::NWAVES / 2) {
    const int pc = pt * 32 + r, oy = pc / C::TW, ox = pc - oy * C::TW;
    const f32x16 acc = c64_mma<T, CI, KS>(xs, (oy * C::HW + ox) * RS, C::HW, w, c64_bias<T>(bias, ch, hh), lane);
    const int Y = ty0 + oy, X = tx0 + ox;
    if (Y < H && X < W) {
      const size_t o = (((size_t)n * H + Y) * W + X) * C::CO + 32 * ch + 4 * hh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        HalfT v, rv;
        if (ADD) rv = *reinterpret_cast<const HalfT*>(res + o + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float f = c3_act<ACT>(acc[4 * g + j]);
          if (ADD) f += (float)rv[j];
          v[j] = (T)f;
        }
        *reinterpret_cast<HalfT*>(y + o + 8 * g) = v;
      }
    }
  }
}

// =============================================================================================
// One ResidualBlockNoBN per launch, inference (bf16): x on the tile + 2-pixel halo (20 x 20) in LDS; conv1 + ReLU on the tile +
// 1-pixel halo (18 x 18, 11 pixel tiles) -> t in LDS only (zero outside the image: conv2's padding); conv2 + x on the core
// -> y.  Each wave holds its output half of conv1's weights, then of conv2's, in registers.  Same products in the same order and
// the same bf16 rounding points as c64_conv<ReLU> followed by c64_conv<none, +x>.
// LDS: (400 + 324) rows x 144 B = 104,256 B (one workgroup per CU, 2 waves per SIMD).
// =============================================================================================
template <typename T>
__global__ __launch_bounds__(C64Cfg::NTHREADS) void c64_resblock_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                      const T* __restrict__ w1_, const T* __restrict__ w2_,
                                                                      int H, int W, int tiles_x, C3Dir dir) {
  static_assert(sizeof(T) == 2, "bf16 only (LDS budget)");
  typedef C64Cfg C;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int RS = C::rs<T>(64), KS = C::ks(64);
  __shared__ __attribute__((aligned(16))) T smem[(C::NP2 + C::NPXH) * RS];
  T* const X2 = smem;
  T* const T1 = smem + C::NP2 * RS;
  const T* const w1 = w1_ + c3_dir_off(dir, blockIdx.y);
  const T* const w2 = w2_ + c3_dir_off(dir, blockIdx.y);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, ch = wave & 1;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::TH, tx0 = (tile % tiles_x) * C::TW;
  const size_t img = (size_t)n * H * W * C::CO;
  C64W<T, KS> w;
  w.load(w1, ch, lane);
  c64_stage<T, 64, C::W2, C::NP2>(X2, x + img, H, W, ty0 - 2, tx0 - 2, tid);
  __syncthreads();

  // ---- conv1 + ReLU on the tile + 1-pixel halo -> T1 ----
#pragma unroll 1
  for (int pt = wave >> 1; pt < C::NPT_H; pt += C::NWAVES / 2) {
    const int hp = pt * 32 + r;
    const bool live = hp < C::NPXH;
    const int hpc = live ? hp : 0, hy = hpc / C::HW, hx = hpc - hy * C::HW;
    const f32x16 acc = c64_mma<T, 64, KS>(X2, (hy * C::W2 + hx) * RS, C::W2, w, c64_bias<T>(w1 + 2 * KS * 512, ch, hh), lane);
    if (live) {
      const int Y = ty0 - 1 + hy, X = tx0 - 1 + hx;
      const bool inimg = Y >= 0 && Y < H && X >= 0 && X < W;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        HalfT v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = inimg ? (T)c3_act<1>(acc[4 * g + j]) : (T)0.f;
        *reinterpret_cast<HalfT*>(T1 + hp * RS + 32 * ch + 8 * g + 4 * hh) = v;
      }
    }
  }
  w.load(w2, ch, lane);
  __syncthreads();

  // ---- conv2 + x on the core -> y ----
#pragma unroll 1
  for (int pt = wave >> 1; pt < C::NPT_O; pt += C::NWAVES / 2) {
    const int pc = pt * 32 + r, oy = pc / C::TW, ox = pc - oy * C::TW;
    const f32x16 acc = c64_mma<T, 64, KS>(T1, (oy * C::HW + ox) * RS, C::HW, w, c64_bias<T>(w2 + 2 * KS * 512, ch, hh), lane);
    const int Y = ty0 + oy, X = tx0 + ox;
    if (Y < H && X < W) {
      const size_t o = img + ((size_t)Y * W + X) * C::CO + 32 * ch + 4 * hh;
      const T* xr = X2 + ((oy + 2) * C::W2 + ox + 2) * RS + 32 * ch + 4 * hh;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const HalfT rv = *reinterpret_cast<const HalfT*>(xr + 8 * g);
        HalfT v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (T)(acc[4 * g + j] + (float)rv[j]);
        *reinterpret_cast<HalfT*>(y + o + 8 * g) = v;
      }
    }
  }
}
