// Per-frame video network (models/single_image_model.py Result_Model, the trainers' 'single' model), inference on 32-wide NHWC
// activations (gfx950).  Reference ops replaced, per frame:
//   e = encoder(x);  y_{i+1} = conv2(ReLU(conv1(y_i))) + y_i (Block);  f = conv(y_nb) + e;
//   D = ConvTranspose2d(C, 3, 5, stride 4)(f)  ((4h + 1) x (4w + 1));  out = interpolate(D, size, 'bilinear')
// Activations: [frame][H][W][32] in the hot dtype; the model's C <= 32 channels come first, the rest are exactly zero (zero weight
// rows and columns, zero bias).  The encoder is sr_head_fwd (wdsr_ends.h) with mean = 0.
//
//   fn_block_kernel<T, false>  one Block per launch, one workgroup = one 8 x 32 tile of one frame.  x is staged with a 2-pixel halo
//                              as [pixel][40] (an odd number of 16-byte slots per pixel: conflict-free ds_read_b128 over consecutive
//                              pixels); t = ReLU(conv1(x) + b1) on the 10 x 34 tile + halo lives in LDS only and is ZERO outside the
//                              image (conv2 zero-pads t, not ReLU(b1 + ..)); y = conv2(t) + b2 + x, x taken from the staged tile.
//   fn_block_kernel<T, true>   the body's last conv: one conv on a 1-pixel halo, no ReLU, + e read from a second image.
//   Both are rm_conv_kernel's implicit GEMM (result_block.h) on v_mfma_f32_32x32x16_bf16 (fp32: 8 x v_mfma_f32_32x32x2_f32):
//   A = the conv's 18 packed weight fragments (rows = output channels, k = tap * 32 + ci), loaded once per wave and conv and held in
//   registers for all of the wave's pixel tiles; B = 8 consecutive channels of one staged pixel.  So every MFMA reads exactly one
//   operand from LDS.  The bias is the accumulator's initial value.
//   fn_up_kernel               the phase form of mv_recon.h without its fusion: E (75 rows per LR pixel, a 1 x 1 contraction over the 32
//                              channels) -> D tile (fp32, LDS) -> either D itself ((4h + 1) x (4w + 1), NCHW fp32) or the fixed two-tap
//                              blend (4h + 1) -> 4h with ATen's fp32 weights (mv_lambda), NCHW fp32.
//   fn_up_sized_kernel         the same phases, then the resize of D to ANY (OH, OW) from host-made axis tables (FnResize,
//                              packing.resize_axis): each workgroup blends the outputs whose first taps it owns.  The `hot_resize` route.
// Packed blob (packing.fn_tables), elements of T: conv j at conv_off[j] = 18 fragments (512 each) + 32 biases; the upsampler at
// conv_off[2 nb + 1] = 5 fragments of the 16 x 16 x 32 MFMA (rows r = 25 o + 5 ky + kx) + 3 biases + 5 zeros.  No atomics.
#pragma once
#include "mv_recon.h"

struct FnCfg {
  static constexpr int C = 32, TH = 8, TW = 32, NT = 256, NW = 4, CS = 40, KS = 18;
  static constexpr int CONV_ELEMS = KS * 512 + 32;
  // x with a 2-pixel halo, t with a 1-pixel halo (NTT 32-pixel MFMA tiles, the last one partly past the region)
  static constexpr int XW = TW + 4, XH = TH + 4, NPX = XW * XH;
  static constexpr int TTW = TW + 2, TTH = TH + 2, NPT = TTW * TTH, NTT = (NPT + 31) / 32;
  // the last conv: x with a 1-pixel halo
  static constexpr int LW = TW + 2, LH = TH + 2, NPL = LW * LH;
  // upsampler (MVCfg's geometry at 32 channels, one k-step)
  static constexpr int UTH = 8, UTW = 16, HH = UTH + 2, HWD = UTW + 2, NPH = HH * HWD, NG = (NPH + 15) / 16, NPHP = NG * 16;
  static constexpr int RS = C + 8, EB = 5, ERS = 84, DH = 4 * UTH + 1, DW = 4 * UTW + 1, ND = 3 * DH * DW;
  static constexpr int UP_ELEMS = EB * 512 + 8;
};

// one 3x3 conv tile: 32 output channels x the 32 pixels whose staged top-left tap sits at element offset `base` (per lane)
template <typename T>
SR_DEV f32x16 fn_conv_tile(const typename FragOf<T>::type (&a)[FnCfg::KS], const T* img, int base, int row_stride, int hh, f32x16 acc) {
#pragma unroll
  for (int s = 0; s < FnCfg::KS; ++s) {
    const int tap = s >> 1, dy = tap / 3, dx = tap - 3 * dy;
    acc = mma16<T>(a[s], lds_chunk<T>(img, base + (dy * row_stride + dx) * FnCfg::CS + 16 * (s & 1) + 8 * hh), acc);
  }
  return acc;
}

template <typename T> SR_DEV f32x16 fn_bias_init(const T* __restrict__ bias, int hh) {
  f32x16 c;
#pragma unroll
  for (int i = 0; i < 16; ++i) c[i] = (float)bias[(i & 3) + 8 * (i >> 2) + 4 * hh];
  return c;
}

// x, res, y: the frame stack's base pointers ([frame][H][W][32]); wp: this launch's conv(s) in the blob.  TRAIN (a Block only): the
// tile's core pixels of t go to tsave, and bit c of mask[pixel] = (conv1's fp32 accumulator of channel c > 0), rm_conv_kernel's
// EP_BLOCK form; y is computed by the same instructions either way.
template <typename T, bool LAST, bool TRAIN>
SR_DEV void fn_block_body(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y, const T* __restrict__ wp,
                          T* __restrict__ tsave, uint32_t* __restrict__ mask, int H, int W, int tiles_x) {
  typedef FnCfg C;
  typedef typename FragOf<T>::type FragT;
  typedef typename FragOf<T>::half_type HalfT;
  constexpr int HALO = LAST ? 1 : 2, SW = C::TW + 2 * HALO, NPS = SW * (C::TH + 2 * HALO);
  constexpr int X_ELEMS = NPS * C::CS, T_ELEMS = LAST ? 0 : C::NTT * 32 * C::CS;
  __shared__ __attribute__((aligned(16))) unsigned char fn_smem[(X_ELEMS + T_ELEMS) * sizeof(T)];
  T* const xs = reinterpret_cast<T*>(fn_smem);
  T* const ts = xs + X_ELEMS;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
  const int n = blockIdx.y, ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int ty0 = ty * C::TH, tx0 = tx * C::TW;
  const size_t img = (size_t)n * H * W;
  rm_stage<T, C::C, C::CS, SW, NPS, false, 256>(xs, x + img * C::C, nullptr, H, W, ty0 - HALO, tx0 - HALO, tid);
  __syncthreads();

  FragT a[C::KS];
  if constexpr (!LAST) {
#pragma unroll
    for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(wp, s, lane);
    const f32x16 c1 = fn_bias_init<T>(wp + C::KS * 512, hh);
#pragma unroll 1
    for (int q = wave; q < C::NTT; q += C::NW) {
      const int p = 32 * q + r, pc = p < C::NPT ? p : C::NPT - 1;       // lanes past the region compute a copy of its last pixel
      const int py = pc / C::TTW, px = pc - py * C::TTW;
      const f32x16 acc = fn_conv_tile<T>(a, xs, (py * SW + px) * C::CS, SW, hh, c1);
      const int Y = ty0 - 1 + py, X = tx0 - 1 + px;
      const bool in = Y >= 0 && Y < H && X >= 0 && X < W;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        HalfT v;
        T e0, e1, e2, e3;
        cvt_pair<T>(e0, e1, fmaxf(acc[4 * g], 0.f), fmaxf(acc[4 * g + 1], 0.f));
        cvt_pair<T>(e2, e3, fmaxf(acc[4 * g + 2], 0.f), fmaxf(acc[4 * g + 3], 0.f));
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
        for (int i = 0; i < 16; ++i) mbits |= (acc[i] > 0.f ? 1u : 0u) << ((i & 3) + 8 * (i >> 2) + 4 * hh);
        mbits |= __shfl_xor(mbits, 32);
        if (hh == 0 && in && p < C::NPT && py >= 1 && py <= C::TH && px >= 1 && px <= C::TW) mask[img + (size_t)Y * W + X] = mbits;
      }
    }
    __syncthreads();
  }
  const T* const w2 = LAST ? wp : wp + C::CONV_ELEMS;
#pragma unroll
  for (int s = 0; s < C::KS; ++s) a[s] = load_wfrag<T>(w2, s, lane);
  const f32x16 c2 = fn_bias_init<T>(w2 + C::KS * 512, hh);
  const T* const src = LAST ? xs : ts;
  constexpr int SRW = LAST ? SW : C::TTW;
  const int X = tx0 + r;
#pragma unroll 1
  for (int q = wave; q < C::TH; q += C::NW) {
    const f32x16 acc = fn_conv_tile<T>(a, src, (q * SRW + r) * C::CS, SRW, hh, c2);
    const int Y = ty0 + q;
    if (Y < H && X < W) {
      const size_t pix = img + (size_t)Y * W + X;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c0 = 8 * g + 4 * hh;
        HalfT x4;
        if constexpr (LAST) x4 = *reinterpret_cast<const HalfT*>(res + pix * C::C + c0);
        else x4 = *reinterpret_cast<const HalfT*>(xs + ((q + 2) * SW + r + 2) * C::CS + c0);
        HalfT o4;
        T e0, e1, e2, e3;
        cvt_pair<T>(e0, e1, acc[4 * g] + (float)x4[0], acc[4 * g + 1] + (float)x4[1]);
        cvt_pair<T>(e2, e3, acc[4 * g + 2] + (float)x4[2], acc[4 * g + 3] + (float)x4[3]);
        o4[0] = e0; o4[1] = e1; o4[2] = e2; o4[3] = e3;
        *reinterpret_cast<HalfT*>(y + pix * C::C + c0) = o4;
      }
    }
  }
}

template <typename T, bool LAST>
__global__ void __launch_bounds__(256) fn_block_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                       const T* __restrict__ wp, int H, int W, int tiles_x) {
  fn_block_body<T, LAST, false>(x, res, y, wp, nullptr, nullptr, H, W, tiles_x);
}

// the training forward of one Block: fn_block_kernel<T, false> that also leaves t and the ReLU bit mask behind
template <typename T>
__global__ void __launch_bounds__(256) fn_block_train_kernel(const T* __restrict__ x, T* __restrict__ y, const T* __restrict__ wp,
                                                             T* __restrict__ tsave, uint32_t* __restrict__ mask, int H, int W,
                                                             int tiles_x) {
  fn_block_body<T, false, true>(x, nullptr, y, wp, tsave, mask, H, W, tiles_x);
}

// Output size and axis tables of the sized upsampler kernels (packing.resize_axis, one pair per axis, built on the host):
// ty = i0 [OH] | lo [4H + 1] | hi [4H + 1] (int), ly = lam [OH]; tx, lx the same over OW and 4W + 1.  Output d reads D rows i0[d] and
// min(i0[d] + 1, 4H) with weights 1 - lam[d], lam[d]; [lo[i], hi[i]] are the outputs with i0 == i (empty: hi = lo - 1).
struct FnResize {
  const int* ty;
  const float* ly;
  const int* tx;
  const float* lx;
  int OH, OW;
};

// the upsampler's first two phases: f with a 1-pixel halo -> cs, E = W f of the tile's NPH pixels -> es; ends synchronised
template <typename T>
SR_DEV void fn_up_stage_e(const T* __restrict__ fi, const T* __restrict__ blob, T* __restrict__ cs, float* __restrict__ es, int H, int W,
                          int ty0, int tx0) {
  typedef FnCfg C;
  typedef typename FragOf<T>::type FragT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l16 = lane & 15, q = lane >> 4;
  for (int idx = tid; idx < C::NPHP * 4; idx += C::NT) {
    const int p = idx >> 2, cc = idx & 3;
    const int hy = p / C::HWD, hx = p - hy * C::HWD;
    const int Y = ty0 - 1 + hy, X = tx0 - 1 + hx;
    FragT v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (T)0.f;
    if (p < C::NPH && Y >= 0 && Y < H && X >= 0 && X < W) v = *reinterpret_cast<const FragT*>(fi + ((size_t)Y * W + X) * C::C + cc * 8);
    *reinterpret_cast<FragT*>(cs + p * C::RS + cc * 8) = v;
  }
  __syncthreads();
  FragT wl[C::EB];
#pragma unroll
  for (int eb = 0; eb < C::EB; ++eb) wl[eb] = load_wfrag<T>(blob, eb, lane);
#pragma unroll 1
  for (int g = wave; g < C::NG; g += C::NW) {
    const int p = g * 16 + l16;
    const FragT b = lds_chunk<T>(cs, p * C::RS + 8 * q);
#pragma unroll
    for (int eb = 0; eb < C::EB; ++eb) {
      const f32x4 e = vr_mma32<T>(wl[eb], b, f32x4{0.f, 0.f, 0.f, 0.f});
      if (p < C::NPH) *reinterpret_cast<f32x4*>(es + p * C::ERS + 16 * eb + 4 * q) = e;
    }
  }
  __syncthreads();
}

// D[o][dy][dx] of the tile from es: the bias plus the (at most) four LR pixels whose 5 x 5 patches cover it
SR_DEV float fn_up_d(const float* __restrict__ es, float bias, int o, int dy, int dx) {
  typedef FnCfg C;
  const int ly = dy >> 2, i = dy & 3, lx = dx >> 2, j = dx & 3;
  const int p = (ly + 1) * C::HWD + lx + 1;
  float v = bias + es[p * C::ERS + o * 25 + i * 5 + j];
  if (i == 0) v += es[(p - C::HWD) * C::ERS + o * 25 + 20 + j];
  if (j == 0) v += es[(p - 1) * C::ERS + o * 25 + i * 5 + 4];
  if (i == 0 && j == 0) v += es[(p - C::HWD - 1) * C::ERS + o * 25 + 24];
  return v;
}

// f: [frame][H][W][32]; out: frame n at out + n * out_is, NCHW fp32: (3, 4H, 4W) blended, or (3, 4H + 1, 4W + 1) when WRITE_D
template <typename T, bool WRITE_D>
__global__ __launch_bounds__(256) void fn_up_kernel(const T* __restrict__ f, const T* __restrict__ blob, float* __restrict__ out,
                                                    long out_is, int H, int W, int tiles_x) {
  typedef FnCfg C;
  __shared__ __attribute__((aligned(32))) unsigned char fn_smem[C::NPHP * C::RS * sizeof(T) + C::NPH * C::ERS * 4 + C::ND * 4];
  T* const cs = reinterpret_cast<T*>(fn_smem);
  float* const es = reinterpret_cast<float*>(fn_smem + C::NPHP * C::RS * sizeof(T));
  float* const ds = es + C::NPH * C::ERS;
  const int tid = threadIdx.x;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::UTH, tx0 = (tile % tiles_x) * C::UTW;
  fn_up_stage_e<T>(f + (size_t)n * H * W * C::C, blob, cs, es, H, W, ty0, tx0);
  const float b0 = (float)blob[C::EB * 512], b1 = (float)blob[C::EB * 512 + 1], b2 = (float)blob[C::EB * 512 + 2];
  const int H4 = 4 * H, W4 = 4 * W;
  float* const o_ = out + (size_t)n * out_is;
  for (int idx = tid; idx < C::ND; idx += C::NT) {
    const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
    const int dy = rem / C::DW, dx = rem - dy * C::DW;
    const float v = fn_up_d(es, o == 0 ? b0 : o == 1 ? b1 : b2, o, dy, dx);
    if constexpr (WRITE_D) {
      // row 4 UTH / column 4 UTW of the tile belongs to the next tile, except at the image's bottom / right edge
      const int Y = 4 * ty0 + dy, X = 4 * tx0 + dx;
      const bool mine = (dy < 4 * C::UTH || ty0 + C::UTH >= H) && (dx < 4 * C::UTW || tx0 + C::UTW >= W);
      if (mine && Y <= H4 && X <= W4) o_[((size_t)o * (H4 + 1) + Y) * (W4 + 1) + X] = v;
    } else {
      ds[idx] = v;
    }
  }
  if constexpr (!WRITE_D) {
    __syncthreads();
    const float sy = (float)(H4 + 1) / (float)H4, sx = (float)(W4 + 1) / (float)W4;
    for (int idx = tid; idx < 16 * C::UTH * C::UTW; idx += C::NT) {
      const int oy = idx / (4 * C::UTW), ox = idx - oy * (4 * C::UTW);
      const int Y = 4 * ty0 + oy, X = 4 * tx0 + ox;
      if (Y < H4 && X < W4) {
        const float ly = mv_lambda(Y, sy), lx = mv_lambda(X, sx);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float* const d = ds + (c * C::DH + oy) * C::DW + ox;
          const float top = (1.f - lx) * d[0] + lx * d[1], bot = (1.f - lx) * d[C::DW] + lx * d[C::DW + 1];
          o_[((size_t)c * H4 + Y) * W4 + X] = (1.f - ly) * top + ly * bot;
        }
      }
    }
  }
}

// fn_up_kernel with the resize to any (OH, OW) >= (1, 1) fused: out (3, OH, OW) NCHW fp32, every element written once.  The D tile
// is built in LDS as above; the workgroup then blends every output whose (i0_y, i0_x) lies in the D rows and columns it OWNS:
// WRITE_D's `mine` rule, the tile's 4 UTH x 4 UTW core plus row 4 UTH / column 4 UTW at the image's bottom / right edge.  i0 is
// non-decreasing, so these are the outputs lo[first owned] .. hi[last owned] per axis (none at all when a downscale skips the
// tile), and the second tap min(i0 + 1, 4H) lies inside the 33 x 65 tile.  No second tile is read, nothing is written twice.
template <typename T>
__global__ __launch_bounds__(256) void fn_up_sized_kernel(const T* __restrict__ f, const T* __restrict__ blob, float* __restrict__ out,
                                                          long out_is, int H, int W, int tiles_x, FnResize rz) {
  typedef FnCfg C;
  __shared__ __attribute__((aligned(32))) unsigned char fn_smem[C::NPHP * C::RS * sizeof(T) + C::NPH * C::ERS * 4 + C::ND * 4];
  T* const cs = reinterpret_cast<T*>(fn_smem);
  float* const es = reinterpret_cast<float*>(fn_smem + C::NPHP * C::RS * sizeof(T));
  float* const ds = es + C::NPH * C::ERS;
  const int tid = threadIdx.x;
  const int n = blockIdx.y, tile = blockIdx.x;
  const int ty0 = (tile / tiles_x) * C::UTH, tx0 = (tile % tiles_x) * C::UTW;
  const int H4 = 4 * H, W4 = 4 * W, r0 = 4 * ty0, c0 = 4 * tx0;
  const int r1 = ty0 + C::UTH >= H ? H4 : r0 + 4 * C::UTH - 1, c1 = tx0 + C::UTW >= W ? W4 : c0 + 4 * C::UTW - 1;
  const int* const lo_y = rz.ty + rz.OH;
  const int* const lo_x = rz.tx + rz.OW;
  const int oy0 = lo_y[r0], ny = lo_y[H4 + 1 + r1] - oy0 + 1;
  const int ox0 = lo_x[c0], nx = lo_x[W4 + 1 + c1] - ox0 + 1;
  if (ny <= 0 || nx <= 0) return;                          // the whole workgroup: no output reads this tile first
  fn_up_stage_e<T>(f + (size_t)n * H * W * C::C, blob, cs, es, H, W, ty0, tx0);
  const float b0 = (float)blob[C::EB * 512], b1 = (float)blob[C::EB * 512 + 1], b2 = (float)blob[C::EB * 512 + 2];
  for (int idx = tid; idx < C::ND; idx += C::NT) {
    const int o = idx / (C::DH * C::DW), rem = idx - o * (C::DH * C::DW);
    const int dy = rem / C::DW, dx = rem - dy * C::DW;
    ds[idx] = fn_up_d(es, o == 0 ? b0 : o == 1 ? b1 : b2, o, dy, dx);
  }
  __syncthreads();
  float* const o_ = out + (size_t)n * out_is;
  const size_t plane = (size_t)rz.OH * rz.OW;
  for (int idx = tid; idx < ny * nx; idx += C::NT) {
    const int ry = idx / nx, oy = oy0 + ry, ox = ox0 + idx - ry * nx;
    const int iy = rz.ty[oy], ix = rz.tx[ox];
    const float ly = rz.ly[oy], lx = rz.lx[ox];
    const int sy = iy < H4 ? C::DW : 0, sx = ix < W4 ? 1 : 0;      // the second taps, clamped to D's last row / column
    const float* const d0 = ds + (iy - r0) * C::DW + (ix - c0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* const d = d0 + c * C::DH * C::DW;
      const float top = (1.f - lx) * d[0] + lx * d[sx], bot = (1.f - lx) * d[sy] + lx * d[sy + sx];
      o_[c * plane + (size_t)oy * rz.OW + ox] = (1.f - ly) * top + ly * bot;
    }
  }
}
